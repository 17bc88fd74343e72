"""Training attentionMode 'GAT_Similarity' on the HIP graph kernels: GraphFilterBatchSimilarityAttentional(hip_backward=True) ->
_GatCosTrainFunction -> magat_gat_train_forward_cos_f32 / magat_gat_train_backward_cos_f32 (the KeyQuery training kernels on the
normalised operands, gat_cos_prepare_kernel with its norms output in front, gat_cos_backward_kernel behind).

Yardstick: graphml._composite in float64 on the CPU, inputs and references from tests/similarity_train_cases.py
(tests/test_host_similarity_train.py pins them).  Gate: max|got - want| <= 2e-4 * max(1, max|want|) per tensor, the gate of the
training tests of the other modes.  For dx the clamped rows (|x| or |W x| under 1e-9: gradients near 1e9) are taken out of the
tensor and compared on their own at 2e-4 of their own max|want| - inside the tensor they would set the scale and hide every other
row.  The float32 composite's own error against the float64 one, measured on the CPU
(test_float32_composite_error_stays_far_from_the_gate), is at most 5.3e-7 of that scale over all cases (worst:
long-cat-hubs-B2N130G64K3, weight).  Every case runs twice and must repeat bit for bit (the kernels sum without atomics)."""
import copy
import os

import numpy as np
import pytest
import torch

import similarity_train_cases as sc
from conftest import golden_paths, load_layer_fixture, load_model_fixture

pytestmark = pytest.mark.gpu
NODE = "_GatCosTrainFunctionBackward"
COSGRAD = golden_paths("cosgrad_")


def _ran(fn, name):
    """Is an autograd node called `name` among fn and its ancestors?"""
    seen, todo = set(), [fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if type(f).__name__ == name:
            return True
        todo += [g for g, _ in f.next_functions]
    return False


def _forms():
    from magat_pathplanning_amd import _native as nat
    return nat.lib().magat_form_count(nat.FORMS["gat_cos_train"])


def _device_pass(layer, x, wgt, dev, tag_counts):
    """One forward + backward on the device: the HIP function is in the graph, its launches are tagged, one form count."""
    layer.zero_grad(set_to_none=True)
    xg = x.to(dev).requires_grad_(True)
    before = _forms()
    with tag_counts() as tc:
        y = layer(xg)
        assert _ran(y.grad_fn, NODE)           # the HIP function, not the composite
        (y * wgt.to(dev)).sum().backward()
    assert _forms() == before + 1
    assert tc["gat_graph"] > 0 and tc["gat_maps_gemm"] > 0 and tc["gat_prepare"] > 0, tc.counts
    got = {"y": y.detach(), "dx": xg.grad}
    got.update({n: None if p.grad is None else p.grad.clone() for n, p in layer.named_parameters()})
    return got


@pytest.mark.parametrize("cid", list(sc.CASES))
def test_similarity_training_matches_float64_composite(gpu_device, tag_counts, cid):
    """One forward + backward in train() mode through the HIP training kernels against the float64 composite: y, dx and every
    parameter gradient (mixer, weight_bias: None; weight at K = 1: None or zeros), twice, bit-identical."""
    r = sc.reference(cid)
    k = r.case
    assert r.row_deg >= k.row_deg and r.col_deg >= k.col_deg, (r.row_deg, r.col_deg)       # the input still reaches its branch
    layer = sc.make_layer(k, r.state, hip_backward=True).to(gpu_device).train()
    layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    got = _device_pass(layer, r.x, r.wgt, gpu_device, tag_counts)
    again = _device_pass(layer, r.x, r.wgt, gpu_device, tag_counts)
    assert got["y"].shape == (k.B, k.G, k.nin)
    assert got["mixer"] is None and got["weight_bias"] is None
    sc.compare(cid, got, r.want, r.clamped, again=again)
    if k.clamp:
        assert float(got["dx"][r.clamped.unsqueeze(1).expand_as(got["dx"])].abs().max()) > 1e6
    if k.distinct:                  # every instance has its own graph and input: its own gradient, too
        dx = got["dx"]
        assert all(not torch.equal(dx[a], dx[b]) for a in range(k.B) for b in range(a + 1, k.B))


def _rel(a, b):
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


@pytest.mark.parametrize("path", COSGRAD, ids=[os.path.basename(p)[:-4] for p in COSGRAD])
def test_reference_made_gradients_through_the_hip_path(gpu_device, tag_counts, path):
    """The two reference-made gradient fixtures at widths the kernels take: float32 on the HIP path against the reference's
    float64 numbers, max|got - want| < 2e-4 max|want| per tensor (the rule of tests/test_gpu_train.py), the clamped rows of dx
    apart; None where the reference has None."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    z, p = load_layer_fixture(path)
    G, K = int(z["G"]), int(z["K"])
    layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1, hip_backward=True)
    layer.load_state_dict(p, strict=True)
    layer = layer.to(gpu_device).train()
    layer.addGSO(torch.from_numpy(z["S"]).to(gpu_device))
    got = _device_pass(layer, torch.from_numpy(z["x"]).float(), torch.from_numpy(z["wgt"]).float(), gpu_device, tag_counts)
    none = set(str(z["none_grads"]).split(","))
    assert none == {"mixer", "weight_bias"}
    assert _rel(got["y"].cpu().double(), torch.from_numpy(z["y"])) < 2e-4
    x64 = torch.from_numpy(z["x"]).transpose(1, 2)
    q64 = x64 @ p["weight"][0, 0].double().t()
    clamped = ((x64.norm(dim=2) < 1e-9) | (q64.norm(dim=2) < 1e-9)).unsqueeze(1).expand(-1, G, -1)
    assert clamped.any()
    dx, want = got["dx"].cpu().double(), torch.from_numpy(z["dx"])
    assert _rel(dx[~clamped], want[~clamped]) < 2e-4
    assert _rel(dx[clamped], want[clamped]) < 2e-4 and float(want[clamped].abs().max()) > 1e6
    for name, _ in layer.named_parameters():
        if name in none:
            assert got[name] is None, name
        else:
            assert _rel(got[name].cpu().double(), torch.from_numpy(z["g_" + name])) < 2e-4, name


def _model(path, dev, key):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = str(dev)
    if key:
        cfg.gat_hip_backward = True
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return z, cfg, net.to(dev).train()


def test_model_training_step_with_the_config_key(gpu_device, tag_counts):
    """DecentralPlannerGATNet in train() mode, cross-entropy on random targets, one backward: config.gat_hip_backward = True
    against the same model without the key (the composite on the device) - logits and every parameter gradient within the gate;
    graph kernels are counted only with the key."""
    import torch.nn.functional as tnf
    path = [q for q in golden_paths("gatsim_model_") if "skipconcat_b32_n12_k2" in q][0]
    res = {}
    for key in (True, False):
        z, cfg, net = _model(path, gpu_device, key)
        assert net.GFL[0].hip_backward is key
        x = torch.from_numpy(z["x"].astype(np.float32)).to(gpu_device)
        S = torch.from_numpy(z["S"].copy()).to(gpu_device)
        tgt = torch.randint(0, 5, (x.shape[0] * x.shape[1],), generator=torch.Generator().manual_seed(7)).to(gpu_device)
        before = _forms()
        with tag_counts() as tc:
            net.addGSO(S)
            logits = net(x)
            assert _ran(logits.grad_fn, NODE) == key
            tnf.cross_entropy(logits, tgt).backward()
        if key:
            assert tc["gat_graph"] > 0 and tc["gat_maps_gemm"] > 0 and _forms() == before + 1, tc.counts
        else:
            assert tc["gat_graph"] == 0 and tc["gat_maps_gemm"] == 0 and _forms() == before, tc.counts
        res[key] = (logits.detach().cpu().double(), {n: None if v.grad is None else v.grad.detach().cpu().double()
                                                     for n, v in net.named_parameters()})
    (lh, gh), (lc, gc) = res[True], res[False]
    assert float((lh - lc).abs().max()) <= sc.GATE * max(1.0, float(lc.abs().max()))
    assert gh.keys() == gc.keys()
    for n, want in gc.items():
        if want is None:
            assert gh[n] is None, n
            continue
        err, scale = float((gh[n] - want).abs().max()), max(1.0, float(want.abs().max()))
        assert err <= sc.GATE * scale, (n, err, scale)
    assert gc["GFL.0.weight"] is not None and gc["GFL.0.filterWeight"] is not None and gc["GFL.0.mixer"] is None


def test_default_is_intact(gpu_device, tag_counts):
    """Without the keyword: the composite - no HIP function in the graph, no graph kernel and no form counted."""
    k = sc.CASES["rounds-cat-rounds-B9N10G32K3"]
    r = sc.reference(k.id)
    layer = sc.make_layer(k, r.state).to(gpu_device).train()
    assert layer.hip_backward is False
    layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    xg = r.x.to(gpu_device).requires_grad_(True)
    before = _forms()
    with tag_counts() as tc:
        y = layer(xg)
        (y * r.wgt.to(gpu_device)).sum().backward()
    assert not _ran(y.grad_fn, NODE)
    assert tc["gat_graph"] == 0 and tc["gat_maps_gemm"] == 0 and tc["gat_prepare"] == 0 and _forms() == before, tc.counts
    # ... and with it, return_attention = True keeps the composite too
    layer.hip_backward = True
    layer.return_attention = True
    y = layer(xg)
    assert not _ran(y.grad_fn, NODE) and layer.aij is not None


def test_unsupported_width_raises_the_typed_error(gpu_device):
    """A width the entry points refuse: MagatNativeError naming the limits, no composite takes over, no gradient anywhere."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    from magat_pathplanning_amd import _native as nat
    B, N, G = 2, 6, 8
    layer = GraphFilterBatchSimilarityAttentional(G, G, 2, 1, hip_backward=True).to(gpu_device).train()
    layer.addGSO(sc.tg.gso_rounds(B, N, 5).unsqueeze(1).to(gpu_device))
    xg = (torch.randn(B, G, N, generator=torch.Generator().manual_seed(4)) * 0.6).to(gpu_device).requires_grad_(True)
    with pytest.raises(nat.MagatNativeError, match="8190"):
        layer(xg)
    torch.cuda.synchronize()
    assert xg.grad is None and all(p.grad is None for p in layer.parameters())
