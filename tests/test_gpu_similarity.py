"""attentionMode 'GAT_Similarity' on the device (MAGAT_MODE_SIMILARITY).  32 / 64 features on graphs of up to 128 agents and 128
features on 97 .. 105 agents, K = 2 | 3: ONE launch, cosine scores inside gat_small.hip / gat_mid.hip, with the float32 form behind
it as the range guard's predicated re-run (overflow, and rows too small for the f16 planes).  Everything else: cosine scores as KeyQuery scores of normalised operands -
maps GEMM (float32 MFMA), gat_cos_prepare_kernel, then the KeyQuery graph kernels (dense up to their LDS tiles, the generic CSR kernels beyond).
Against the gatsim_* fixtures the real reference made and, at shapes no fixture holds, the float64 restatement that
test_host_similarity.py pins on those fixtures.  WHICH kernels ran is asserted by launch tag."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_paths, load_layer_fixture, load_model_fixture
import gat_route_restatement as rr
from similarity_restatement import similarity_layer

pytestmark = pytest.mark.gpu
ONE_LAUNCH = "gat_layer (one launch)"
LAYER = golden_paths("gatsim_layer_")
MODEL = [p for p in golden_paths("gatsim_model_") if "state_only" not in p]
HEADS2 = golden_paths("gatsim_model_heads2_state_only")
GRAD = golden_paths("gatsim_grad_")


def _ids(paths):
    return [os.path.basename(p)[7:-4] for p in paths]


def _layer(p, G, K, dev, concat=True):
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1, concatenate=concat)
    layer.load_state_dict(p, strict=True)
    return layer.to(dev).eval()


def _random_layer(G, K, seed):
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    torch.manual_seed(seed)
    layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1)
    p = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    return layer, p


def _restate(p, x, S):
    y, aij = similarity_layer(x.numpy(), S.numpy(), p["weight"].numpy(), p["filterWeight"].numpy(), p["bias"].numpy())
    return y, aij


def _status(layer):
    """(flag of the last forward, re-runs so far) of the layer's range guard."""
    import ctypes
    from magat_pathplanning_amd import _native as nat
    st = (ctypes.c_int32 * 2)()
    ws = layer._scratch.workspace
    with torch.cuda.device(ws.device):
        nat.check(nat.lib().magat_gat_read_status(nat.ptr(ws), st, nat.current_stream(ws.device)), "magat_gat_read_status")
    return int(st[0]), int(st[1])


def _small(N, G, K):
    """Shapes of the one-launch cosine forms: gat_small.hip up to 32 agents, gat_mid.hip beyond; the 128-wide form where the float32
    re-run exists (gat_dense_kernel's tiles end at 105 agents)."""
    return K in (2, 3) and ((G in (32, 64) and N <= 128) or (G == 128 and 97 <= N <= 105))


def _assert_route(tc, dense, one_launch=False):
    """One launch of the cosine form of gat_small.hip / gat_mid.hip with the predicated float32 launches behind it (maps GEMM, normalisation, graph
    kernel: tag range_guard); or two launches and the normalisation kernel between them (dense); or the same in front of the
    generic CSR kernels."""
    if one_launch:
        assert tc[ONE_LAUNCH] == 1 and tc["range_guard"] >= 1, tc.counts
        assert tc["gat_maps_gemm"] == 0 and tc["gat_prepare"] == 0 and tc["gat_graph"] == 0 and tc["gso_to_csr"] == 0, tc.counts
        return
    assert tc[ONE_LAUNCH] == 0 and tc["gat_maps_gemm"] == 1 and tc["gat_prepare"] == 1, tc.counts
    if dense:
        assert tc["gat_graph"] == 1 and tc["gso_to_csr"] == 0, tc.counts
    else:
        assert tc["gat_graph"] >= 1 and tc["gso_to_csr"] >= 1, tc.counts


@pytest.mark.parametrize("want_att", [False, True], ids=["default_kernels", "with_attention"])
@pytest.mark.parametrize("path", LAYER, ids=_ids(LAYER))
def test_layer_vs_reference_golden(gpu_device, tag_counts, path, want_att):
    """Every layer fixture: y within 1e-5 max(1, |y|), returnAttentionGSO() within 2e-6; concat and mean (one head: the same
    numbers); Nin < N.  128 features on 128 agents lie beyond gat_dense_kernel's tiles: the CSR kernels."""
    from magat_pathplanning_amd import _native as nat
    z, p = load_layer_fixture(path)
    N, G, K = int(z["N"]), int(z["G"]), int(z["K"])
    x = torch.from_numpy(z["x"]).to(gpu_device)
    S = torch.from_numpy(z["S"]).to(gpu_device)
    dense = bool(nat.lib().magat_gat_dense_supported(N, G, G))
    assert dense == (not (G == 128 and N > 105)) and dense == rr.dense_supported(N, G, G)
    assert bool(nat.lib().magat_gat_one_launch_supported(N, G, G, K, nat.MODE_SIMILARITY, 1)) == _small(N, G, K)
    assert rr.one_launch_supported(N, G, G, K, rr.SIMILARITY, rr.DEFAULT_OPT) == _small(N, G, K)      # (the dispatcher restated)
    one = _small(N, G, K) and not want_att      # (requests for the attention tensor take the two-launch form)
    tol = 1e-5 * max(1.0, float(np.abs(z["y"]).max()))
    for concat in (True, False):
        layer = _layer(p, G, K, gpu_device, concat)
        layer.return_attention = want_att
        layer.addGSO(S)
        with tag_counts() as tc, torch.no_grad():
            y = layer(x)
        _assert_route(tc, dense, one)
        if one:      # the fixtures' agent of norm 1e-12 is zero in f16 planes: it raises the flag, the float32 re-run serves it
            assert _status(layer)[0] == 1
        assert tuple(y.shape) == tuple(z["y"].shape)
        np.testing.assert_allclose(y.cpu().numpy(), z["y"], rtol=0, atol=tol)
        if want_att:
            np.testing.assert_allclose(layer.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)
        else:
            assert layer.aij is None
    if "y_nin" in z.files:
        with torch.no_grad():
            yn = layer(x[:, :, :int(z["nin"])].contiguous())
        np.testing.assert_allclose(yn.cpu().numpy(), z["y_nin"], rtol=0, atol=tol)


def _net(path, dev):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = str(dev)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    return z, cfg, net.to(dev).eval()


@pytest.mark.parametrize("path", MODEL, ids=_ids(MODEL))
def test_model_vs_reference_golden(gpu_device, tag_counts, path):
    z, cfg, net = _net(path, gpu_device)
    net.GFL[0].return_attention = True
    x = torch.from_numpy(z["x"].astype(np.float32)).to(gpu_device)
    S = torch.from_numpy(z["S"].copy()).to(gpu_device)
    with torch.no_grad(), tag_counts() as tc:
        net.addGSO(S)
        got = net(x).cpu().numpy()
    _assert_route(tc, True)
    np.testing.assert_allclose(got, z["logits"], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(S.cpu().numpy(), z["S_after"])
    np.testing.assert_allclose(net.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)


def test_two_head_model_raises_before_any_graph_launch(gpu_device, tag_counts):
    z, cfg, net = _net(HEADS2[0], gpu_device)
    assert str(z["forward_raises"]) == "RuntimeError"
    N = cfg.num_agents
    net.addGSO(torch.zeros(1, N, N, device=gpu_device))
    with tag_counts() as tc:
        with pytest.raises(RuntimeError, match="invalid for input of size"), torch.no_grad():
            net(torch.zeros(1, N, 3, cfg.FOV + 2, cfg.FOV + 2, device=gpu_device))
    assert tc["gat_maps_gemm"] == 0 and tc["gat_graph"] == 0 and tc["gat_prepare"] == 0, tc.counts


def test_range_guard_rerun(gpu_device, tag_counts):
    """N = 128, G = 64, K = 3, |x| ~ 1e5 behind gat_mid.hip's cosine form: the flag is raised and the predicated float32 form (maps
    GEMM, gat_cos_prepare_kernel, gat_dense_kernel) rewrites the output - the restatement's numbers within 2e-5 relative."""
    from magat_pathplanning_amd.synthetic import comm_gso
    B, N, G, K = 3, 128, 64, 3
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, G, N, generator=g) * 3.0e4
    S = comm_gso(B, N, 50, seed=5)
    layer, p = _random_layer(G, K, seed=1)
    y_ref, _ = _restate(p, x, S)
    layer = layer.to(gpu_device).eval()
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad(), tag_counts() as tc:
        y = layer(x.to(gpu_device)).cpu().numpy()
    _assert_route(tc, True, True)
    assert np.isfinite(y).all()
    assert float(np.abs(y - y_ref).max()) <= 2e-5 * max(1.0, float(np.abs(y_ref).max()))
    assert _status(layer) == (1, 1)


@pytest.mark.parametrize("N,G,K,B,f64", [(5, 32, 2, 3, False), (10, 32, 2, 5, True), (20, 64, 3, 6, False), (31, 64, 2, 5, False),
                                         (32, 32, 3, 5, True), (20, 32, 3, 1100, False), (33, 32, 2, 5, False), (64, 64, 3, 5, True),
                                         (65, 32, 3, 5, False), (96, 64, 2, 4, False), (100, 64, 3, 5, False), (128, 32, 2, 5, True),
                                         (97, 128, 3, 4, False), (105, 128, 2, 5, True)])
def test_one_launch_against_the_restatement(gpu_device, tag_counts, N, G, K, B, f64):
    """The cosine forms of gat_small.hip (N <= 32) and gat_mid.hip (every row-tile count, and the 128-wide form) on ordinary inputs: one launch, no re-run (the predicated launches return at once), the
    restatement's numbers within 1e-5 max(1, |y|), both merges the same, twice bit-identical.  Directed GSOs with a diagonal -1,
    a 5e-10 entry, an agent without edges; a zero row of x.  B = 1100: more instances than waves in the grid."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    from magat_pathplanning_amd.synthetic import directed_gso
    g = torch.Generator().manual_seed(N * 5 + G + K)
    x = torch.randn(B, G, N, generator=g) * 0.5
    x[0, :, N // 2] = 0.0
    S = torch.nan_to_num(directed_gso(B, N, min(1.0, 6.0 / N), seed=N + G, dtype=torch.float64 if f64 else torch.float32))
    if N > 4:
        S[0, 3, :] = 0
        S[1, 2, 2] = -1.0
        S[2, N - 1, 0] = 5e-10
    layer, p = _random_layer(G, K, seed=N + K)
    pick = sorted({0, 1, 2, B // 2, B - 1})
    y_ref, _ = _restate(p, x[pick], S[pick])
    layer = layer.to(gpu_device).eval()
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        with tag_counts() as tc:
            y = layer(x.to(gpu_device)).cpu()
        y2 = layer(x.to(gpu_device)).cpu()
    _assert_route(tc, True, True)
    assert _status(layer) == (0, 0)
    assert torch.equal(y, y2)
    assert float(np.abs(y[pick].numpy() - y_ref).max()) <= 1e-5 * max(1.0, float(np.abs(y_ref).max()))
    mean = GraphFilterBatchSimilarityAttentional(G, G, K, 1, concatenate=False)
    mean.load_state_dict(p)
    mean = mean.to(gpu_device).eval()
    mean.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        assert torch.equal(mean(x.to(gpu_device)).cpu(), y)


@pytest.mark.parametrize("N,G", [(32, 64), (100, 32), (100, 128)])
@pytest.mark.parametrize("scale,what", [(3.0e4, "overflow"), (1.0e-3, "underflow")])
def test_range_guard_rerun_overflow_and_underflow(gpu_device, tag_counts, scale, what, N, G):
    """Behind the one-launch cosine form: |x| ~ 1e5 leaves the f16 planes' range, |x| ~ 1e-3 their resolution (the direction of a
    row is lost below a scaled norm of 1 / 8) - either raises the flag, and the predicated float32 form (maps GEMM,
    gat_cos_prepare_kernel, gat_dense_kernel) rewrites the output: the restatement's numbers within 2e-5 relative, the re-run counted
    once; a sane forward afterwards runs no float32 work."""
    from magat_pathplanning_amd.synthetic import comm_gso
    B, K = 3, 3
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, G, N, generator=g) * scale
    S = comm_gso(B, N, 30, seed=5)
    layer, p = _random_layer(G, K, seed=1)
    y_ref, _ = _restate(p, x, S)
    layer = layer.to(gpu_device).eval()
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad(), tag_counts() as tc:
        y = layer(x.to(gpu_device)).cpu().numpy()
    _assert_route(tc, True, True)
    assert np.isfinite(y).all()
    assert float(np.abs(y - y_ref).max()) <= 2e-5 * max(1.0, float(np.abs(y_ref).max()))
    assert _status(layer) == (1, 1)
    x_ok = torch.randn(B, G, N, generator=g) * 0.5
    y_ok_ref, _ = _restate(p, x_ok, S)
    with torch.no_grad():
        y_ok = layer(x_ok.to(gpu_device)).cpu().numpy()
    assert float(np.abs(y_ok - y_ok_ref).max()) <= 1e-5 * max(1.0, float(np.abs(y_ok_ref).max()))
    assert _status(layer) == (0, 1)


def test_many_instances_and_run_to_run(gpu_device, tag_counts):
    """More planning instances than workgroups, twice: bit-identical; five sampled instances against the restatement."""
    from magat_pathplanning_amd.synthetic import comm_gso
    B, N, G, K = 1100, 100, 32, 2
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, G, N, generator=g) * 0.6
    S = comm_gso(B, N, 50, seed=3)
    layer, p = _random_layer(G, K, seed=9)
    layer = layer.to(gpu_device).eval()
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        with tag_counts() as tc:
            y1 = layer(x.to(gpu_device)).cpu()
        y2 = layer(x.to(gpu_device)).cpu()
    _assert_route(tc, True, True)      # (gat_mid.hip's cosine form: more instances than workgroups)
    assert _status(layer) == (0, 0)
    assert torch.equal(y1, y2)
    pick = [0, 255, 256, 777, 1099]
    y_ref, _ = _restate(p, x[pick], S[pick])
    assert float(np.abs(y1[pick].numpy() - y_ref).max()) <= 1e-5 * max(1.0, float(np.abs(y_ref).max()))


@pytest.mark.parametrize("want_att", [False, True], ids=["no_attention", "with_attention"])
@pytest.mark.parametrize("N", [130, 200])
def test_csr_route_beyond_128_agents(gpu_device, tag_counts, N, want_att):
    """Graphs beyond the dense kernels: the structure by edge rule 1 (self-loops; a diagonal -1 cancels one), the generic CSR
    score and hop kernels on the normalised operands."""
    from magat_pathplanning_amd.synthetic import directed_gso
    B, G, K = 2, 32, 3
    g = torch.Generator().manual_seed(N)
    x = torch.randn(B, G, N, generator=g) * 0.5
    x[0, :, 4] = 0.0
    S = torch.nan_to_num(directed_gso(B, N, 8.0 / N, seed=N + 1, dtype=torch.float64))
    S[0, 3, :] = 0
    S[1, :, 5] = 0
    S[1, 9, 9] = -1.0
    S[0, N - 1, 0] = 5e-10
    layer, p = _random_layer(G, K, seed=N + 2)
    y_ref, a_ref = _restate(p, x, S)
    layer = layer.to(gpu_device).eval()
    layer.return_attention = want_att
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad(), tag_counts() as tc:
        y = layer(x.to(gpu_device)).cpu().numpy()
    _assert_route(tc, False)
    assert float(np.abs(y - y_ref).max()) <= 1e-5 * max(1.0, float(np.abs(y_ref).max()))
    if want_att:
        np.testing.assert_allclose(layer.returnAttentionGSO(), a_ref.mean(axis=1), rtol=0, atol=2e-6)


def test_step_plan_and_captured_graph(gpu_device, tag_counts):
    """addGSO(S); model(x) of the N = 10 model fixture: the step plan (second forward) equals the general path, and a captured
    graph, replayed once, gives the eager logits."""
    path = [q for q in MODEL if "n10" in q][0]
    z, cfg, net = _net(path, gpu_device)
    x = torch.from_numpy(z["x"].astype(np.float32)).to(gpu_device)
    S = torch.from_numpy(z["S"].copy()).to(gpu_device)
    sx, sS = x.clone(), S.clone()
    with torch.no_grad():
        net.addGSO(S.clone())
        eager = net(x).clone()
        with tag_counts() as tc:
            net.addGSO(S.clone())
            planned = net(x).clone()
        _assert_route(tc, True)
        assert torch.equal(eager, planned)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(2):
                net.addGSO(sS)
                net(sx)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            net.addGSO(sS)
            out = net(sx)
        sS.copy_(S)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)
    np.testing.assert_allclose(out.cpu().numpy(), z["logits"], rtol=0, atol=1e-4)


def test_training_step_of_the_composite_on_the_device(gpu_device, tag_counts):
    """Under autograd the layer takes the torch composite on the device too (no HIP backward for this mode): float32 against the
    reference's float64 gradients at the tolerance tests/test_train_golden.py applies to the device path (2e-4)."""
    z, p = load_layer_fixture(GRAD[0])
    G, K, tol = int(z["G"]), int(z["K"]), 2e-4
    layer = _layer(p, G, K, gpu_device).train()
    x = torch.from_numpy(z["x"]).float().to(gpu_device).requires_grad_(True)
    layer.addGSO(torch.from_numpy(z["S"]).to(gpu_device))
    with tag_counts() as tc:
        y = layer(x)
        (y * torch.from_numpy(z["wgt"]).float().to(gpu_device)).sum().backward()
    assert tc["gat_graph"] == 0 and tc["gat_maps_gemm"] == 0, tc.counts
    np.testing.assert_allclose(y.detach().cpu().numpy(), z["y"], rtol=0, atol=tol * max(1.0, float(np.abs(z["y"]).max())))
    none = set(str(z["none_grads"]).split(","))
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k == "dx" or k.startswith("g_"))
    grads = {"dx": x.grad}
    grads.update({"g_" + k: v.grad for k, v in layer.named_parameters()})
    for k, g in grads.items():
        if k != "dx" and k[2:] in none:
            assert g is None, k
            continue
        want = z[k]
        np.testing.assert_allclose(g.cpu().numpy(), want, rtol=0, atol=tol * (10 * float(np.abs(want).max()) + 1e-2 * gmax),
                                   err_msg=k)
