"""attentionMode 'GAT_Similarity' (GraphFilterBatchSimilarityAttentional, MAGAT_MODE_SIMILARITY): host-side checks against the
gatsim_* fixtures the real reference made (tools/make_golden_similarity.py) - no GPU needed."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_paths, load_layer_fixture, load_model_fixture
from similarity_restatement import similarity_layer, similarity_mask

LAYER = golden_paths("gatsim_layer_")
MODEL = [p for p in golden_paths("gatsim_model_") if "state_only" not in p]
HEADS2 = golden_paths("gatsim_model_heads2_state_only")
GRAD = golden_paths("gatsim_grad_")
SHAPES = {(7, 16, 3), (9, 32, 1), (12, 32, 2), (32, 64, 3), (33, 32, 3), (65, 64, 2), (100, 32, 2), (128, 64, 3), (10, 128, 3),
          (97, 128, 2), (128, 128, 3)}
ORDER = ["mixer", "weight_bias", "weight", "filterWeight", "bias"]


def _ids(paths):
    return [os.path.basename(p)[7:-4] for p in paths]


def test_fixture_set_covers_the_issue_matrix():
    assert len(MODEL) == 2 and len(HEADS2) == 1 and len(GRAD) == 1
    shapes, f64, nin = set(), 0, 0
    for path in LAYER:
        z, p = load_layer_fixture(path)
        assert os.path.getsize(path) < 1 << 20
        N = int(z["N"])
        if "y_nin" in z.files:
            nin += 1
            assert int(z["nin"]) == N - 2
        else:
            shapes.add((N, int(z["G"]), int(z["K"])))
        S, x = z["S"][:, 0], z["x"]
        assert S.shape == (2, N, N) and list(p) == ORDER
        f64 += S.dtype == np.float64
        M = similarity_mask(S)
        off = M & ~np.eye(N, dtype=bool)
        assert (~off.any(axis=2) & ~off.any(axis=1)).any(), "an isolated agent"
        assert (off.any(axis=2) & ~off.any(axis=1)).any(), "an agent nobody listens to"
        assert (S == 5e-10).any() and np.isnan(S).any() and (np.diagonal(S, axis1=1, axis2=2) == -1).any()
        assert not np.array_equal(M, M.transpose(0, 2, 1)), "directed"
        norms = np.linalg.norm(x, axis=1)
        assert (norms == 0).any() and ((norms > 0) & (norms < 1e-9)).any()
        for v in p.values():       # bfloat16-representable
            assert torch.equal(v, v.to(torch.bfloat16).float())
    assert shapes == SHAPES and nin == 1 and 0 < f64 < len(LAYER)


@pytest.mark.parametrize("path", LAYER, ids=_ids(LAYER))
def test_restatement_reproduces_the_reference(path):
    z, p = load_layer_fixture(path)
    y, aij = similarity_layer(z["x"], z["S"], p["weight"].numpy(), p["filterWeight"].numpy(), p["bias"].numpy())
    np.testing.assert_allclose(aij, z["aij"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(y, z["y"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("path", LAYER, ids=_ids(LAYER))
def test_cpu_composite_reproduces_the_reference(path):
    """The differentiable torch composite (what every autograd forward of this mode runs), concat and mean, Nin < N."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    z, p = load_layer_fixture(path)
    G, K = int(z["G"]), int(z["K"])
    for concat in (True, False):
        layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1, concatenate=concat)
        layer.load_state_dict(p, strict=True)
        layer.return_attention = True
        layer.addGSO(torch.from_numpy(z["S"]))
        y = layer(torch.from_numpy(z["x"]))
        np.testing.assert_allclose(y.detach().numpy(), z["y"], rtol=0, atol=5e-6)
        np.testing.assert_allclose(layer.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)
        if "y_nin" in z.files:
            yn = layer(torch.from_numpy(z["x"][:, :, :int(z["nin"])].copy()))
            np.testing.assert_allclose(yn.detach().numpy(), z["y_nin"], rtol=0, atol=5e-6)
    assert "attentionMode=GAT_Similarity" in repr(layer)


def test_state_dict_order_shapes_init_and_pickling():
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    torch.manual_seed(3)
    layer = GraphFilterBatchSimilarityAttentional(32, 32, 3, 1)
    assert [(k, tuple(v.shape)) for k, v in layer.state_dict().items()] == [
        ("mixer", (1, 1, 64)), ("weight_bias", (1, 1, 32)), ("weight", (1, 1, 32, 32)), ("filterWeight", (1, 32, 1, 3, 32)),
        ("bias", (32, 1))]
    # graphML.py:4776-4784: draw order weight, (weight_bias = 0,) mixer, filterWeight, bias; U(+-1 / sqrt(G P))
    torch.manual_seed(3)
    stdv = 1.0 / np.sqrt(32.0)
    for name in ("weight", "mixer", "filterWeight", "bias"):
        want = torch.empty_like(getattr(layer, name)).uniform_(-stdv, stdv)
        assert torch.equal(getattr(layer, name).detach(), want), name
    assert float(layer.weight_bias.detach().abs().max()) == 0.0
    assert layer.edge_rule == 1 and layer.attentionMode == "GAT_Similarity"
    assert [k for k, _ in GraphFilterBatchSimilarityAttentional(16, 16, 2, 1, bias=False).state_dict().items()] == ORDER[:4]
    layer.addGSO(torch.zeros(1, 1, 4, 4))
    clone = pickle.loads(pickle.dumps(layer))
    assert clone._scratch.packed is None and clone.aij is None
    for (k1, v1), (k2, v2) in zip(layer.state_dict().items(), clone.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


@pytest.mark.parametrize("path", MODEL + HEADS2, ids=_ids(MODEL + HEADS2))
def test_model_state_dict_keys_in_order_and_shapes(path):
    from magat_pathplanning_amd import DecentralPlannerGATNet, GraphFilterBatchSimilarityAttentional
    z, sd, cfg = load_model_fixture(path)
    cfg.device = "cpu"
    assert cfg.attentionMode == "GAT_Similarity"
    net = DecentralPlannerGATNet(cfg)
    assert isinstance(net.GFL[0], GraphFilterBatchSimilarityAttentional)
    own = net.state_dict()
    assert list(own) == list(sd)
    assert [tuple(v.shape) for v in own.values()] == [tuple(v.shape) for v in sd.values()]
    assert [k for k in own if k.startswith("GFL.0.")] == ["GFL.0." + n for n in ORDER]
    net.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("path", MODEL, ids=_ids(MODEL))
def test_model_cpu_composite_reproduces_reference_logits(path):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = "cpu"
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    net.train(False)
    net.GFL[0].return_attention = True
    S = torch.from_numpy(z["S"].copy())
    net.addGSO(S)
    np.testing.assert_array_equal(S.numpy(), z["S_after"])
    y = net(torch.from_numpy(z["x"].astype(np.float32))).detach().numpy()
    np.testing.assert_allclose(y, z["logits"], rtol=0, atol=5e-6 * max(1.0, float(np.abs(z["logits"]).max())))
    np.testing.assert_allclose(net.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)


def test_composite_gradients_match_reference_made_gradients():
    """float64 composite on the CPU against the reference's autograd, at the tolerances of tests/test_train_golden.py
    (1e-6: outputs to tol * max(1, |y|), gradients to tol * (10 |g| + 1e-2 max |g|)); None where the reference has None."""
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    z, p = load_layer_fixture(GRAD[0])
    G, K, tol = int(z["G"]), int(z["K"]), 1e-6
    layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1)
    layer.load_state_dict(p, strict=True)
    layer = layer.double()
    x = torch.from_numpy(z["x"]).requires_grad_(True)
    layer.addGSO(torch.from_numpy(z["S"]))
    y = layer(x)
    (y * torch.from_numpy(z["wgt"])).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), z["y"], rtol=0, atol=tol * max(1.0, float(np.abs(z["y"]).max())))
    grads = {"dx": x.grad}
    grads.update({"g_" + k: v.grad for k, v in layer.named_parameters()})
    none = set(str(z["none_grads"]).split(","))
    assert none == {"mixer", "weight_bias"}
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k == "dx" or k.startswith("g_"))
    for k, g in grads.items():
        if k[2:] in none and k != "dx":
            assert g is None, k
            continue
        want = z[k]
        np.testing.assert_allclose(g.numpy(), want, rtol=0, atol=tol * (10 * float(np.abs(want).max()) + 1e-2 * gmax), err_msg=k)


def test_pack_torch_follows_the_pack_layout():
    """KeyQuery's layout: rows [0, G) of Bt = W, rows G + k F + f = filterWeight[0, f, 0, k, :], zero column bias."""
    from magat_pathplanning_amd import graphml
    z, p = load_layer_fixture([q for q in LAYER if "N12_G32_K2" in q][0])
    G, K = int(z["G"]), int(z["K"])
    Bt, cb = graphml.pack_torch(p["weight"], p["weight_bias"], p["mixer"], p["filterWeight"], "GAT_Similarity")
    assert tuple(Bt.shape) == (graphml._packed_cols("GAT_Similarity", G, G, K, 1), G) == (G + K * G, G)
    assert torch.equal(Bt[:G], p["weight"][0, 0]) and float(cb.abs().max()) == 0.0 and cb.numel() == G + K * G
    for k in range(K):
        assert torch.equal(Bt[G + k * G:G + (k + 1) * G], p["filterWeight"][0, :, 0, k])
    ref = graphml.pack_torch(p["weight"], None, None, p["filterWeight"], "KeyQuery")
    assert torch.equal(Bt, ref[0])


def test_the_three_refusals():
    from magat_pathplanning_amd import DecentralPlannerGATNet, GraphFilterBatchAttentional, GraphFilterBatchSimilarityAttentional
    from magat_pathplanning_amd.synthetic import make_config
    with pytest.raises(NotImplementedError, match="F == G"):
        GraphFilterBatchSimilarityAttentional(32, 64, 2, 1)
    with pytest.raises(NotImplementedError, match="GraphFilterBatchSimilarityAttentional"):
        GraphFilterBatchAttentional(32, 32, 2, 1, attentionMode="GAT_Similarity")
    for P, E in ((2, 1), (1, 2)):
        layer = GraphFilterBatchSimilarityAttentional(16, 16, 2, P, E)
        layer.addGSO(torch.zeros(1, E, 5, 5))
        with pytest.raises(RuntimeError, match="invalid for input of size"):
            layer(torch.zeros(1, 16, 5))
    layer = GraphFilterBatchSimilarityAttentional(16, 16, 2, 1)
    layer.addGSO(torch.zeros(1, 1, 5, 5))
    layer.storage_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="float32 storage"):
        layer(torch.zeros(1, 16, 5))
    layer = GraphFilterBatchSimilarityAttentional(16, 16, 2, 1, nonlinearity=torch.tanh)
    layer.addGSO(torch.zeros(1, 1, 5, 5))
    with pytest.raises(NotImplementedError, match="ReLU"):
        layer(torch.zeros(1, 16, 5))
    with pytest.raises(NotImplementedError, match="gat_storage"):
        DecentralPlannerGATNet(make_config(num_agents=5, attentionMode="GAT_Similarity", gat_storage="bf16", device="cpu"))


def test_two_head_model_raises_where_the_reference_does():
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(HEADS2[0])
    assert str(z["forward_raises"]) == "RuntimeError" and cfg.nAttentionHeads == 2
    cfg.device = "cpu"
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    N = cfg.num_agents
    net.addGSO(torch.zeros(1, N, N))
    with pytest.raises(RuntimeError, match="invalid for input of size"):
        net(torch.zeros(1, N, 3, cfg.FOV + 2, cfg.FOV + 2))


def test_header_constant_is_bound_and_the_abi_refuses_what_is_not_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import graphml
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert int(re.search(r"#define MAGAT_MODE_SIMILARITY (\d+)", hdr).group(1)) == nat.MODE_SIMILARITY == 4
    assert nat._MODE_IDS["GAT_Similarity"] == graphml._MODES["GAT_Similarity"] == 4
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    # sizes: KeyQuery's pack; the workspaces grow by the B N G floats of the normalised rows (256-byte granules)
    B, N, G, K = 3, 20, 32, 2
    assert lib.magat_gat_packed_floats(G, G, K, 1, 4) == lib.magat_gat_packed_floats(G, G, K, 1, 0)
    grow = (B * N * G * 4 + 255) // 256 * 256
    assert lib.magat_gat_workspace_bytes(B, N, G, G, K, 1, 4, 1) == lib.magat_gat_workspace_bytes(B, N, G, G, K, 1, 0, 1) + grow
    assert lib.magat_gat_csr_workspace_bytes(B, N, 50, G, G, K, 1, 4, 1) == \
        lib.magat_gat_csr_workspace_bytes(B, N, 50, G, G, K, 1, 0, 1) + grow
    assert lib.magat_gat_csc_workspace_bytes(B, N, 50, G, G, K, 1, 4, 1, 0) == \
        lib.magat_gat_csc_workspace_bytes(B, N, 50, G, G, K, 1, 0, 1, 0) + grow
    # one launch: the cosine forms of gat_small.hip / gat_mid.hip - 32 / 64 features up to 128 agents, 128 features on 97 .. 105,
    # K = 2 | 3 (default options: range guard on)
    assert lib.magat_gat_one_launch_supported(N, G, G, K, 4, 1) == 1 and lib.magat_gat_one_launch_supported(32, 64, 64, 3, 4, 0) == 1
    for n, g, k in ((33, 32, 2), (128, 64, 3), (97, 128, 2), (105, 128, 3)):
        assert lib.magat_gat_one_launch_supported(n, g, g, k, 4, 1) == 1, (n, g, k)
    for n, g, k in ((96, 128, 2), (106, 128, 2), (20, 128, 2), (20, 16, 2), (20, 32, 1), (129, 64, 3)):
        assert lib.magat_gat_one_launch_supported(n, g, g, k, 4, 1) == 0, (n, g, k)
    # refusals, decided on the host before any pointer is touched (host dummies: a launch would not survive them)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    assert lib.magat_gat_pack_weights(p, None, None, p, p, G, G, K, 2, 4, None) == -2
    assert lib.magat_gat_pack_weights(p, None, None, p, p, G, 64, K, 1, 4, None) == -2
    assert lib.magat_gat_forward_packed_f32(p, p, 0, p, None, p, 2 * G, None, p, big, B, N, G, G, K, 2, 4, 1, None) == -2
    assert lib.magat_gat_forward_csr_f32(p, p, p, 50, p, None, p, 2 * G, None, p, big, B, N, G, G, K, 2, 4, 1, None) == -2
    assert lib.magat_gat_forward_csr_bf16(p, p, p, 50, p, None, p, G, None, p, big, B, N, G, G, K, 1, 4, 1, None) == -2
    assert lib.magat_gat_forward_csc_bf16(p, p, p, p, p, p, 50, p, None, p, G, None, p, big, B, N, G, G, K, 1, 4, 1, None) == -2
    assert lib.magat_gat_train_forward_f32(p, p, p, 50, p, None, p, p, p, p, p, p, p, p, B, N, G, G, K, 1, 4, None) == -2
    assert lib.magat_gat_train_backward_f32(p, p, p, p, p, p, p, p, p, p, 50, p, p, p, B, N, G, G, K, 1, 4, None) == -2
