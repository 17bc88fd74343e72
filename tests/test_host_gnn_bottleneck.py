"""DecentralPlannerBottleneckNet (the reference's bottleneck GNN files) and magat_gnn_forward_dense_f32: host-side checks
against the reference-made gnnbn_* fixtures (tools/make_golden_gnn_bottleneck.py) - no GPU needed."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_paths, load_model_fixture

GNNBN = golden_paths("gnnbn_")
RUNNABLE = [p for p in GNNBN if "skipaddgnn" not in os.path.basename(p)]


def test_fixture_set_covers_the_issue_matrix():
    assert len(RUNNABLE) >= 5 and len(GNNBN) == len(RUNNABLE) + 1
    modes, cnns, feats, taps, gso, dropout, big, nan = set(), set(), set(), set(), set(), False, False, False
    for path in RUNNABLE:
        z, sd, cfg = load_model_fixture(path)
        modes.add(cfg.bottleneckMode)
        cnns.add(cfg.CNN_mode)
        feats.add(cfg.bottleneckFeature)
        taps.add(cfg.nGraphFilterTaps)
        gso.add(cfg.GSO_mode)
        dropout |= bool(cfg.use_dropout)
        big |= cfg.num_agents >= 60
        nan |= bool(np.isnan(z["logits"]).any())
        assert os.path.getsize(path) <= 1 << 20
    assert modes == {"BottomNeck_only", "BottomNeck_skipConcat", "BottomNeck_skipConcatGNN"}
    assert {"ResNetLarge_withMLP", "ResNetSlim", "Default"} <= cnns
    assert {32, 128} <= feats and {2, 3} <= taps and {"dist_GSO", "dist_GSO_one"} <= gso
    assert dropout and big and nan


@pytest.mark.parametrize("path", GNNBN, ids=[os.path.basename(p)[:-4] for p in GNNBN])
def test_reference_state_dict_loads_strict_and_module_pickles(path):
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = "cpu"
    net = DecentralPlannerBottleneckNet(cfg)
    net.load_state_dict(sd, strict=True)
    again = pickle.loads(pickle.dumps(net))
    for k, v in again.state_dict().items():
        assert torch.equal(v, sd[k].to(v.dtype)), k
    assert isinstance(net.GFL[1], torch.nn.ReLU) and len(net.GFL) == 2


@pytest.mark.parametrize("path", RUNNABLE, ids=[os.path.basename(p)[:-4] for p in RUNNABLE])
def test_cpu_composite_reproduces_reference_logits(path):
    """Grad-enabled forward on CPU tensors (the differentiable torch composite): the reference's logits, NaN rows included
    (the files other than BottomNeck_only do not scrub the GSO's NaN entry); addGSO mutates the caller's tensor alike."""
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = "cpu"
    net = DecentralPlannerBottleneckNet(cfg)
    net.load_state_dict(sd, strict=True)
    net.train(False)
    x = torch.from_numpy(z["x"].astype(np.float32))
    S = torch.from_numpy(z["S"].copy())
    net.addGSO(S)
    np.testing.assert_array_equal(S.numpy(), z["S_after"])
    for p_ in net.parameters():
        p_.requires_grad_(True)
    y = net(x).detach().numpy()
    ref = z["logits"]
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    np.testing.assert_allclose(y, ref, rtol=0, atol=5e-6 * scale)


def test_skip_add_gnn_builds_and_raises_like_the_reference():
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    path = [p for p in GNNBN if "skipaddgnn" in os.path.basename(p)][0]
    z, sd, cfg = load_model_fixture(path)
    assert str(z["forward_raises"]) == "TypeError"
    cfg.device = "cpu"
    net = DecentralPlannerBottleneckNet(cfg)
    net.load_state_dict(sd, strict=True)
    N = cfg.num_agents
    net.addGSO(torch.zeros(1, N, N))
    with pytest.raises(TypeError, match="SkipAddGNN.py:311"):
        net(torch.zeros(1, N, 3, cfg.FOV + 2, cfg.FOV + 2))


@pytest.mark.parametrize("mode", ["", "None", "BottomNeck_other"])
def test_other_bottleneck_modes_point_to_decentral_planner_net(mode):
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    from magat_pathplanning_amd.synthetic import make_config
    cfg = make_config(num_agents=5, bottleneckMode=mode, device="cpu")
    with pytest.raises(ValueError, match="DecentralPlannerNet"):
        DecentralPlannerBottleneckNet(cfg)


def test_dense_gnn_entry_is_declared_exported_and_tagged():
    from magat_pathplanning_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert re.search(r"\bint magat_gnn_forward_dense_f32\s*\(", hdr)
    assert "magat_gnn_forward_dense_f32" in nat.EXPORTED_SYMBOLS
    para = re.search(r"\* Alignment \(every graph-layer entry point: (.*?)\*/", hdr, flags=re.S).group(1)
    assert "magat_gnn_forward_dense_f32" in para
    assert int(re.search(r"#define MAGAT_TAG_GNN_DENSE (\d+)", hdr).group(1)) == nat.TAG_GNN_DENSE == 25
    assert nat.TAGS[nat.TAG_GNN_DENSE] == "gnn_dense"
    assert int(re.search(r"#define MAGAT_PROF_TAGS (\d+)", hdr).group(1)) == 26
    assert int(re.search(r"#define MAGAT_FORM_GNN_DENSE (\d+)", hdr).group(1)) == nat.FORMS["gnn_dense"] == 15
    assert int(re.search(r"#define MAGAT_FORMS (\d+)", hdr).group(1)) == 16
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    assert lib.magat_form_count(nat.FORMS["gnn_dense"]) >= 0


@pytest.mark.parametrize("N,G,F,K", [(129, 32, 32, 2), (150, 64, 128, 4), (0, 32, 32, 2), (10, 48, 32, 2), (10, 32, 256, 2),
                                     (10, 32, 32, 9), (10, 32, 32, 0)])
def test_dense_gnn_refuses_other_shapes_before_launching(N, G, F, K):
    """Shapes outside 1 <= N <= 128, G, F in {16, 32, 64, 128}, 1 <= K <= 8: MAGAT_ERR_UNSUPPORTED, decided on the host
    before any pointer is touched (the pointers here are host dummies: a launch would not survive them)."""
    import ctypes
    from magat_pathplanning_amd import _native as nat
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = nat.lib().magat_gnn_forward_dense_f32(p, G, p, 0, p, None, p, F, 1, N, max(N, 1), G, F, K, 1, None)
    assert rc == -2
