"""CPU-only checks of the fused action head + loss (csrc/head_loss.hip, magat_pathplanning_amd/loss.py): the entry points are
exported, bound and refuse what they document without a device; the torch composite - the semantic reference of the HIP path -
reproduces the REAL reference's LabelSmoothing fixtures (tools/make_golden_loss.py) and torch's cross-entropy; and
net.training_loss reproduces the reference's training step (tests/golden/train_*.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as tnf

import head_loss_cases as hc
from conftest import golden_paths, load_model_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSLS = golden_paths("lossls_")
TRAIN = golden_paths("train_")
ERR_NULL, BAD_SHAPE, UNSUPPORTED, ERR_WORKSPACE = -5, -1, -2, -3

_BUF = (ctypes.c_float * 4096)()
# a 16-byte aligned host address inside the buffer: the refusals are answered before anything would read it
ONE = ctypes.c_void_p((ctypes.addressof(_BUF) + 15) // 16 * 16)
ENTRIES = ("magat_head_loss_workspace_floats", "magat_head_loss_forward_f32", "magat_head_loss_backward_f32", "magat_action_loss_f32")


def _lib():
    from magat_pathplanning_amd import _native as nat
    return nat.lib()


def _off(p, nbytes):
    return ctypes.c_void_p(p.value + nbytes)


def test_entry_points_are_declared_exported_and_bound_behind_abi_9():
    from magat_pathplanning_amd import _native as nat, build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "head_loss.hip" in build_native.SOURCES
    lib = _lib()
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None
    tag = int(re.search(r"#define MAGAT_TAG_HEAD_LOSS (\d+)", common).group(1))
    assert tag == nat.TAG_HEAD_LOSS == 33 and nat.TAGS[tag] == "head_loss"
    assert int(re.search(r"#define MAGAT_PROF_TAGS_TABLE (\d+)", common).group(1)) == 34
    assert re.search(r"#define MAGAT_PROF_TAGS 26\b", hdr)
    c, ms = ctypes.c_longlong(-1), ctypes.c_double(-1)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0
    assert lib.magat_profile_read(tag + 1, ctypes.byref(c), ctypes.byref(ms)) != 0


def test_the_package_exports_the_loss():
    import magat_pathplanning_amd as pkg
    from magat_pathplanning_amd import loss
    assert pkg.head_loss is loss.head_loss and pkg.ActionLoss is loss.ActionLoss
    assert "head_loss" in pkg.__all__ and "ActionLoss" in pkg.__all__
    for cls in (pkg.DecentralPlannerGATNet, pkg.DecentralPlannerNet, pkg.DecentralPlannerBottleneckNet):
        assert callable(cls.training_loss)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _fwd(X=ONE, ldx=None, W=ONE, b=ONE, target=ONE, mode=0, s=0.0, logits=ONE, dlogits=ONE, row_loss=ONE, loss=ONE, ws=ONE, M=8,
         width=36):
    return _lib().magat_head_loss_forward_f32(X, width if ldx is None else ldx, W, b, target, mode, s, logits, dlogits, row_loss,
                                              loss, ws, M, width, None)


def _bwd(dlogits=ONE, g=ONE, X=ONE, ldx=None, W=ONE, dX=ONE, lddx=None, dW=ONE, db=ONE, ws=ONE, M=8, width=36):
    return _lib().magat_head_loss_backward_f32(dlogits, g, X, width if ldx is None else ldx, W, dX, width if lddx is None else lddx,
                                               dW, db, ws, M, width, None)


def _act(logits=ONE, ld=5, target=ONE, mode=0, s=0.0, dlogits=ONE, row_loss=ONE, loss=ONE, ws=ONE, M=8):
    return _lib().magat_action_loss_f32(logits, ld, target, mode, s, dlogits, row_loss, loss, ws, M, None)


BAD_LOSS = [dict(mode=2), dict(mode=-1), dict(mode=1, s=1.0), dict(mode=1, s=-0.1), dict(mode=0, s=1.5), dict(mode=1, s=float("nan"))]
BAD_WIDTH = [dict(width=6), dict(width=35), dict(width=1028), dict(width=2048)]


def test_forward_argument_checks_answer_before_anything_touches_a_device():
    f = _fwd
    for name in ("X", "W", "target", "logits", "dlogits", "loss", "ws"):
        assert f(**{name: None}) == ERR_NULL, name
    for name in ("M", "width"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -4}) == BAD_SHAPE, name
    for kw in BAD_WIDTH + BAD_LOSS + [dict(ldx=32), dict(ldx=35), dict(width=128, ldx=127)]:
        assert f(**kw) == UNSUPPORTED, kw
        assert f(b=None, row_loss=None, **kw) == UNSUPPORTED, kw          # (the nullable ones do not change the answer)
    assert f(ldx=38) == UNSUPPORTED and f(X=_off(ONE, 4)) == UNSUPPORTED and f(W=_off(ONE, 8)) == UNSUPPORTED      # 16-byte rows
    assert f(ws=_off(ONE, 4)) == ERR_WORKSPACE
    # null, then sizes, then what is not covered
    assert f(X=None, M=0) == ERR_NULL and f(loss=None, width=35) == ERR_NULL and f(M=0, width=35) == BAD_SHAPE
    assert f(width=0, mode=7) == BAD_SHAPE


def test_backward_argument_checks_answer_before_anything_touches_a_device():
    f = _bwd
    for name in ("dlogits", "g", "X", "W", "ws"):
        assert f(**{name: None}) == ERR_NULL, name
    for name in ("M", "width"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -4}) == BAD_SHAPE, name
    for kw in BAD_WIDTH + [dict(ldx=32), dict(lddx=32), dict(width=128, lddx=127), dict(lddx=38), dict(dX=_off(ONE, 4))]:
        assert f(**kw) == UNSUPPORTED, kw
        assert f(dW=None, db=None, **kw) == UNSUPPORTED, kw
    assert f(dX=None, dW=None, db=None, ldx=35) == UNSUPPORTED
    assert f(g=None, width=35) == ERR_NULL and f(M=-1, width=35) == BAD_SHAPE


def test_action_loss_argument_checks_answer_before_anything_touches_a_device():
    f = _act
    for name in ("logits", "target", "loss", "ws"):
        assert f(**{name: None}) == ERR_NULL, name
    assert f(M=0) == BAD_SHAPE and f(M=-2) == BAD_SHAPE
    for kw in BAD_LOSS + [dict(ld=4), dict(ld=0), dict(ld=-5)]:
        assert f(**kw) == UNSUPPORTED, kw
        assert f(dlogits=None, row_loss=None, **kw) == UNSUPPORTED, kw
    assert f(ws=_off(ONE, 4)) == ERR_WORKSPACE
    assert f(loss=None, M=0) == ERR_NULL and f(M=0, ld=4) == BAD_SHAPE


def test_workspace_is_zero_for_every_refused_shape_and_covers_both_directions():
    w = _lib().magat_head_loss_workspace_floats
    for M, width in ((0, 36), (-1, 36), (8, 0), (8, -4), (8, 6), (8, 35), (8, 1028)):
        assert w(M, width) == 0, (M, width)
    for M, width, _ in hc.SHAPES:
        blocks = min(128, -(-M // 32))                       # the backward's row chunks: at least 32 rows, at most 128 chunks
        per = -(-M // blocks)
        blocks = -(-M // per)
        assert w(M, width) == max(2 * 1024, blocks * (5 * width + 8)), (M, width)      # 1024 loss partials in double | dW, db partials


# ---- semantics of the composite --------------------------------------------------------------------------------------------------
def test_loss_fixtures_present():
    assert [os.path.basename(p) for p in LOSSLS] == ["lossls_s01.npz", "lossls_s03.npz"]
    for p in LOSSLS:
        z = np.load(p, allow_pickle=False)
        assert sorted(z.files) == sorted(["X", "W", "b", "target", "logits", "loss", "dX", "dW", "db", "smoothing"])
        assert z["X"].shape == (37, 36) and z["W"].shape == (5, 36) and set(z["target"].tolist()) == set(range(5))
        assert np.array_equal(z["X"], z["X"].astype(np.float32).astype(np.float64))
        assert os.path.getsize(p) < 64 << 10


@pytest.mark.parametrize("path", LOSSLS, ids=[os.path.basename(p)[:-4] for p in LOSSLS])
@pytest.mark.parametrize("onehot", [False, True], ids=["indices", "onehot"])
def test_composite_reproduces_the_references_label_smoothing(path, onehot):
    from magat_pathplanning_amd import head_loss
    z = np.load(path, allow_pickle=False)
    X, W, b = (torch.from_numpy(z[k]).requires_grad_(True) for k in ("X", "W", "b"))
    target = torch.from_numpy(z["target"])
    if onehot:
        target = tnf.one_hot(target, 5).double()
    loss, logits = head_loss(X, W, b, target, float(z["smoothing"]))
    loss.backward()
    assert not logits.requires_grad
    for got, key in ((loss, "loss"), (logits, "logits"), (X.grad, "dX"), (W.grad, "dW"), (b.grad, "db")):
        np.testing.assert_allclose(got.detach().numpy(), z[key], rtol=0, atol=1e-9, err_msg=key)


@pytest.mark.parametrize("path", LOSSLS, ids=[os.path.basename(p)[:-4] for p in LOSSLS])
def test_action_loss_composite_and_the_tests_own_reference_agree_with_the_fixture(path):
    from magat_pathplanning_amd import ActionLoss
    z = np.load(path, allow_pickle=False)
    s = float(z["smoothing"])
    logits = torch.from_numpy(z["logits"]).requires_grad_(True)
    target = torch.from_numpy(z["target"])
    loss = ActionLoss(s)(logits, target)
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-9
    # head_loss_cases.reference (what the GPU tests compare with) against the real reference's numbers
    ref = hc.reference(torch.from_numpy(z["X"]), torch.from_numpy(z["W"]), torch.from_numpy(z["b"]), target, 1, s)
    for key in ("loss", "logits", "dX", "dW", "db"):
        np.testing.assert_allclose(ref[key].numpy(), z[key], rtol=0, atol=1e-9, err_msg=key)
    loss.backward()
    np.testing.assert_allclose(logits.grad.numpy(), ref["dlogits"].numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_composite_without_smoothing_is_torch_cross_entropy_exactly(dtype):
    from magat_pathplanning_amd import ActionLoss, head_loss
    X, W, b, target = (t.to(dtype) if t.is_floating_point() else t for t in hc.make_inputs(65, 36, 5))
    leaves = [t.clone().requires_grad_(True) for t in (X, W, b)]
    loss, logits = head_loss(*leaves, target, 0.0)
    loss.backward()
    ref = [t.clone().requires_grad_(True) for t in (X, W, b)]
    want_logits = tnf.linear(*ref)
    want = tnf.cross_entropy(want_logits, target)
    want.backward()
    assert torch.equal(loss, want) and torch.equal(logits, want_logits)
    for a, r in zip(leaves, ref):
        assert torch.equal(a.grad, r.grad)
    assert torch.equal(ActionLoss()(want_logits.detach(), target), want)
    assert torch.equal(ActionLoss(0.0)(want_logits.detach(), tnf.one_hot(target, 5)), want)
    # a width the kernels refuse, a bias-free head and (B, N, 5) one-hot targets take the same composite
    l2, _ = head_loss(X[:, :35], W[:, :35], None, tnf.one_hot(target, 5).view(5, 13, 5), 0.0)
    assert torch.equal(l2, tnf.cross_entropy(tnf.linear(X[:, :35], W[:, :35]), target))


def test_smoothing_outside_the_range_is_refused_and_cpu_tensors_need_the_composite_switch(monkeypatch):
    from magat_pathplanning_amd import ActionLoss, head_loss
    from magat_pathplanning_amd._native import MagatNativeError
    X, W, b, target = hc.make_inputs(8, 36, 3)
    for s in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError):
            head_loss(X, W, b, target, s)
        with pytest.raises(ValueError):
            ActionLoss(s)
    monkeypatch.setenv("MAGAT_ALLOW_TORCH_COMPOSITE", "0")
    with pytest.raises(MagatNativeError):
        head_loss(X, W, b, target)
    with pytest.raises(MagatNativeError):
        ActionLoss()(X[:, :5], target)


# ---- the whole model -------------------------------------------------------------------------------------------------------------
def _training_loss_step(path, label_smoothing=None, config_smoothing="unset"):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = "cpu"
    if config_smoothing != "unset":
        cfg.label_smoothing = config_smoothing
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net = net.double().train()
    x = torch.from_numpy(z["x"]).double()
    tgt = torch.from_numpy(z["target"])
    net.addGSO(torch.from_numpy(z["S"]).clone())
    loss, logits = net.training_loss(x, tgt, label_smoothing)
    return z, net, x, tgt, logits, loss


def test_train_fixtures_have_the_single_linear_head():
    assert len(TRAIN) == 2
    for path in TRAIN:
        _, sd, cfg = load_model_fixture(path)
        assert not cfg.use_dropout and sd["actionsMLP.0.weight"].shape[0] == 5 and "actionsMLP.3.weight" not in sd


@pytest.mark.parametrize("path", TRAIN, ids=[os.path.basename(p)[:-4] for p in TRAIN])
def test_training_loss_reproduces_the_references_training_step_on_the_cpu(path):
    from test_train_golden import _check
    z, net, _, _, logits, loss = _training_loss_step(path)
    assert not logits.requires_grad
    loss.backward()
    _check(z, net, logits, loss, 1e-6)


def test_training_loss_reads_the_configs_label_smoothing():
    path = TRAIN[0]
    z, net, x, tgt, logits, loss = _training_loss_step(path, config_smoothing=None)          # None there means 0
    assert abs(float(loss) - float(z["loss"])) < 1e-6
    for kw in (dict(config_smoothing=0.1), dict(label_smoothing=0.1), dict(label_smoothing=0.1, config_smoothing=0.3)):
        _, net, x, tgt, logits, loss = _training_loss_step(path, **kw)
        want = hc.reference_loss(logits.double(), tgt, 1, 0.1)
        assert abs(float(loss) - float(want)) < 1e-9 * max(1.0, abs(float(want))), kw
        assert float(want) > 2 * float(z["loss"])            # the sum over the rows, not the mean
    # one-hot (B, N, 5) targets, as the reference's loader hands them over
    _, net, x, tgt, logits, loss = _training_loss_step(path)
    B, N = x.shape[:2]
    net.addGSO(torch.from_numpy(z["S"]).clone())
    l2, _ = net.training_loss(x, tnf.one_hot(tgt, 5).view(B, N, 5).double())
    # (train mode: the second forward sees the same batch statistics)
    assert abs(float(l2) - float(loss)) < 1e-12


def test_training_loss_keeps_the_dropout_head_on_the_composite_and_refuses_what_forward_refuses():
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet, DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    cfg = make_config(num_agents=5, use_dropout=True, device="cpu")
    torch.manual_seed(3)
    net = DecentralPlannerGATNet(cfg).double().train()
    x, S = fov_states(2, 5, seed=1).double(), comm_gso(2, 5, 20, seed=2)
    tgt = torch.randint(0, 5, (10,))
    net.addGSO(S.clone())
    torch.manual_seed(11)
    loss, logits = net.training_loss(x, tgt, 0.1)
    assert logits.requires_grad and logits.shape == (10, 5)                 # actionsMLP ran as it is, Dropout included
    assert abs(float(loss) - float(hc.reference_loss(logits.detach(), tgt, 1, 0.1))) < 1e-9
    net.addGSO(S.clone())
    torch.manual_seed(11)
    assert torch.equal(net(x), logits)
    with pytest.raises(TypeError):
        DecentralPlannerGATNet(make_config(num_agents=5, device="cpu")).training_loss(x, tgt)            # addGSO first
    bad = DecentralPlannerBottleneckNet(make_config(num_agents=5, device="cpu", bottleneckMode="BottomNeck_skipAddGNN"))
    bad.addGSO(S.clone())
    with pytest.raises(TypeError, match="SkipAddGNN"):
        bad.training_loss(x, tgt)
