"""The fused action head + loss on the device (csrc/head_loss.hip through magat_pathplanning_amd/loss.py) against float64 torch
autograd on the CPU over the same float32 values (tests/head_loss_cases.py): every shape of the table in both loss modes at the
project's gates for float32 FMA kernels, the reference's own LabelSmoothing fixtures, the edge cases of the contract (extreme
logits, one class, an out-of-range target, grad_loss != 1, equal bits run to run), ActionLoss, and the whole model's training step
through net.training_loss."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as tnf

import head_loss_cases as hc
from conftest import golden_paths, load_model_fixture

pytestmark = pytest.mark.gpu
LOSSLS = golden_paths("lossls_")
TRAIN = golden_paths("train_")


def _maxabs(t):
    return float(t.abs().max())


def _close(got, want, gate, floor=0.0, what=""):
    """max|got - want| <= gate * max(floor, max|want|), printed before it is asserted"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err, bound = _maxabs(got - want), gate * max(floor, _maxabs(want))
    print("%-8s err %.3e  bound %.3e" % (what, err, bound))
    assert torch.isfinite(got).all(), what
    assert err <= bound, (what, err, bound)


def _check(ref, logits, loss, dX, dW, db):
    _close(logits, ref["logits"], hc.GATE_ROWS, 1.0, "logits")
    _close(loss.reshape(()), ref["loss"], hc.GATE_LOSS, 1.0, "loss")
    _close(dX, ref["dX"], hc.GATE_ROWS, 0.0, "dX")
    _close(dW, ref["dW"], hc.GATE_PARAMS, 0.0, "dW")
    if db is not None:
        _close(db, ref["db"], hc.GATE_PARAMS, 0.0, "db")


def _run(dev, X, W, b, target, smoothing, ldx=None, scale=1.0):
    """head_loss on the device -> (logits, loss, dX, dW, db); ldx: X is the first columns of an (M, ldx) matrix"""
    from magat_pathplanning_amd import head_loss
    M, width = X.shape
    if ldx is None:
        Xd = X.to(dev).requires_grad_(True)
        rows = Xd
    else:
        Xd = torch.randn(M, ldx, generator=torch.Generator().manual_seed(1)).to(dev)
        Xd[:, :width] = X.to(dev)
        Xd.requires_grad_(True)
        rows = Xd[:, :width]
    Wd = W.to(dev).requires_grad_(True)
    bd = None if b is None else b.to(dev).requires_grad_(True)
    loss, logits = head_loss(rows, Wd, bd, target.to(dev), smoothing)
    (loss * scale if scale != 1.0 else loss).backward()
    dX = Xd.grad
    if ldx is not None:
        assert not dX[:, width:].any()
        dX = dX[:, :width]
    return logits, loss, dX, Wd.grad, None if bd is None else bd.grad


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
@pytest.mark.parametrize("shape", hc.SHAPES, ids=[hc.shape_id(s) for s in hc.SHAPES])
def test_head_loss_matches_float64(gpu_device, tag_counts, shape, mode_key):
    (X, W, b, target), ref = hc.case(shape, mode_key)
    with tag_counts() as tc:
        logits, loss, dX, dW, db = _run(gpu_device, X, W, b, target, mode_key[1], ldx=shape[2])
    assert tc["head_loss"] == 2                     # the fused forward and the fused backward, not the composite
    assert not logits.requires_grad
    _check(ref, logits, loss, dX, dW, db)


@pytest.mark.parametrize("path", LOSSLS, ids=[os.path.basename(p)[:-4] for p in LOSSLS])
def test_head_loss_reproduces_the_references_label_smoothing(gpu_device, tag_counts, path):
    z = np.load(path, allow_pickle=False)
    X, W, b = (torch.from_numpy(z[k]).float() for k in ("X", "W", "b"))
    ref = {k: torch.from_numpy(np.asarray(z[k])) for k in ("logits", "loss", "dX", "dW", "db")}
    with tag_counts() as tc:
        out = _run(gpu_device, X, W, b, torch.from_numpy(z["target"]), float(z["smoothing"]))
    assert tc["head_loss"] == 2
    _check(ref, *out)


def _raw_forward(dev, X, W, b, target, mode, smoothing):
    """magat_head_loss_forward_f32 itself -> (logits, dlogits, row_loss, loss)"""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    M, width = X.shape
    X, W, b, target = X.to(dev).contiguous(), W.to(dev).contiguous(), b.to(dev).contiguous(), target.to(dev).contiguous()
    logits = torch.empty(M, 5, device=dev)
    dlogits = torch.empty(M, 5, device=dev)
    row_loss = torch.empty(M, device=dev)
    loss = torch.empty((), device=dev)
    ws = torch.empty(lib.magat_head_loss_workspace_floats(M, width), device=dev)
    with torch.cuda.device(dev):
        nat.check(lib.magat_head_loss_forward_f32(nat.ptr(X), width, nat.ptr(W), nat.ptr(b), nat.ptr(target), mode, smoothing,
                                                  nat.ptr(logits), nat.ptr(dlogits), nat.ptr(row_loss), nat.ptr(loss), nat.ptr(ws),
                                                  M, width, nat.current_stream(dev)), "magat_head_loss_forward_f32")
    torch.cuda.synchronize()
    return logits, dlogits, row_loss, loss


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
def test_extreme_logits_stay_finite(gpu_device, mode_key):
    X, W, b, target = hc.extreme_inputs()
    ref = hc.reference(X, W, b, target, *mode_key)
    assert _maxabs(ref["logits"]) > 9990 and float(ref["logits"].min()) < -9990
    logits, dlogits, row_loss, loss = _raw_forward(gpu_device, X, W, b, target, *mode_key)
    assert torch.isfinite(dlogits).all() and torch.isfinite(row_loss).all() and torch.isfinite(loss)
    _close(dlogits, ref["dlogits"], hc.GATE_ROWS, 0.0, "dlogits")
    _check(ref, *_run(gpu_device, X, W, b, target, mode_key[1]))


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
def test_all_targets_in_one_class(gpu_device, mode_key):
    X, W, b, _ = hc.make_inputs(65, 36, 21)
    target = torch.full((65,), 3, dtype=torch.int64)
    _check(hc.reference(X, W, b, target, *mode_key), *_run(gpu_device, X, W, b, target, mode_key[1]))


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
@pytest.mark.parametrize("bad", [5, -1, 2 ** 40], ids=["five", "minus-one", "huge"])
def test_out_of_range_target_poisons_its_own_row_only(gpu_device, mode_key, bad):
    X, W, b, target = hc.make_inputs(65, 36, 22)
    clean = _raw_forward(gpu_device, X, W, b, target, *mode_key)
    t2 = target.clone()
    t2[40] = bad
    logits, dlogits, row_loss, loss = _raw_forward(gpu_device, X, W, b, t2, *mode_key)
    keep = torch.arange(65) != 40
    assert torch.isnan(dlogits[40]).all() and torch.isnan(row_loss[40]) and torch.isnan(loss)
    assert torch.equal(dlogits.cpu()[keep], clean[1].cpu()[keep]) and torch.equal(row_loss.cpu()[keep], clean[2].cpu()[keep])
    assert torch.equal(logits, clean[0]) and torch.isfinite(clean[3])


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
def test_grad_loss_scales_all_three_gradients(gpu_device, mode_key):
    X, W, b, target = hc.make_inputs(65, 132, 23)
    ref3 = hc.reference(X, W, b, target, *mode_key, grad_scale=3.0)
    ref1 = hc.reference(X, W, b, target, *mode_key)
    for k in ("dX", "dW", "db"):
        assert torch.allclose(ref3[k], 3 * ref1[k], rtol=1e-9, atol=0)
    _check(ref3, *_run(gpu_device, X, W, b, target, mode_key[1], scale=3.0))


@pytest.mark.parametrize("shape", [(6400, 128, None), (257, 640, None)], ids=["M6400-w128", "M257-w640"])
def test_forward_and_backward_are_deterministic(gpu_device, shape):
    (X, W, b, target), _ = hc.case(shape, hc.MODES[1])
    first = _run(gpu_device, X, W, b, target, hc.SMOOTHING)
    second = _run(gpu_device, X, W, b, target, hc.SMOOTHING)
    for a, c in zip(first, second):
        assert torch.equal(a, c)


@pytest.mark.parametrize("mode_key", hc.MODES, ids=["ce", "ls"])
@pytest.mark.parametrize("M", [1, 65, 6400])
def test_action_loss_matches_float64(gpu_device, tag_counts, M, mode_key):
    from magat_pathplanning_amd import ActionLoss
    g = torch.Generator().manual_seed(300 + M)
    logits = torch.randn(M, 5, generator=g) * 3.0
    target = torch.randint(0, 5, (M,), generator=g)
    l64 = logits.double().requires_grad_(True)
    want = hc.reference_loss(l64, target, *mode_key)
    (want * 2.0).backward()
    ld = logits.to(gpu_device).requires_grad_(True)
    assert ld.stride(0) == 5
    with tag_counts() as tc:
        loss = ActionLoss(mode_key[1])(ld, target.to(gpu_device))
        (loss * 2.0).backward()
        with torch.no_grad():
            plain = ActionLoss(mode_key[1])(ld.detach(), tnf.one_hot(target, 5).to(gpu_device))
    assert tc["head_loss"] == 2
    assert torch.equal(plain, loss.detach())
    _close(loss, want.detach(), hc.GATE_LOSS, 1.0, "loss")
    _close(ld.grad, l64.grad, hc.GATE_ROWS, 0.0, "dlogits")


# ---- the whole model -------------------------------------------------------------------------------------------------------------
def _model(path, dev):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    z, sd, cfg = load_model_fixture(path)
    cfg.device = str(dev)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net = net.to(device=dev, dtype=torch.float32).train()
    x = torch.from_numpy(z["x"]).to(device=dev, dtype=torch.float32)
    return z, net, x, torch.from_numpy(z["S"]).to(dev), torch.from_numpy(z["target"]).to(dev)


@pytest.mark.parametrize("path", TRAIN, ids=[os.path.basename(p)[:-4] for p in TRAIN])
def test_training_loss_on_the_hip_path_matches_the_reference(gpu_device, tag_counts, monkeypatch, path):
    """net.training_loss against the REFERENCE's own training step at test_train_golden.py's gate, on the fused entry points; its
    loss and head gradients against the net(x) + cross_entropy route on the same weights at the head's gates."""
    from test_train_golden import _check as check_step
    monkeypatch.setenv("MAGAT_TRAIN_CNN", "hip")
    z, net, x, S, tgt = _model(path, gpu_device)
    plain = copy.deepcopy(net)
    net.addGSO(S.clone())
    with tag_counts() as tc:
        loss, logits = net.training_loss(x, tgt)
        loss.backward()
    assert tc["head_loss"] == 2
    check_step(z, net, logits, loss, 2e-4)
    plain.addGSO(S.clone())
    with tag_counts() as tc:
        want_logits = plain(x)
        want = tnf.cross_entropy(want_logits, tgt)
        want.backward()
    assert tc["head_loss"] == 0
    _close(logits, want_logits, hc.GATE_ROWS, 1.0, "logits")
    _close(loss, want, hc.GATE_LOSS, 1.0, "loss")
    _close(net.actionsMLP[0].weight.grad, plain.actionsMLP[0].weight.grad, hc.GATE_PARAMS, 0.0, "dW")
    _close(net.actionsMLP[0].bias.grad, plain.actionsMLP[0].bias.grad, hc.GATE_PARAMS, 0.0, "db")


def test_the_dropout_head_keeps_the_composite_in_training_and_takes_action_loss_in_eval(gpu_device, tag_counts):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    torch.manual_seed(4)
    net = DecentralPlannerGATNet(make_config(num_agents=5, use_dropout=True, device=str(gpu_device))).to(gpu_device).train()
    x, S = fov_states(2, 5, seed=1).to(gpu_device), comm_gso(2, 5, 20, seed=2).to(gpu_device)
    tgt = torch.randint(0, 5, (10,)).to(gpu_device)
    net.addGSO(S.clone())
    with tag_counts() as tc:
        loss, logits = net.training_loss(x, tgt, 0.1)
        loss.backward()
    assert tc["head_loss"] == 0 and logits.requires_grad and net.actionsMLP[3].weight.grad is not None
    # (torch's own float32 ops over ten rows: a few float32 roundings of a loss of ~15)
    _close(loss, hc.reference_loss(logits.detach().cpu().double(), tgt.cpu(), 1, 0.1), 1e-5, 1.0, "loss")
    net.eval()
    net.addGSO(S.clone())
    with tag_counts() as tc, torch.no_grad():
        loss, logits = net.training_loss(x, tgt, 0.1)
        want_logits = net(x)
    assert tc["head_loss"] == 1
    assert torch.equal(logits, want_logits)
    _close(loss, hc.reference_loss(logits.cpu().double(), tgt.cpu(), 1, 0.1), hc.GATE_LOSS, 1.0, "loss")
