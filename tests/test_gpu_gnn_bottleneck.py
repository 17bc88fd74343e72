"""DecentralPlannerBottleneckNet on the HIP path and its graph layer, magat_gnn_forward_dense_f32 (gnn_dense.hip): against the
reference-made gnnbn_* / gnn_* fixtures, the oracle, the CSR entry point, graph capture, weight swaps and training."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden_paths, load_model_fixture

pytestmark = pytest.mark.gpu
TOL = 1e-4            # model tolerance of tests/test_gpu_model.py
GNNBN = [p for p in golden_paths("gnnbn_") if "skipaddgnn" not in os.path.basename(p)]
GNN_FIX = golden_paths("gnn_")


def _net(cfg, sd, dev):
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet
    cfg.device = str(dev)
    net = DecentralPlannerBottleneckNet(cfg)
    if sd is not None:
        net.load_state_dict(sd, strict=True)
    return net.to(dev).eval()


def _cfg(**kw):
    from magat_pathplanning_amd.synthetic import make_config
    base = dict(bottleneckMode="BottomNeck_skipConcat", CNN_mode="Default", bottleneckFeature=32, nGraphFilterTaps=3)
    base.update(kw)
    return make_config(**base)


def _dense(X, ldx, S, w, b, Y, ldy, B, N, Nin, G, F, K, relu):
    from magat_pathplanning_amd import _native as nat
    return nat.lib().magat_gnn_forward_dense_f32(nat.ptr(X), ldx, nat.ptr(S), 1 if S.dtype == torch.float64 else 0, nat.ptr(w),
                                                 nat.ptr(b), ctypes.c_void_p(Y), ldy, B, N, Nin, G, F, K, relu,
                                                 nat.current_stream(X.device))


@pytest.mark.parametrize("path", GNNBN, ids=[os.path.basename(p)[:-4] for p in GNNBN])
def test_model_vs_reference_golden(gpu_device, tag_counts, path):
    z, sd, cfg = load_model_fixture(path)
    net = _net(cfg, sd, gpu_device)
    x = torch.from_numpy(z["x"].astype(np.float32)).to(gpu_device)
    S = torch.from_numpy(z["S"].copy()).to(gpu_device)
    with torch.no_grad():
        net.addGSO(S)
        first = net(x).clone()          # (weights folded, activation scales calibrated)
        with tag_counts() as tc:
            net.addGSO(S)
            logits = net(x)
    got, ref = logits.cpu().numpy(), z["logits"]
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got, first.cpu().numpy(), equal_nan=True)
    ok = ~np.isnan(ref)
    assert float(np.abs(got[ok] - ref[ok]).max()) <= TOL
    np.testing.assert_array_equal(S.cpu().numpy(), z["S_after"])
    assert tc["gnn_dense"] == 1 and tc["gso_to_csr"] == 0, tc.counts


@pytest.mark.parametrize("path", GNN_FIX, ids=[os.path.basename(p)[:-4] for p in GNN_FIX])
def test_dense_kernel_vs_layer_golden(gpu_device, path):
    """The reference GraphFilterBatch outputs (gnn_* fixtures, G != F included) within 1e-5; the N = 150 fixture is refused
    with MAGAT_ERR_UNSUPPORTED and nothing is written."""
    z = np.load(path)
    N, G, F, K = int(z["N"]), int(z["G"]), int(z["F"]), int(z["K"])
    B = z["x"].shape[0]
    X = torch.from_numpy(z["x"]).permute(0, 2, 1).contiguous().to(gpu_device)
    S = torch.from_numpy(z["S"][:, 0].copy()).to(gpu_device)
    w = torch.from_numpy(z["p_weight"]).to(gpu_device).contiguous()
    b = torch.from_numpy(z["p_bias"]).to(gpu_device).contiguous()
    Y = torch.full((B * N, F), -7.0, device=gpu_device)
    rc = _dense(X, G, S, w, b, Y.data_ptr(), F, B, N, N, G, F, K, 0)
    torch.cuda.synchronize()
    if N > 128:
        assert rc == -2
        assert bool((Y == -7.0).all())
        return
    assert rc == 0
    want = z["y"].transpose(0, 2, 1).reshape(B * N, F)
    np.testing.assert_allclose(Y.cpu().numpy(), want, rtol=0, atol=1e-5)


@pytest.mark.parametrize("seed", range(8))
def test_dense_kernel_randomised_vs_oracle_and_csr(gpu_device, seed):
    """K 1..8, float32 / float64 S, Y an odd-offset column block of a wider buffer, Nin < N zero padding, ReLU on / off:
    against oracle.magat_oracle.graph_filter_batch_forward and against GraphFilterBatch's CSR entry point."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import GraphFilterBatch
    rng = np.random.default_rng(100 + seed)
    widths = [16, 32, 64, 128]
    K = seed + 1
    G, F = int(rng.choice(widths)), int(rng.choice(widths))
    N = int(rng.integers(1, 129)) if seed % 3 else int(rng.choice([1, 33, 64, 65, 100, 128]))
    Nin = max(1, N - int(rng.integers(0, 4)))
    B = int(rng.integers(1, 6))
    f64 = seed % 2 == 0
    relu = seed % 3 == 1
    gen = torch.Generator().manual_seed(seed)
    Wadj = (torch.rand(B, N, N, generator=gen) < 0.2).double() * torch.rand(B, N, N, generator=gen).double()
    S = (Wadj / max(1.0, float(Wadj.sum(2).max()))).to(torch.float64 if f64 else torch.float32)
    x = torch.randn(B, G, Nin, generator=gen)
    layer = GraphFilterBatch(G, F, K)
    xp = torch.cat((x, torch.zeros(B, G, N - Nin)), dim=2)
    want = orc.graph_filter_batch_forward(xp, S.unsqueeze(1), layer.weight.detach(), layer.bias.detach())[:, :, :Nin]
    if relu:
        want = torch.relu(want)
    want = want.permute(0, 2, 1).reshape(B * Nin, F).numpy()
    ld = F + 12
    buf = torch.full((B * Nin, ld), -7.0, device=gpu_device)
    X = x.permute(0, 2, 1).contiguous().to(gpu_device).view(B * Nin, G)
    Sd = S.to(gpu_device)
    lg = layer.to(gpu_device)
    w, b = lg.weight.detach().contiguous(), lg.bias.detach().contiguous()
    rc = _dense(X, G, Sd, w, b, buf.data_ptr() + 3 * 4, ld, B, N, Nin, G, F, K, int(relu))
    assert rc == 0
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:, :3] == -7.0).all() and (out[:, 3 + F:] == -7.0).all()
    got = out[:, 3:3 + F]
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5 * scale)
    with torch.no_grad():
        lg.addGSO(Sd.unsqueeze(1))
        csr = lg(x.to(gpu_device))
        if relu:
            csr = torch.relu(csr)
    np.testing.assert_allclose(got, csr.permute(0, 2, 1).reshape(B * Nin, F).cpu().numpy(), rtol=0, atol=1e-5 * scale)


def test_large_graph_falls_back_to_csr_and_matches(gpu_device, tag_counts):
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    B, N = 2, 150
    cfg = _cfg(num_agents=N, bottleneckMode="BottomNeck_skipConcatGNN", nGraphFilterTaps=2)
    torch.manual_seed(3)
    cpu = _net(copy.deepcopy(cfg), None, torch.device("cpu"))
    net = _net(cfg, cpu.state_dict(), gpu_device)
    x, S = fov_states(B, N, seed=4), comm_gso(B, N, 40, seed=5, dtype=torch.float64)
    with torch.no_grad():
        cpu.addGSO(S.clone())
        for p_ in cpu.parameters():
            p_.requires_grad_(True)
    with torch.enable_grad():
        want = cpu(x).detach().numpy()
    with torch.no_grad(), tag_counts() as tc:
        net.addGSO(S.clone().to(gpu_device))
        got = net(x.to(gpu_device)).cpu().numpy()
    assert tc["gnn_dense"] == 0
    assert float(np.abs(got - want).max()) <= TOL


@pytest.mark.parametrize("B,N", [(1, 10), (4, 100)])
def test_graph_capture_replay_matches_eager(gpu_device, B, N):
    """addGSO(S); net(x) captured in a torch.cuda.CUDAGraph: no host synchronisation inside, replays bit-equal to eager on fresh
    inputs (the CSR route's edge count travels to the host, so it cannot be captured)."""
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    cfg = _cfg(num_agents=N, bottleneckMode="BottomNeck_only", CNN_mode="ResNetLarge_withMLP", GSO_mode="dist_GSO_one")
    torch.manual_seed(N)
    net = _net(cfg, None, gpu_device)
    x, S = fov_states(B, N, seed=1).to(gpu_device), comm_gso(B, N, 20 + N // 4, seed=2, dtype=torch.float64).to(gpu_device)
    sx, sS = x.clone(), S.clone()
    with torch.no_grad():
        net.addGSO(S)
        eager = net(x).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                net.addGSO(sS.copy_(S))
                net(sx)
        torch.cuda.current_stream().wait_stream(side)
        sS.copy_(S)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            net.addGSO(sS)
            out = net(sx)
        x2, S2 = fov_states(B, N, seed=7).to(gpu_device), comm_gso(B, N, 20 + N // 4, seed=8, dtype=torch.float64).to(gpu_device)
        sx.copy_(x2); sS.copy_(S2)
        g.replay()
        torch.cuda.synchronize()
        net.addGSO(S2)
        assert torch.equal(out, net(x2))
        sx.copy_(x); sS.copy_(S)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_load_state_dict_between_forwards_is_seen(gpu_device):
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    cfg = _cfg(num_agents=12, bottleneckMode="BottomNeck_skipConcatGNN", CNN_mode="ResNetSlim")
    torch.manual_seed(1)
    net = _net(copy.deepcopy(cfg), None, gpu_device)
    torch.manual_seed(2)
    other = _net(copy.deepcopy(cfg), None, gpu_device)
    x, S = fov_states(2, 12, seed=3).to(gpu_device), comm_gso(2, 12, 16, seed=4).to(gpu_device)
    with torch.no_grad():
        net.addGSO(S)
        a = net(x).clone()
        net.load_state_dict(other.state_dict())
        net.addGSO(S)
        b = net(x).clone()
        other.addGSO(S)
        want = other(x)
    assert not torch.equal(a, b)
    assert float((b - want).abs().max()) <= 1e-6


def test_skip_add_gnn_forward_raises_before_any_launch(gpu_device, tag_counts):
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    net = _net(_cfg(num_agents=6, bottleneckMode="BottomNeck_skipAddGNN"), None, gpu_device)
    with tag_counts() as tc, torch.no_grad():
        net.addGSO(comm_gso(1, 6, 8, seed=1).to(gpu_device))
        with pytest.raises(TypeError, match="SkipAddGNN.py:311"):
            net(fov_states(1, 6, seed=2).to(gpu_device))
    assert not tc.counts


def test_training_forward_and_gradients(gpu_device):
    """Grad-enabled forward (HIP train function of the graph layer, torch ops around it) = the eval logits of the HIP path;
    its gradients = those of a CPU float64 copy of the module (the differentiable composite)."""
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    B, N = 2, 14
    cfg = _cfg(num_agents=N, bottleneckMode="BottomNeck_skipConcat", nGraphFilterTaps=3)
    torch.manual_seed(9)
    net = _net(copy.deepcopy(cfg), None, gpu_device)
    ref = copy.deepcopy(net).cpu().double()
    ref.config = copy.deepcopy(cfg)
    ref.config.device = "cpu"
    x, S = fov_states(B, N, seed=5), comm_gso(B, N, 18, seed=6, dtype=torch.float64)
    with torch.no_grad():
        net.addGSO(S.clone().to(gpu_device))
        want = net(x.to(gpu_device)).clone()
    net.addGSO(S.clone().to(gpu_device))
    y = net(x.to(gpu_device))
    assert y.requires_grad
    assert float((y.detach() - want).abs().max()) <= TOL
    wts = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * wts.to(gpu_device)).sum().backward()
    ref.addGSO(S.clone())
    yr = ref(x.double())
    (yr * wts.double()).sum().backward()
    for (name, p_), (_, q_) in zip(net.named_parameters(), ref.named_parameters()):
        if q_.grad is None:
            assert p_.grad is None or float(p_.grad.abs().max()) == 0.0, name
            continue
        scale = max(1e-3, float(q_.grad.abs().max()))
        err = float((p_.grad.double().cpu() - q_.grad).abs().max())
        assert err <= 2e-4 * scale, (name, err, scale)
