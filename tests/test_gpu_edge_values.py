"""The GSO's values on the edge structure on the device (csrc/gso_edge_values.hip, GraphEdges.values) and the GNN classes on them:
lambda and the values against the tensor path (batched_gso), numpy's eigenvalues, closed forms and the numpy restatement beyond
batched_gso's 2048 agents; the capacity re-build; GraphFilterBatch, the GNN planners, training and the closed loop on valued edges
against the same on batched_gso's tensor."""
import numpy as np
import pytest
import torch

import edge_values_restatement as ev

pytestmark = pytest.mark.gpu
LAYER_TOL = 1e-5       # |dy| <= 1e-5 max(1, |y|): the layer gate of tests/test_gpu_kernels.py
MODEL_TOL = 1e-4       # the model gate of tests/test_gpu_model.py
TRAIN_TOL = 2e-4       # |d| <= 2e-4 max(1, max |ref|): GraphFilterBatch's training gate (test_graph_filter_batch_backward_matches_autograd)


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def radius_arg(radii, dev):
    """one instance: the number (the entry's comm_radius); a batch: per-instance radii on the device"""
    return float(radii[0]) if len(radii) == 1 else dv(radii, dev)


def valued(pos, radii, sym, dev):
    from magat_pathplanning_amd import batched_edges
    return batched_edges(dv(pos, dev), radius_arg(np.atleast_1d(np.asarray(radii, np.float64)), dev), values=True, symmetric_norm=sym)


def read(edges):
    """-> (structure, nnz, rowptr, colidx, vals, lam) as numpy"""
    st, vals, lam = edges.values()
    nnz = st.exact_nnz()
    torch.cuda.synchronize()
    return st, nnz, st.rowptr.cpu().numpy(), st.colidx[:nnz].cpu().numpy(), vals[:nnz].cpu().numpy(), lam.cpu().numpy()


def close(got, want, rtol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rtol * np.abs(want)).all())


def within(got, want, tol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return bool(((got - want).abs() <= tol * want.abs().clamp(min=1.0)).all())


# ---- 1. lambda and the values against the tensor path ------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
@pytest.mark.parametrize("B,N", [(3, 2), (3, 63), (1, 64), (3, 65), (3, 129), (2, 257), (1, 1025)])
def test_lambda_and_values_equal_the_tensor_path(gpu_device, B, N, sym):
    from magat_pathplanning_amd import batched_gso
    pos, radii = ev.case_positions(B, N)
    edges = valued(pos, radii, sym, gpu_device)
    st, nnz, rowptr, colidx, vals, lam = read(edges)
    S, lam_t = batched_gso(dv(pos, gpu_device), radius_arg(radii, gpu_device), symmetric_norm=sym, dtype=torch.float32, return_lambda=True)
    print("lam", lam, "tensor path", lam_t.cpu().numpy())
    assert close(lam, lam_t.cpu().numpy(), 1e-9)
    if N <= 257:
        for b in range(B):
            M = ev.matrix(pos[b], radii[b], sym)
            want = float(np.linalg.eigvalsh(M)[-1]) if M.any() else 0.0
            assert close(lam[b], want, 1e-9), (b, lam[b], want)
    if B == 3:
        assert lam[1] == 0 and close(lam[2], 1.0 if sym else N - 1.0, 1e-9)      # edgeless, clique
    rows = np.repeat(np.arange(B * N), np.diff(rowptr.reshape(B, N + 1), axis=1).reshape(-1))
    assert len(rows) == nnz == int(np.count_nonzero(S.cpu().numpy()))
    want = S.reshape(B * N, N).cpu().numpy()[rows, colidx]
    # two float64 quotients that differ by <= 1e-9 relative round to float32 numbers at most one ulp apart
    np.testing.assert_allclose(vals, want, rtol=2.0 ** -23, atol=0)
    assert edges.values()[1] is edges.values()[1]                                 # kept until refresh()


# ---- 2. beyond batched_gso ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(64, 64), (33, 63), (62, 66), (63, 65)])
def test_lattices_reach_the_closed_forms(gpu_device, a, b):
    """64 x 64 and 33 x 63: beyond batched_gso.  62 x 66 = 4092 agents is the last size whose tridiagonal matrix stands in LDS (with
    the kernel's static 144 bytes the workgroup's 160 KB are full to the byte), 63 x 65 = 4095 keeps it in the workspace."""
    pos = ev.lattice(a, b)
    want = ev.lattice_lambda(a, b)
    st, nnz, rowptr, colidx, vals, lam = read(valued(pos, 1.2, False, gpu_device))
    print("lattice", a, b, "lam", lam, "closed form", want)
    assert nnz == 2 * (a * (b - 1) + b * (a - 1)) and close(lam[0], want, 1e-9)
    assert (ev.ulps32(vals, np.float32(1.0 / want)) <= 1).all()
    st, nnz, rowptr, colidx, vals, lam = read(valued(pos, 1.2, True, gpu_device))
    print("lattice", a, b, "symmetric lam", lam)
    assert close(lam[0], 1.0, 1e-9)
    deg = np.diff(rowptr)
    rows = np.repeat(np.arange(a * b), deg)
    inv = np.sqrt(1.0 / deg)
    assert (ev.ulps32(vals, ((inv[rows] * inv[colidx]) / 1.0).astype(np.float32)) <= 1).all()


def test_2049_random_cells_against_eigvalsh_and_the_restatement(gpu_device):
    N = 2049
    pos = ev.random_cells(N)
    st, nnz, rowptr, colidx, vals, lam = read(valued(pos, 7.0, False, gpu_device))
    want = float(np.linalg.eigvalsh(ev.matrix(pos[0], 7.0, False))[-1])
    print("2049 cells lam", lam, "eigvalsh", want)
    assert close(lam[0], want, 1e-9)
    for sym in (False, True):
        r = ev.edge_values(pos, 7.0, sym)
        st, nnz, rowptr, colidx, vals, lam = read(valued(pos, 7.0, sym, gpu_device))
        assert nnz == r["nnz"] and np.array_equal(colidx, r["colidx"]) and close(lam, r["lam"], 1e-9)
        assert (ev.ulps32(vals, r["vals"]) <= 1).all()


def test_4093_agents_the_first_size_with_the_tridiagonal_matrix_in_the_workspace(gpu_device):
    """40 N + 16 + 144 bytes of LDS are 163 880 at N = 4093, past the 163 840 of a workgroup: the plan must not ask for them.
    Under symmetric_norm lambda is 1 for any graph with an edge; the values follow from the degrees."""
    N = 4093
    pos = ev.random_cells(N)
    st, nnz, rowptr, colidx, vals, lam = read(valued(pos, 7.0, True, gpu_device))
    print("4093 cells lam", lam, "edges", nnz)
    assert nnz > 2 * N and close(lam[0], 1.0, 1e-9)
    deg = np.diff(rowptr)
    inv = np.where(deg > 0, np.sqrt(1.0 / np.maximum(deg, 1)), 0.0)
    rows = np.repeat(np.arange(N), deg)
    assert (ev.ulps32(vals, (inv[rows] * inv[colidx]).astype(np.float32)) <= 1).all()


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------------
def test_values_follow_a_capacity_rebuild(gpu_device):
    N = 200
    pos = np.stack(np.divmod(np.arange(N), 15), axis=1).astype(np.int32)[None]          # 200 cells within 20 of one another
    edges = valued(pos, 100.0, False, gpu_device)
    assert 32 * N < N * (N - 1)                                                   # the builder's guess is too small
    st, nnz, rowptr, colidx, vals, lam = read(edges)
    assert nnz == N * (N - 1) and st.cap >= nnz
    print("clique lam", lam)
    assert close(lam[0], N - 1.0, 1e-9) and (ev.ulps32(vals, np.float32(1.0 / (N - 1))) <= 1).all()


# ---- 4. the layer --------------------------------------------------------------------------------------------------------------------
def _layer(dev, seed=0):
    from magat_pathplanning_amd import GraphFilterBatch
    torch.manual_seed(seed)
    return GraphFilterBatch(32, 32, 3).to(dev)


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
@pytest.mark.parametrize("B,N", [(2, 130), (1, 1100)])
def test_layer_on_valued_edges_equals_the_layer_on_the_tensor(gpu_device, B, N, sym):
    from magat_pathplanning_amd import batched_gso
    pos, radii = ev.case_positions(B, N)
    layer = _layer(gpu_device).eval()
    x = torch.randn(B, 32, N, generator=torch.Generator().manual_seed(N)).to(gpu_device)
    with torch.no_grad():
        layer.addGSO(batched_gso(dv(pos, gpu_device), radius_arg(radii, gpu_device), symmetric_norm=sym).unsqueeze(1))
        want = layer(x).clone()
        edges = valued(pos, radii, sym, gpu_device)
        layer.addGSO(edges)
        got = layer(x)
    assert layer.S is edges
    print("layer", B, N, sym, "max diff", float((got - want).abs().max()))
    assert within(got, want, LAYER_TOL)


@pytest.mark.parametrize("sym", [False, True], ids=["plain", "symmetric_norm"])
def test_layer_on_a_lattice_of_2079_agents_against_the_float64_composite(gpu_device, sym):
    a, b = 33, 63
    N = a * b
    pos = ev.lattice(a, b)
    lam = 1.0 if sym else ev.lattice_lambda(a, b)
    S = torch.from_numpy((ev.matrix(pos[0], 1.2, sym) / lam).astype(np.float32)).double().view(1, 1, N, N)    # (the layer multiplies by S.float())
    layer = _layer(gpu_device).eval()
    ref = _layer("cpu").double()
    ref.load_state_dict({k: v.double().cpu() for k, v in layer.state_dict().items()})
    x = torch.randn(1, 32, N, generator=torch.Generator().manual_seed(5))
    ref.addGSO(S)
    want = ref(x.double()).detach()                                               # CPU tensors under autograd: the torch composite
    with torch.no_grad():
        layer.addGSO(valued(pos, 1.2, sym, gpu_device))
        got = layer(x.to(gpu_device))
    print("lattice layer", sym, "max diff", float((got.cpu().double() - want).abs().max()))
    assert within(got, want, LAYER_TOL)


# ---- 5. the models -------------------------------------------------------------------------------------------------------------------
def _planner(cls, dev, N, seed=3, **kw):
    from magat_pathplanning_amd.synthetic import make_config
    base = dict(num_agents=N, CNN_mode="Default", bottleneckFeature=32, numInputFeatures=32, nGraphFilterTaps=3, device=str(dev))
    base.update(kw)
    torch.manual_seed(seed)
    return cls(make_config(**base)).to(dev).eval()


def _model_case(dev, B, N):
    from magat_pathplanning_amd.synthetic import fov_states
    pos, _ = ev.case_positions(B, N)
    return pos, fov_states(B, N, seed=N).to(dev)


@pytest.mark.parametrize("N", [130, 20])
@pytest.mark.parametrize("which", ["gnn", "BottomNeck_only", "BottomNeck_skipConcat"])
def test_gnn_planners_on_valued_edges_equal_the_tensor_route(gpu_device, which, N):
    import magat_pathplanning_amd as pkg
    B = 2
    if which == "gnn":
        net = _planner(pkg.DecentralPlannerNet, gpu_device, N)
    else:
        net = _planner(pkg.DecentralPlannerBottleneckNet, gpu_device, N, bottleneckMode=which)
    pos, x = _model_case(gpu_device, B, N)
    with torch.no_grad():
        net.addGSO(pkg.batched_gso(dv(pos, gpu_device), 7.0))
        want = net(x).clone()
        edges = valued(pos, 7.0, False, gpu_device)
        net.addGSO(edges)
        got = net(x)
    if which == "gnn" or N > 128:
        assert net.S is edges                                                     # the CSR route on the structure's arrays
    else:
        assert torch.is_tensor(net.S) and tuple(net.S.shape) == (B, 1, N, N)      # the one-launch dense kernel: edges.gso()
    print("model", which, N, "max diff", float((got - want).abs().max()))
    assert tuple(got.shape) == (B * N, 5) and within(got, want, MODEL_TOL)
    if net.S is edges:                                                            # the attention model's message for a wrong batch
        with pytest.raises(ValueError, match="forward a batch of 1 x %d" % N), torch.no_grad():
            net(x[:1])


def test_dist_gso_one_through_the_model(gpu_device):
    import magat_pathplanning_amd as pkg
    B, N = 2, 130
    net = _planner(pkg.DecentralPlannerNet, gpu_device, N, GSO_mode="dist_GSO_one")
    pos, x = _model_case(gpu_device, B, N)
    for sym in (False, True):
        with torch.no_grad():
            net.addGSO(pkg.batched_gso(dv(pos, gpu_device), 7.0, symmetric_norm=sym))
            want = net(x).clone()
            edges = valued(pos, 7.0, sym, gpu_device)
            net.addGSO(edges)
            got = net(x)
        st, vals, lam = edges.values(normalize=False)
        assert net.S is edges and bool((vals[:st.exact_nnz()] == 1).all()) and bool((lam == 0).all())
        assert within(got, want, MODEL_TOL)


def test_attention_model_treats_valued_edges_like_plain_ones(gpu_device):
    import magat_pathplanning_amd as pkg
    B, N = 2, 130
    net = _planner(pkg.DecentralPlannerGATNet, gpu_device, N, nAttentionHeads=1, bottleneckMode="BottomNeck_only")
    pos, x = _model_case(gpu_device, B, N)
    with torch.no_grad():
        net.addGSO(pkg.batched_edges(dv(pos, gpu_device), 7.0))
        want = net(x).clone()
        net.addGSO(valued(pos, 7.0, True, gpu_device))
        got = net(x)
    assert torch.equal(got, want)


# ---- 6. training ---------------------------------------------------------------------------------------------------------------------
def test_layer_gradients_on_valued_edges_equal_the_tensor_route(gpu_device):
    from magat_pathplanning_amd import batched_gso
    B, N = 2, 130
    pos, radii = ev.case_positions(B, N)
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(B, 32, N, generator=g).to(gpu_device)
    wgt = torch.randn(B, 32, N, generator=g).to(gpu_device)

    def run(graph):
        layer = _layer(gpu_device).train()
        x = x0.clone().requires_grad_(True)
        layer.addGSO(graph)
        y = layer(x)
        assert type(y.grad_fn).__name__ == "_GnnTrainFunctionBackward"
        (y * wgt).sum().backward()
        return y.detach(), x.grad, layer.weight.grad, layer.bias.grad

    want = run(batched_gso(dv(pos, gpu_device), dv(radii, gpu_device), symmetric_norm=True).unsqueeze(1))
    got = run(valued(pos, radii, True, gpu_device))
    for a, b, what in zip(got, want, ("y", "dx", "dweight", "dbias")):
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        print("train", what, err, scale)
        assert err <= TRAIN_TOL * scale, (what, err, scale)


# ---- 7. the closed loop --------------------------------------------------------------------------------------------------------------
def test_episode_values_follow_the_positions(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, batched_gso, generate_cases
    cases = generate_cases(8, 20, 20, 12, density=0.1, complexity=0.05, seed=11, device=gpu_device)
    keep = torch.nonzero(cases["valid"].reshape(-1) != 0).flatten()[:2]
    assert keep.numel() == 2
    maps, start, goal = (cases[k][keep].contiguous() for k in ("map", "start", "goal"))
    ep = BatchedEpisode(maps, start, goal, 20, 4.0, symmetric_norm=True)
    g = torch.Generator(device="cpu").manual_seed(3)
    for step in range(5):
        edges = ep.edges(values=True)
        assert edges is ep.edges(values=True) and edges is not ep.edges() and edges.valued and not ep.edges().valued
        st, nnz, rowptr, colidx, vals, lam = read(edges)
        S, lam_t = batched_gso(ep.pos, ep.radii, symmetric_norm=True, dtype=torch.float32, return_lambda=True)      # ep.gso()'s call
        assert close(lam, lam_t.cpu().numpy(), 1e-9), step
        rows = np.repeat(np.arange(2 * 12), np.diff(rowptr.reshape(2, 13), axis=1).reshape(-1))
        assert nnz == int(np.count_nonzero(S.cpu().numpy()))
        np.testing.assert_allclose(vals, S.reshape(24, 12).cpu().numpy()[rows, colidx], rtol=2.0 ** -23, atol=0)
        ep.step(actions=torch.randint(0, 5, (2, 12), generator=g, dtype=torch.int32).to(gpu_device))
    assert float(ep.radii.min()) >= 4.0 / 1.1


def test_evaluate_cases_on_valued_edges(gpu_device):
    import magat_pathplanning_amd as pkg
    net = _planner(pkg.DecentralPlannerNet, gpu_device, 4, nGraphFilterTaps=2)
    cases = pkg.generate_cases(16, 8, 8, 4, density=0.15, complexity=0.05, seed=31, device=gpu_device)
    keep = torch.nonzero(cases["valid"].reshape(-1) != 0).flatten()[:4]
    assert keep.numel() == 4
    maps, start, goal = (cases[k][keep].contiguous() for k in ("map", "start", "goal"))
    res = pkg.evaluate_cases(net, maps, start, goal, 10, 2, 7.0, poll=4, action_select="soft_max", graph="valued_edges")
    r = {k: v.cpu().numpy() for k, v in res.items()}
    assert (r["retired"] == 1).all() and len(r["steps"]) == 4 and (r["steps"] >= 1).all() and (r["steps"] <= 10).all()
    assert not torch.is_tensor(net.S) and net.S.valued
