"""The communication graph as an edge structure straight from agent positions (csrc/gso_edges.hip, magat_pathplanning_amd/edges.py;
DESIGN 4.5) on the device: against the numpy restatement (tests/edges_restatement.py), against the existing builder behind
batched_gso's tensor, the capacity protocol, the model bit for bit on both routes, beyond the dense GSO's limits, in the closed
loop, and the entry point's plumbing.  Integer arrays and logits of the same kernels on the same rows: every comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

import edges_restatement as er

pytestmark = pytest.mark.gpu
ARRAYS = ("rowptr", "colidx", "cscptr", "cscsrc", "cscpos")


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def form_count(form="gso_edges"):
    from magat_pathplanning_amd import _native as nat
    return nat.lib().magat_form_count(nat.FORMS[form])


def got_arrays(st, dev):
    nnz = st.ready(dev)
    torch.cuda.synchronize()
    return dict(rowptr=st.rowptr.cpu().numpy(), cscptr=st.cscptr.cpu().numpy(), colidx=st.colidx[:nnz].cpu().numpy(),
                cscsrc=st.csc[0, :nnz].cpu().numpy(), cscpos=st.csc[1, :nnz].cpu().numpy(), nnz=nnz)


def assert_arrays(got, want, what):
    assert got["nnz"] == want["nnz"], (what, got["nnz"], want["nnz"])
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def raw_build(pos, radii, rule, cap, dev, comm_radius=0.0, null_index=False, stream=None):
    """magat_gso_edges_build through the C ABI with buffers of exactly the documented sizes -> (rc, dict of host arrays)"""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    B, N, _ = pos.shape
    rowptr = torch.full((B * (N + 1),), -7, dtype=torch.int32, device=dev)
    cscptr = torch.full((B * (N + 1),), -7, dtype=torch.int32, device=dev)
    idx = [None] * 3 if null_index else [torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    nnz = torch.full((1,), -7, dtype=torch.int64, device=dev)
    ws = torch.empty(max(lib.magat_gso_edges_workspace_bytes(B, N), 8), dtype=torch.uint8, device=dev).fill_(0xA5)
    rc = lib.magat_gso_edges_build(nat.ptr(pos), nat.ptr(radii), float(comm_radius), rule, nat.ptr(rowptr), nat.ptr(idx[0]),
                                   nat.ptr(cscptr), nat.ptr(idx[1]), nat.ptr(idx[2]), cap, nat.ptr(nnz), nat.ptr(ws), ws.numel(), B, N,
                                   stream if stream is not None else nat.current_stream(dev))
    torch.cuda.synchronize()
    out = dict(rowptr=rowptr.cpu().numpy(), cscptr=cscptr.cpu().numpy(), nnz=int(nnz.item()))
    for k, t in zip(("colidx", "cscsrc", "cscpos"), idx):
        out[k] = None if t is None else t.cpu().numpy()
    return rc, out


# ---- 1. equality with the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", er.CASE_N)
def test_edges_equal_the_restatement(gpu_device, N):
    """all five arrays and the count, both rules, B = 1 and 3 with one radius per instance: instance 0 holds a clique of up to 65
    agents on indices 0 .. 64 (rows and columns 63 | 64 of the bit words), the last instance of B = 3 is edgeless at radius 0.5"""
    from magat_pathplanning_amd import batched_edges
    for B in er.CASE_B:
        pos, radii = er.case_positions(B, N)
        pattern = er.edge_pattern(pos, radii, 0)
        if N >= 65:
            assert pattern[0, :65, :65].sum() == 65 * 64                       # the clique
        if B > 1:
            assert not pattern[B - 1].any()                                    # the edgeless instance
        edges = batched_edges(dv(pos, gpu_device), dv(radii, gpu_device))
        before, builds = form_count(), 0
        for rule in (0, 1):
            if rule:
                idx = np.arange(N)
                pattern[:, idx, idx] = True
            want = er.arrays_of_pattern(pattern)
            assert_arrays(got_arrays(edges.structure(rule), gpu_device), want, (B, N, rule))
            # one build, and one more where the graph has more edges than the first guess holds (32 per node, 4096 at least)
            builds += 1 + (want["nnz"] > min(B * N * N, max(32 * B * N, 4096)))
        assert form_count() == before + builds
        if B == 1:                                                             # one radius for all, as a number
            one = batched_edges(dv(pos, gpu_device), float(radii[0]))
            assert_arrays(got_arrays(one.structure(0), gpu_device), er.edge_arrays(pos, radii, 0), (B, N, "number"))


@pytest.mark.parametrize("B,N", [(520, 40), (260, 70), (16, 2049)])
def test_many_instances_take_64_rows_per_workgroup(gpu_device, B, N):
    """B * ceil(N / 64) >= 512: the batches of a closed loop, 64 rows per workgroup instead of 16"""
    from magat_pathplanning_amd import batched_edges
    assert B * ((N + 63) // 64) >= 512
    pos, radii = er.case_positions(B, N)
    radii = 4.0 + 0.01 * np.arange(B)
    edges = batched_edges(dv(pos, gpu_device), dv(radii, gpu_device))
    for rule in (0, 1):
        assert_arrays(got_arrays(edges.structure(rule), gpu_device), er.edge_arrays(pos, radii, rule), (B, N, rule))


# ---- 2. equality with the existing builder for N <= 1024 ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 63, 64, 65, 129, 1000, 1024])
def test_edges_equal_the_builder_behind_batched_gso(gpu_device, N):
    from magat_pathplanning_amd import batched_edges, batched_gso
    from magat_pathplanning_amd.graphml import CsrStructure
    B = 3
    pos, radii = er.case_positions(B, N)
    p, r = dv(pos, gpu_device), dv(radii, gpu_device)
    edges = batched_edges(p, r)
    mine = {rule: got_arrays(edges.structure(rule), gpu_device) for rule in (0, 1)}
    for dtype in (torch.float32, torch.float64):
        for sym in (False, True):
            S = batched_gso(p, r, symmetric_norm=sym, dtype=dtype)
            for rule in (0, 1):
                assert_arrays(mine[rule], got_arrays(CsrStructure().build(S, rule), gpu_device), (N, dtype, sym, rule))


# ---- 3. capacity -------------------------------------------------------------------------------------------------------------------
def test_capacity_contract_and_rebuild(gpu_device):
    from magat_pathplanning_amd import batched_edges
    B, N = 3, 129
    pos, radii = er.case_positions(B, N)
    p, r = dv(pos, gpu_device), dv(radii, gpu_device)
    for rule in (0, 1):
        full = er.edge_arrays(pos, radii, rule)
        for cap in (1, 100, full["nnz"] - 1, full["nnz"]):
            rc, got = raw_build(p, r, rule, cap, gpu_device)
            assert rc == 0 and got["nnz"] == full["nnz"]                       # the true total
            assert np.array_equal(got["rowptr"], full["rowptr"]) and np.array_equal(got["cscptr"], full["cscptr"])
            for k in ("colidx", "cscsrc", "cscpos"):
                assert np.array_equal(got[k][:cap], full[k][:cap]), (rule, cap, k)
        rc, got = raw_build(p, r, rule, 0, gpu_device, null_index=True)        # cap == 0: the index arrays may be NULL
        assert rc == 0 and got["nnz"] == full["nnz"] and np.array_equal(got["rowptr"], full["rowptr"])
    # the protocol: a clique of 65 agents has more than 32 edges per node - the first build overflows its guess, ready() re-builds
    pos, radii = er.case_positions(1, 65)
    edges = batched_edges(dv(pos, gpu_device), dv(radii, gpu_device))
    before = form_count()
    st = edges.structure(1)
    st.event.synchronize()
    first_cap = st.cap
    assert int(st.nnz_host[0]) == 65 * 65 > first_cap
    assert_arrays(got_arrays(st, gpu_device), er.edge_arrays(pos, radii, 1), "rebuild")
    assert st.cap >= 65 * 65 and st.exact_nnz() == 65 * 65 and form_count() == before + 2


# ---- 4. the model, bit for bit -----------------------------------------------------------------------------------------------------
def model(dev, N, seed=3, **kw):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import make_config
    from oracle import magat_oracle as orc
    cfg = make_config(num_agents=N, device=str(dev), **kw)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(orc.init_state_dict(cfg, seed=seed))
    return net.to(dev).eval()


def loop_inputs(B, N, dev, seed=0):
    from magat_pathplanning_amd.synthetic import fov_states
    pos, radii = er.case_positions(B, N, seed)
    radii[:] = 7.0 + 0.37 * np.arange(B)                                        # (no edgeless instance in the model cases)
    return dv(pos, dev), dv(radii, dev), fov_states(B, N, seed=5 + seed).to(dev), pos, radii


def both_routes(net, p, r, x):
    """logits behind addGSO(batched_gso(pos, r)) and behind addGSO(edges)"""
    from magat_pathplanning_amd import batched_edges, batched_gso
    with torch.no_grad():
        net.addGSO(batched_gso(p, r))
        want = net(x).clone()
        edges = batched_edges(p, r)
        net.addGSO(edges)
        got = net(x).clone()
    return got, want, edges


MODES = {"KeyQuery": dict(nAttentionHeads=2), "GAT_modified": dict(nAttentionHeads=2), "GAT_origin": dict(nAttentionHeads=2),
         "GAT_Similarity": dict(nAttentionHeads=1)}


@pytest.mark.parametrize("mode", list(MODES))
def test_model_dense_route_takes_the_adjacency(gpu_device, mode):
    """N = 16: the LDS-resident kernels read the tensor - edges.dense() through today's addGSO"""
    net = model(gpu_device, 16, attentionMode=mode, bottleneckFeature=64, numInputFeatures=64, **MODES[mode])
    p, r, x, pos, radii = loop_inputs(2, 16, gpu_device)
    before = form_count()
    got, want, edges = both_routes(net, p, r, x)
    assert torch.equal(got, want)
    assert torch.is_tensor(net.S) and tuple(net.S.shape) == (2, 1, 16, 16) and net._edges is None
    assert np.array_equal(net.S[:, 0].cpu().numpy(), er.dense(pos, radii)) and form_count() == before + 1


@pytest.mark.parametrize("mode", list(MODES))
def test_model_csr_route_float32(gpu_device, mode, monkeypatch):
    """N = 130: beyond the LDS-resident kernels - the CSR kernels on the structure from the positions, nothing densified"""
    from magat_pathplanning_amd import graphml
    net = model(gpu_device, 130, attentionMode=mode, bottleneckFeature=64, numInputFeatures=64, nGraphFilterTaps=3, **MODES[mode])
    p, r, x, _, _ = loop_inputs(2, 130, gpu_device)
    got, want, edges = both_routes(net, p, r, x)
    assert torch.equal(got, want)
    assert net.S is edges and not torch.is_tensor(net.S)

    def refuse(*a, **k):
        raise AssertionError("dense_gso_to_csr entered on the edges route")
    monkeypatch.setattr(graphml, "dense_gso_to_csr", refuse)
    with torch.no_grad():
        net.addGSO(edges.refresh())
        assert torch.equal(net(x), want)                                       # and again: determinism of the whole step


def test_model_csr_route_bf16_fused(gpu_device):
    """config 5's layer (bf16 storage, KeyQuery, K = 2, 128 features, P = 4) at N = 130: the fused CSR form on both routes"""
    net = model(gpu_device, 130, attentionMode="KeyQuery", nGraphFilterTaps=2, nAttentionHeads=4, gat_storage="bf16")
    p, r, x, _, _ = loop_inputs(2, 130, gpu_device)
    fused = form_count("csr_fused")
    got, want, edges = both_routes(net, p, r, x)
    assert form_count("csr_fused") == fused + 2                                 # one per route
    assert torch.equal(got, want) and net.S is edges


def test_model_behind_the_one_pass_builder(gpu_device):
    """N = 1100: today's route is dense_gso_to_csr and the in-call transpose; the edges route brings the column view"""
    net = model(gpu_device, 1100, attentionMode="KeyQuery", bottleneckFeature=32, numInputFeatures=32, nGraphFilterTaps=2,
                nAttentionHeads=2)
    p, r, x, _, _ = loop_inputs(2, 1100, gpu_device)
    got, want, edges = both_routes(net, p, r, x)
    assert torch.equal(got, want) and net.S is edges


def test_wrong_graph_and_other_classes_raise(gpu_device):
    from magat_pathplanning_amd import DecentralPlannerBottleneckNet, DecentralPlannerNet, batched_edges
    from magat_pathplanning_amd.synthetic import make_config
    net = model(gpu_device, 130, bottleneckFeature=32, numInputFeatures=32, gat_storage="bf16")      # (the CSR route at any N)
    p, r, x, _, _ = loop_inputs(2, 130, gpu_device)
    with torch.no_grad():
        net.addGSO(batched_edges(p[:1], r[:1]))
        with pytest.raises(ValueError, match="1 instances x 130 agents"):
            net(x)
        net.addGSO(batched_edges(p[:, :129].contiguous(), r))
        with pytest.raises(ValueError, match="129 agents"):
            net(x)
    edges = batched_edges(p, r)
    for cls, kw in ((DecentralPlannerNet, {}), (DecentralPlannerBottleneckNet, dict(bottleneckMode="BottomNeck_only"))):
        with pytest.raises(TypeError, match="batched_gso"):
            cls(make_config(num_agents=130, device=str(gpu_device), CNN_mode="Default", **kw)).addGSO(edges)


def test_training_mode_and_attention_take_the_adjacency(gpu_device):
    """the routes that need a tensor get edges.dense() through today's addGSO: train() mode at addGSO time, or return_attention
    switched on behind an addGSO(edges) that chose the CSR route (autograd switched on behind it: tests/test_host_edges.py)"""
    from magat_pathplanning_amd import batched_edges, batched_gso
    net = model(gpu_device, 130, attentionMode="GAT_modified", bottleneckFeature=32, numInputFeatures=32, nAttentionHeads=2)
    p, r, x, pos, radii = loop_inputs(2, 130, gpu_device)
    adjacency = er.dense(pos, radii)
    net.train()
    net.addGSO(batched_edges(p, r))
    assert torch.is_tensor(net.S) and net._edges is None and np.array_equal(net.S[:, 0].cpu().numpy(), adjacency)
    net.eval()
    edges = batched_edges(p, r)
    with torch.no_grad():
        net.addGSO(edges)
        assert net.S is edges
        plain = net(x).clone()
        net.GFL[0].return_attention = True
        got = net(x)
        assert torch.is_tensor(net.S) and net._edges is None
        att = net.returnAttentionGSO()
        net.addGSO(batched_gso(p, r))
        assert torch.equal(got, net(x)) and np.array_equal(att, net.returnAttentionGSO())
        net.GFL[0].return_attention = False
    assert np.array_equal(att[:, 0] != 0, adjacency != 0) and float((got - plain).abs().max()) <= 1e-4      # (another kernel family)


# ---- 5. beyond the dense GSO -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2500, 4096])
def test_model_beyond_the_dense_gso(gpu_device, N, monkeypatch):
    from magat_pathplanning_amd import _native as nat, batched_edges, graphml
    B = 1
    net = model(gpu_device, N, attentionMode="KeyQuery", bottleneckFeature=32, numInputFeatures=32, nGraphFilterTaps=2,
                nAttentionHeads=2)
    p, r, x, pos, radii = loop_inputs(B, N, gpu_device)
    dense = batched_edges(p, r).dense()
    assert dense.dtype == torch.float32 and np.array_equal(dense.cpu().numpy(), er.dense(pos, radii))
    with torch.no_grad():
        net.addGSO(dense)                                                      # today's path: scrub, dense_gso_to_csr, transpose
        want = net(x).clone()
    del dense

    def refuse(*a, **k):
        raise AssertionError("dense_gso_to_csr entered on the edges route")
    monkeypatch.setattr(graphml, "dense_gso_to_csr", refuse)
    torch.cuda.synchronize()
    edges = batched_edges(p, r)
    base = torch.cuda.memory_allocated(gpu_device)
    st = edges.structure(0)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated(gpu_device) - base
    assert grown <= nat.lib().magat_gso_edges_workspace_bytes(B, N) + 4 * (2 * B * (N + 1) + 3 * st.cap) + (1 << 20), grown
    with torch.no_grad():
        net.addGSO(edges)
        got = net(x)
    assert net.S is edges and not torch.is_tensor(net.S)
    assert torch.equal(got, want)


# ---- 6. the closed loop ------------------------------------------------------------------------------------------------------------
def test_episode_and_pool_edges_follow_the_positions(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, EpisodePool, generate_cases
    cases = generate_cases(16, 16, 16, 12, density=0.1, complexity=0.05, seed=11, device=gpu_device)
    keep = torch.nonzero(cases["valid"].reshape(-1) != 0).flatten()[:6]
    assert keep.numel() == 6
    cases = {k: cases[k][keep].contiguous() for k in ("map", "start", "goal")}
    g = torch.Generator(device="cpu").manual_seed(3)
    ep = BatchedEpisode(cases["map"], cases["start"], cases["goal"], 20, 4.0)
    pool = EpisodePool(cases["map"], cases["start"], cases["goal"], 20, 3, 4.0, first_step=0)
    for step in range(4):
        for who, B in ((ep, 6), (pool, 3)):
            edges = who.edges()
            assert edges is who.edges()                                        # one object, refreshed
            pos, radii = who.pos.cpu().numpy(), who.radii.cpu().numpy()
            for rule in (0, 1):
                assert_arrays(got_arrays(edges.structure(rule), gpu_device), er.edge_arrays(pos, radii, rule), (step, B, rule))
            who.step(actions=torch.randint(0, 5, (B, 12), generator=g, dtype=torch.int32).to(gpu_device))
    assert float(ep.radii.min()) >= 4.0 / 1.1 and torch.equal(ep.radii, dv(ep.radii.cpu().numpy(), gpu_device))


def test_evaluate_cases_rows_are_the_same_on_both_graphs(gpu_device):
    from magat_pathplanning_amd import evaluate_cases, generate_cases
    net = model(gpu_device, 4, seed=7, nGraphFilterTaps=2, nAttentionHeads=1)
    cases = generate_cases(32, 8, 8, 4, density=0.15, complexity=0.05, seed=31, device=gpu_device)
    keep = torch.nonzero(cases["valid"].reshape(-1) != 0).flatten()[:12]
    assert keep.numel() == 12
    maps, start, goal = (cases[k][keep].contiguous() for k in ("map", "start", "goal"))
    run = lambda **kw: evaluate_cases(net, maps, start, goal, 12, 4, 7.0, poll=4, action_select="soft_max", **kw)      # noqa: E731
    want, got = run(), run(graph="edges")
    assert set(got) == set(want) and bool((want["retired"] == 1).all())
    for k in want:
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError, match="graph"):
        run(graph="csr")


def test_three_steps_of_1500_agents_on_a_wide_map(gpu_device, monkeypatch):
    from magat_pathplanning_amd import EpisodePool, graphml
    N, H = 1500, 128
    rng = np.random.default_rng(5)
    cells = np.stack([rng.permutation(H * H)[:N] for _ in range(2)])
    start, goal = (np.stack([c // H, c % H], axis=-1).astype(np.int32)[None] for c in cells)
    net = model(gpu_device, N, attentionMode="KeyQuery", bottleneckFeature=32, numInputFeatures=32, nGraphFilterTaps=2,
                nAttentionHeads=2)

    def refuse(*a, **k):
        raise AssertionError("dense_gso_to_csr entered on the edges route")
    monkeypatch.setattr(graphml, "dense_gso_to_csr", refuse)
    before = form_count()
    pool = EpisodePool(torch.zeros(H, H, dtype=torch.uint8, device=gpu_device), dv(start, gpu_device), dv(goal, gpu_device), 3, 1, 7.0,
                       wide=True)
    with torch.no_grad():
        for _ in range(3):
            net.addGSO(pool.edges())
            pool.step(logits=net(pool.states()))
    assert form_count() == before + 3 and net.S is pool.edges() and pool.finished()
    res = pool.results()
    assert int(res["retired"][0]) == 1 and int(res["steps"][0]) == 3 and int(res["status"][0]) == 0


# ---- 7. plumbing -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gpu_device):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    NULL, BAD, UNSUPPORTED, WORKSPACE = -5, -1, -2, -3
    B, N = 2, 70
    pos, radii = er.case_positions(B, N)
    p, r = dv(pos, gpu_device), dv(radii, gpu_device)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=gpu_device)      # noqa: E731
    rowptr, cscptr, colidx, cscsrc, cscpos = i32(B * (N + 1)), i32(B * (N + 1)), i32(64), i32(64), i32(64)
    nnz = torch.full((1,), -7, dtype=torch.int64, device=gpu_device)
    ws = torch.empty(lib.magat_gso_edges_workspace_bytes(B, N) + 256, dtype=torch.uint8, device=gpu_device)

    def call(pos=p, radii=r, R=0.0, rule=0, rowptr=rowptr, colidx=colidx, cscptr=cscptr, cscsrc=cscsrc, cscpos=cscpos, cap=64, nnz=nnz,
             ws=ws.data_ptr(), nbytes=ws.numel() - 256, B=B, N=N):
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        return lib.magat_gso_edges_build(P(pos), P(radii), R, rule, P(rowptr), P(colidx), P(cscptr), P(cscsrc), P(cscpos), cap, P(nnz),
                                         ctypes.c_void_p(ws) if ws else None, nbytes, B, N, nat.current_stream(gpu_device))

    before = form_count()
    assert lib.magat_gso_edges_workspace_bytes(1, 4097) == 0 and lib.magat_gso_edges_workspace_bytes(0, 8) == 0
    assert lib.magat_gso_edges_workspace_bytes(8, 0) == 0 and lib.magat_gso_edges_workspace_bytes(1, 4096) % 256 == 0
    for k in ("pos", "rowptr", "cscptr", "nnz", "colidx", "cscsrc", "cscpos"):
        assert call(**{k: None}) == NULL, k
    assert call(pos=None, B=0) == NULL and call(colidx=None, cap=-1) == NULL and call(rowptr=None, N=5000) == NULL      # NULL first
    for kw in (dict(B=0), dict(N=0), dict(N=-3), dict(cap=-1), dict(rule=2), dict(rule=-1), dict(radii=None, R=0.0),
               dict(radii=None, R=-1.0), dict(radii=None, R=float("nan")), dict(B=0, N=5000), dict(rule=2, nbytes=0)):
        assert call(**kw) == BAD, kw                                            # ... then the sizes ...
    assert call(N=4097) == UNSUPPORTED and call(N=4097, ws=0) == UNSUPPORTED   # ... then the limit ...
    assert call(ws=0) == WORKSPACE and call(nbytes=ws.numel() - 257) == WORKSPACE and call(ws=ws.data_ptr() + 128) == WORKSPACE
    torch.cuda.synchronize()
    assert form_count() == before                                              # nothing was launched,
    assert int(nnz.item()) == -7 and int(rowptr.max()) == -7 and int(colidx.max()) == -7      # nothing was written
    assert call(colidx=None, cscsrc=None, cscpos=None, cap=0) == 0 and call(radii=None, R=7.0) == 0 and form_count() == before + 2


def test_captured_build_replays_on_moved_positions_and_repeats(gpu_device):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    B, N = 3, 200
    pos, radii = er.case_positions(B, N)
    moved, _ = er.case_positions(B, N, seed=1)
    p, r = dv(pos, gpu_device), dv(radii, gpu_device)
    cap = 32 * B * N
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=gpu_device)      # noqa: E731
    out = dict(rowptr=i32(B * (N + 1)), colidx=i32(cap), cscptr=i32(B * (N + 1)), cscsrc=i32(cap), cscpos=i32(cap))
    nnz = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    ws = torch.empty(lib.magat_gso_edges_workspace_bytes(B, N), dtype=torch.uint8, device=gpu_device)
    args = (nat.ptr(p), nat.ptr(r), 0.0, 1, nat.ptr(out["rowptr"]), nat.ptr(out["colidx"]), nat.ptr(out["cscptr"]), nat.ptr(out["cscsrc"]),
            nat.ptr(out["cscpos"]), cap, nat.ptr(nnz), nat.ptr(ws), ws.numel(), B, N)
    assert lib.magat_gso_edges_build(*args, nat.current_stream(gpu_device)) == 0      # (once outside the capture)
    torch.cuda.synchronize()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=gpu_device)
    stream.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.graph(graph, stream=stream):
        rc = lib.magat_gso_edges_build(*args, nat.current_stream(gpu_device))
    assert rc == 0
    for t in list(out.values()) + [nnz]:
        t.fill_(-7)

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        n = int(nnz.item())
        return dict({k: (v if k.endswith("ptr") else v[:n]).cpu().numpy() for k, v in out.items()}, nnz=n)
    first = replay()
    assert_arrays(first, er.edge_arrays(pos, radii, 1), "captured")
    assert_arrays(replay(), first, "repeat")                                   # determinism over two calls
    p.copy_(dv(moved, gpu_device))
    assert_arrays(replay(), er.edge_arrays(moved, radii, 1), "moved")
    assert not np.array_equal(first["colidx"], replay()["colidx"])
