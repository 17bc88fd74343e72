"""Properties of tests/csr_fused_cases.py, checked without a GPU: the probe data is exact where the gates of
tests/test_gpu_csr_fused_probes.py assume it, every case reaches the code it claims to reach (degrees, index-load remainders,
group / chunk / item geometry), the float32 restatement alone stays inside every gate, and three work-dropping defects applied
to the RESTATEMENT (never to a kernel) are flagged by the gates on at least 90 % of the rows or columns they touch.

Measured here (printed by the tests), random-weights gate of the GPU file: the emulation's own distance to the float64
evaluation of the same order gives, with the margin of 4,
    ladder-P4    c = 9.3e-3   floor = 9.8e-4   (row scales 0.34 .. 2.8)
    N257-B9-P4   c = 1.9e-2   floor = 2.0e-3   (row scales 0.32 .. 2.2)
(The two agree to ~1e-6 before the last rounding, so the distance is one bf16 unit at the few elements that sit on a rounding
boundary: 2^-7 of the row scale at the most, which bounds c by 4 x 2^-7.)"""
import pytest
import torch

import csr_fused_cases as C

F32, F64 = torch.float32, torch.float64
SMALL = [c.name for c in C.CASES if c.B * c.N <= 4096]              # (the properties below hold per construction on the others)
ALL = [c.name for c in C.CASES]


def _rt(x):
    return x.to(torch.bfloat16).float()


@pytest.mark.parametrize("name", ALL)
def test_inputs_and_probe_weights_survive_bf16(name):
    case = C.CASE[name]
    pr = case.probes
    X = case.X
    assert torch.equal(_rt(X), X) and float(X.abs().max()) == 1.0 and torch.equal(X * 4, torch.round(X * 4))
    for w in (pr.w_q(), pr.w_u(), pr.h(0), pr.h(1), pr.h(1, -1.0), pr.bias):
        assert torch.equal(_rt(w), w)
    Wq = pr.w_q()
    assert bool(((Wq != 0).sum(1) == 1).all()) and bool(((Wq != 0).sum(2) == 1).all())          # a signed permutation / 2
    for tap in (0, 1):
        H = pr.h(tap)[:, :, tap]
        assert bool(((H != 0).sum(1) == 1).all()) and bool(((H != 0).sum(2) == 1).all())
        assert float(pr.h(tap)[:, :, 1 - tap].abs().max()) == 0.0
    perms = [tuple(pr.perm_h[p, k].tolist()) for p in range(case.P) for k in (0, 1)] + [tuple(q.tolist()) for q in pr.perm_w]
    assert len(set(perms)) == len(perms)                        # a different permutation per head and tap
    # probe X with the bias: +-x + bias is a multiple of 1/8 below 2 - inside 8 significant bits, so the sum, its float32 and
    # its bf16 form are one number
    xs = X[: min(len(X), 512)]
    want = pr.read(xs.unsqueeze(0).expand(case.P, -1, -1), 0, 1.0, pr.bias)
    assert torch.equal(_rt(want), want) and float(want.max()) <= 2.0 and float(pr.bias.abs().max()) > 0
    assert torch.equal(want, C.taps(xs, torch.zeros(case.P, len(xs), C.G), pr.h(0), pr.bias))
    assert float(want.max()) > 0


@pytest.mark.parametrize("name", SMALL)
def test_probe_q_scores_are_exact_in_float32(name):
    case = C.CASE[name]
    s32, s64 = C.stages(name, "Q", F32), C.stages(name, "Q", F64)
    assert torch.equal(s32.q.double(), s64.q) and torch.equal(s32.scores.double(), s64.scores)
    assert torch.equal(_rt(s32.q), s32.q)
    u = C.stages(name, "U", F32)
    assert float(u.scores.abs().max()) == 0.0 if case.graph.nnz else True
    if case.P == 4 and case.graph.nnz > 1000:
        sc = s64.scores
        same = sum(float((sc[a] == sc[b]).float().mean()) for a in range(4) for b in range(a))
        assert same / 6 < 0.01, same
        assert 1.5 < float(sc.std()) < 3.5 and float(sc.abs().max()) < 16          # neither flat nor saturated


@pytest.mark.parametrize("name", ["ladder-P4", "ladder-P2", "ladder-P1"])
def test_ladder_carries_every_degree_both_ways(name):
    g = C.CASE[name].graph
    N = g.N
    for deg in (g.outdeg, g.indeg):
        d0, d1 = set(deg[:N].tolist()), set(deg[N:].tolist())
        assert set(C.LADDER) <= d0, sorted(set(C.LADDER) - d0)
        assert N - 1 in d1 and {v + 1 for v in C.LADDER} <= d1
        allv = d0 | d1
        assert {v % 4 for v in allv if 0 < v <= 8} == {0, 1, 2, 3} and {v % 4 for v in allv if v > 8} == {0, 1, 2, 3}
        assert {v % 2 for v in allv if v > C.KR} == {0, 1}          # both tails of the two-slot pipeline
        assert {8, 9, 62, 63, 64} <= allv
    # rows of very different degree in one 32-row group of a ranking: the lightest rows by out-degree are the heaviest columns
    light = torch.nonzero(g.outdeg[:N] <= 1).reshape(-1)
    assert int(g.indeg[:N][light].max()) >= 63
    # the ranking's group of a light-by-out-degree row holds, in the in-degree ranking, rows of 60+ edges beside rows of < 16
    order_in = torch.argsort(-torch.clamp(g.indeg[:N], max=63), stable=True)
    first = g.indeg[:N][order_in[:32]]
    assert int(first.max()) >= 63 and int(first.min()) < 16


def test_cases_cover_the_sizes_and_geometry_they_claim():
    want = {  # name: (ng, nchunk, items per XCD, scores grid, hop grid, trips)
        "ladder-P4": (11, 2, 2, 16, 32, 1), "ladder-P2": (11, 2, 2, 16, 16, 1), "ladder-P1": (11, 2, 2, 16, 16, 1),
        "N1-B3-P4": (1, 1, 1, 8, 16, 1), "N31-B8-P2": (1, 1, 1, 8, 8, 1), "N32-B9-P1": (1, 1, 2, 16, 16, 1),
        "N33-B17-P4": (2, 1, 3, 24, 48, 1), "N255-B1-P2": (8, 1, 1, 8, 8, 1), "N256-B1-P4": (8, 1, 1, 8, 16, 1),
        "N257-B9-P4": (9, 2, 4, 32, 64, 1), "N1024-B1-P2": (32, 4, 4, 32, 32, 1), "N2500-B1-P4": (79, 10, 10, 80, 160, 1),
        "trip2-B64-N1100-P2": (35, 5, 40, 256, 256, 2), "edges-B2-N300-P4": (10, 2, 2, 16, 32, 1)}
    assert set(want) == set(C.CASE)
    for name, w in want.items():
        geo = C.geometry(C.CASE[name])
        got = (geo["ng"], geo["nchunk"], geo["items"], geo["grid_scores"], geo["grid_hop"], geo["trips_scores"])
        assert got == w and geo["trips_hop"] == w[5], (name, got)
    assert {c.N for c in C.CASES} >= {1, 31, 32, 33, 255, 256, 257, 1024, 2500}
    assert {c.B for c in C.CASES} >= {1, 8, 9, 17} and {c.P for c in C.CASES} == {1, 2, 4}
    assert {c.bias_on for c in C.CASES} == {"f32", "bf16"}
    for c in C.CASES:
        g = c.graph
        assert g.B == c.B and g.nnz > 0
    # hub of N - 1 and rows without edges where the case names them
    for name in ("N31-B8-P2", "N255-B1-P2", "N257-B9-P4", "N1024-B1-P2", "N2500-B1-P4"):
        g = C.CASE[name].graph
        assert int(g.outdeg.max()) == g.N - 1 and int(g.indeg.max()) == g.N - 1
    for name in ("N33-B17-P4", "N256-B1-P4", "N1-B3-P4", "ladder-P4"):
        g = C.CASE[name].graph
        assert int((g.outdeg == 0).sum()) > 0 and (int((g.indeg == 0).sum()) > 0 or name.startswith("N33") or name.startswith("N256"))
    # undirected cases are symmetric, directed ones (and the hub row / column on N255's undirected base) are not
    for c in C.CASES:
        g = c.graph
        key, keyt = set((g.rows * g.B * g.N + g.cols).tolist()), set((g.cols * g.B * g.N + g.rows).tolist())
        assert (key == keyt) == (c.name in ("N32-B9-P1", "edges-B2-N300-P4", "N1-B3-P4")), c.name


@pytest.mark.parametrize("name", SMALL)
def test_structure_arrays_follow_the_builders_conventions(name):
    g = C.CASE[name].graph
    a = g.arrays()
    B, N = g.B, g.N
    rp, cp = a["rowptr"].view(B, N + 1).long(), a["cscptr"].view(B, N + 1).long()
    assert int(rp[0, 0]) == 0 and int(rp[-1, -1]) == g.nnz and int(cp[-1, -1]) == g.nnz
    assert torch.equal(rp[1:, 0], rp[:-1, -1]) and torch.equal((rp[:, 1:] - rp[:, :-1]).reshape(-1), g.outdeg)
    assert torch.equal((cp[:, 1:] - cp[:, :-1]).reshape(-1), g.indeg)
    S = g.dense()
    b, i, j = torch.nonzero(S, as_tuple=True)                                    # row-major: CSR order
    assert torch.equal(j.to(torch.int32), a["colidx"]) and torch.equal(b * N + i, g.rows)
    bt, jt, it = torch.nonzero(S.transpose(1, 2), as_tuple=True)                 # column-major: ascending source per column
    assert torch.equal(it.to(torch.int32), a["cscsrc"])
    pos = a["cscpos"].long()
    assert torch.equal(g.rows[pos], bt * N + it) and torch.equal(g.cols[pos], bt * N + jt)
    assert int(a["colidx"].min()) >= 0 and int(a["colidx"].max()) < N and int(a["cscsrc"].max()) < N


def _y_of(case, st32, flip):
    """what the restatement gives under probe Z: the tap contraction of the rounded hop, rounded"""
    return C.bf16(C.taps(case.X, st32.z16, case.probes.h(1, flip), None))


@pytest.mark.parametrize("name", ALL)
def test_the_restatement_alone_passes_every_gate(name):
    case = C.CASE[name]
    g = case.graph
    for probe in case.score_probes:
        s32, s64 = C.stages(name, probe, F32), C.stages(name, probe, F64)
        own = C.attention_error(g, s32.att, s64.att)
        bad, sum_err, ratio, err = C.attention_gate(g, s32.att, s64.att, own)
        assert not bool(bad.any()) and ratio <= 1.0
        if probe == "Q":
            online = C.online_softmax_f32(g, s32.scores)
            bad2, _, ratio2, err2 = C.attention_gate(g, online, s64.att, own)
            print("%s Q: restatement %.3g, online restatement %.3g of max a*, row sums %.3g" % (name, err, err2, sum_err))
            assert not bool(bad2.any()), ratio2
        else:
            assert not bool(C.uniform_gate(g, s32.att).any())
        t = C.hop_bound(case, s64, s32)
        for flip in (1.0, -1.0):
            y = _y_of(case, s32, flip)
            badz, ratio = C.hop_gate(case, y, s64, t, flip)
            print("%s %s Z%+d: restatement at %.3f of the bound" % (name, probe, flip, ratio))
            assert not bool(badz.any()), ratio


@pytest.mark.parametrize("name", SMALL)
def test_gates_flag_dropped_work_on_nine_rows_in_ten(name):
    """Defects of the restatement, not of a kernel.  softmax: the last out-edge of every row with more than 8 edges is left
    out of the softmax; hop: the last in-edge of every column with more than 8 in-edges is left out of the hop; heads: heads
    1 and 2 exchanged (P = 4; invisible under probe U, where all heads are equal: checked under probe Q)."""
    case = C.CASE[name]
    g = case.graph
    rep = []
    for probe in case.score_probes:
        s32, s64 = C.stages(name, probe, F32), C.stages(name, probe, F64)
        W = case.probes.w_q() if probe == "Q" else case.probes.w_u()
        own = C.attention_error(g, s32.att, s64.att)
        t = C.hop_bound(case, s64, s32)
        # softmax
        rows = g.last_out_edge()[1]
        if len(rows) >= 10:
            m = C.Stages(g, case.X, W, F32, mutate="softmax")
            bad = C.attention_gate(g, m.att, s64.att, own)[0][:, rows]
            if probe == "U":
                bad = bad | _edge_rows_any(g, C.uniform_gate(g, m.att))[:, rows]
            frac = float(bad.any(dim=0).float().mean())                 # the row is flagged: some head of it fails
            rep.append(("softmax", probe, len(rows), frac))
        # hop
        cols = g.last_in_edge()[1]
        if len(cols) >= 10:
            m = C.Stages(g, case.X, W, F32, mutate="hop")
            hit = torch.zeros(len(cols), case.P, dtype=torch.bool)
            for flip in (1.0, -1.0):
                y = C.bf16(C.taps(case.X, m.z16, case.probes.h(1, flip), None))
                hit |= C.hop_gate(case, y, s64, t, flip)[0][cols]
            frac = float(hit.any(dim=1).float().mean())                 # the column is flagged: some element of it fails
            rep.append(("hop", probe, len(cols), frac))
        # heads
        rows2 = torch.nonzero(g.outdeg >= 2).reshape(-1)
        if case.P == 4 and probe == "Q" and len(rows2) >= 10:
            m = C.Stages(g, case.X, W, F32, mutate="heads")
            bad = C.attention_gate(g, m.att, s64.att, own)[0][:, rows2]
            frac = float((bad[1] & bad[2]).float().mean())
            assert not bool(bad[0].any()) and not bool(bad[3].any())
            rep.append(("heads", probe, len(rows2), frac))
    for r in rep:
        print("%s: %s under probe %s: %d affected, %.3f flagged" % ((name,) + r))
    assert all(r[3] >= 0.9 for r in rep), rep


def _edge_rows_any(g, bad_edges):
    out = torch.zeros(bad_edges.shape[0], g.B * g.N, dtype=torch.bool)
    for p in range(bad_edges.shape[0]):
        out[p] = torch.zeros(g.B * g.N).index_add_(0, g.rows, bad_edges[p].float()) > 0
    return out


def test_sensitivity_is_exercised_where_it_matters():
    """the ladder, the N = 257 and the hub cases each have at least ten rows AND ten columns beyond the register slots"""
    for name in ("ladder-P4", "ladder-P2", "ladder-P1", "N257-B9-P4", "N1024-B1-P2", "N2500-B1-P4", "edges-B2-N300-P4"):
        g = C.CASE[name].graph
        assert len(g.last_out_edge()[1]) >= 10 and len(g.last_in_edge()[1]) >= 10, name


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.random])
def test_random_weights_budget_comes_from_the_emulation_itself(name):
    """c and the floor of the per-row gate: the emulation (float32, torch's own summation order) against float64 arithmetic
    from the edge lists with RNE at the same points.  Both agree before the last rounding to ~1e-6, so what is left is a bf16
    unit at elements that sit on a rounding boundary: c = 4 x 2^-7 at the most."""
    case = C.CASE[name]
    W, H, b = C.random_weights(case.P, case.seed)
    X = C.random_inputs(case)
    y_emul = C.emulation(case, W, H, b, X)
    y_same = C.same_order_f64(case, W, H, b, X)
    c, floor = C.row_budget(y_emul, y_same)
    scale = y_emul.abs().amax(dim=1)
    print("%s: c = %.3g, floor = %.3g, row scales %.3g .. %.3g" % (name, c, floor, float(scale.min()), float(scale.max())))
    assert 0 < c <= 4 * 2.0 ** -7 * 1.0001 and floor <= 2.0 ** -7 * float(scale.max())
    frac = float(((y_emul.double() - y_same).abs() > 0).float().mean())
    assert frac < 0.02, frac                                       # the two agree bit for bit almost everywhere
