"""CPU-only checks of tests/large_graph_cases.py, the inputs of tests/test_gpu_large_graph.py: every case keeps the property it
exists for (degrees, N against the tile sizes and against 1024 / 8190, the rule-sensitive entries, distinct instances), no case
of the forced list can sit on the LDS-tiled route and none of the tiled list off it, the yardstick itself is an attention
tensor (zero off the edges, rows that sum to 1), and the float32 composite's own error against the float64 one - the figure the
gates of the device test are made from - is printed per case and stays where a fault would still show."""
import itertools

import pytest
import torch

import large_graph_cases as lg
import train_graph_cases as tg

ALL = list(lg.CASES)


def test_case_lists_are_whole_and_ids_unique():
    """Every id names one case; the three lists are what the device file parametrizes over - nothing filtered, nothing marked."""
    assert len(set(ALL)) == len(ALL) == len(set(lg.FORCED) | set(lg.TILED) | set(lg.LARGE))
    assert all(k.id == cid for cid, k in lg.CASES.items())
    assert not set(lg.FORCED) & set(lg.LARGE) and not set(lg.TILED) & set(lg.LARGE)
    assert set(lg.TRAIN_ONLY) <= set(lg.LARGE_TRAIN)
    assert sorted(lg.LARGE_INFER + list(lg.TRAIN_ONLY)) == sorted(lg.LARGE)
    import test_gpu_large_graph as dev
    assert dev.FORCED_IDS == list(lg.FORCED) and dev.TILED_IDS == list(lg.TILED)
    assert dev.INFER_IDS == lg.LARGE_INFER and dev.TRAIN_IDS == lg.LARGE_TRAIN
    for fn in (dev.test_forced_per_edge_kernels_match_float64, dev.test_tiled_kernels_match_float64,
               dev.test_layers_past_1024_agents_match_float64, dev.test_training_past_1024_agents_matches_float64):
        marks = [m.name for m in getattr(fn, "pytestmark", [])]
        assert marks == ["parametrize"], marks          # (no skip, no xfail)


def test_forced_list_covers_widths_modes_heads_and_depths_pairwise():
    fp32 = [k for k in lg.FORCED.values() if not k.bf16 and k.mode != lg.GNN]
    factors = {"mode": (lg.KQ, lg.GM, lg.GO), "G": (16, 32, 64, 128, 256), "concat": (True, False), "P": (1, 2, 3, 4)}
    for a, b in itertools.combinations(factors, 2):
        have = {(getattr(k, a), getattr(k, b)) for k in fp32}
        missing = set(itertools.product(factors[a], factors[b])) - have
        assert not missing, (a, b, sorted(missing, key=str))
    assert {k.K for k in fp32} >= {1, 2, 3, 4, 5}
    assert {(k.K, k.att) for k in fp32} >= {(1, True), (1, False)}
    assert {k.N for k in fp32} >= {1, 3, 33, 65, 70, 130} and {k.B for k in fp32} >= {9, 17}
    assert all(k.B <= 3 or k.distinct for k in lg.FORCED.values())
    assert {(k.f64, k.mode) for k in fp32} >= {(True, lg.KQ), (True, lg.GO), (False, lg.KQ), (False, lg.GM), (False, lg.GO)}
    assert {k.G for k in lg.FORCED.values() if k.bf16} == {32, 64, 128}
    assert {(k.N, k.G != k.F) for k in lg.FORCED.values() if k.mode == lg.GNN} == {(33, True), (130, True)}
    # the tile tails: more than one score tile (32 rows per block, 64 at width 16) with a short last one, N % 4 != 0 for the hops
    assert any(k.N == 33 and k.G >= 32 for k in fp32) and any(k.N == 65 and k.G == 16 for k in fp32)
    assert all(k.N % 4 for k in fp32 if k.group == "tails")


def test_routes_of_the_lists():
    """tiled_ok (csrc/gat_csr_route.h) restated: with CSR_TILED = 0 no forced case reaches a tiled kernel; with CSR_TILED = 3 every case of the tiled
    list runs at least one and the list holds both kinds, the ends of the size range and a row format of each storage type."""
    for k in lg.FORCED.values():
        assert lg.tiled_route(0, k.mode, k.N, k.G, k.F, k.K, k.bf16, k.att) == (False, False), k.id
    routes = {k.id: lg.tiled_route(3, k.mode, k.N, k.G, k.F, k.K, k.bf16, k.att) for k in lg.TILED.values()}
    assert all(any(v) for v in routes.values()), routes
    assert any(v[0] for v in routes.values()) and any(v == (False, True) for v in routes.values())
    for cid, k in lg.FORCED.items():
        if cid not in lg.TILED:
            assert k.N < lg.TILED_MIN_N or (k.G * (2 if k.bf16 else 4)) % 128 or (k.K == 1 and not (k.mode == lg.KQ and k.att)) or \
                (k.mode != lg.KQ and (k.F * (2 if k.bf16 else 4)) % 128), cid
    own = [k for k in lg.TILED.values() if k.group == "tiled"]
    assert {k.N for k in own} == {9, 255, 513, 1024}
    assert {k.gso.__name__ for k in own} == {"gso_hubs", "gso_dense", "gso_empty"}
    assert any(k.bf16 for k in own) and any(k.mode == lg.GNN for k in own)
    # past 1024 agents the size alone decides, whatever the option says
    for k in lg.LARGE.values():
        assert k.N > lg.TILED_MAX_N and k.N <= lg.MAX_N
        assert lg.tiled_route(3, k.mode, k.N, k.G, k.F, k.K, k.bf16, k.att) == (False, False), k.id
    assert {k.N for k in lg.LARGE.values()} >= {1025, 1100, 2048, 8190}
    big = [k for k in lg.LARGE.values() if k.N == lg.MAX_N]
    assert len(big) <= 4 and all(k.B == 1 and k.P == 1 and k.G == 16 and k.F == 16 for k in big)


def _degree_sets(r):
    m = r.mask
    return set(m.sum(2).reshape(-1).tolist()), set(m.sum(1).reshape(-1).tolist())


@pytest.mark.parametrize("cid", ALL)
def test_case_keeps_its_property_and_float32_composite_error(cid):
    r = lg.reference(cid)
    k = r.case
    N = k.N
    assert r.S.dtype == (torch.float64 if k.f64 else torch.float32) and r.x.dtype == torch.float32
    # the edge list against the rule as train_graph_cases states it (GAT_Similarity: GAT_origin's)
    assert (r.row_deg, r.col_deg) == tg.degrees(r.S, tg.GO if k.mode == lg.SIM else k.mode)
    assert r.nnz == int(r.rowptr[-1]) and torch.equal(lg.csr_rowptr(r).view(k.B, N + 1)[:, 0], r.rowptr[::N][:k.B])
    if r.nnz:
        cols = r.colidx.clone()
        same_row = r.rowid[1:] == r.rowid[:-1]
        assert bool((cols[1:][same_row] > cols[:-1][same_row]).all())          # columns ascending inside a row
    loops = 1 if k.mode in (lg.GO, lg.SIM) else 0
    rows, cols = _degree_sets(r)
    if k.gso is lg.gso_degrees:
        want = {0, 1, 2, 3}
        assert {d - loops for d in rows} >= want and {d - loops for d in cols} >= want, (rows, cols)
        m = r.mask
        assert not m[:, 0].any() or loops                         # node 0: isolated (GAT_origin: its self-loop alone)
        assert int(m[0, 0].sum()) == loops and int(m[0, :, 0].sum()) == loops
        assert int(m[0, 1].sum()) == 1 + loops and int(m[0, :, 1].sum()) == loops          # only sends
        assert int(m[0, 4].sum()) == loops and int(m[0, :, 4].sum()) == 1 + loops          # only receives
        assert float(r.S[0, 7, 8]) != 0 and bool(m[0, 7, 8]) == (k.mode == lg.GNN) and bool(m[0, 8, 7])
    if k.gso is lg.gso_tiny:
        # (with GAT_origin's self-loops a row of three nodes has at most two edges more)
        assert N in (1, 3) and {d - loops for d in rows} >= ({0, 1} if N == 1 else {0, 1, 2, 3 - loops})
        assert bool(r.mask[2, 0, 0]) if N == 1 else (not r.mask[1, 0, 1] and bool(r.mask[1, 0, 2]))
    if k.gso in (tg.gso_hubs, lg.gso_khubs, lg.gso_limit):
        assert r.row_deg == N and r.col_deg == N
    if k.gso is lg.gso_past:
        m = r.mask[0]
        assert r.row_deg >= N - 2 and r.col_deg >= N - 2
        assert int(m[5].sum()) == loops and int(m[:, 5].sum()) == loops                    # isolated
        assert int(m[9].sum()) >= 4 and int(m[:, 9].sum()) == loops                        # only sends
        assert bool(m[20, 21]) == (k.mode == lg.GNN) and bool(m[21, 20])
        assert bool(m[30, N - 1]) or bool(m[3, N - 1])                                     # an edge in the last column
    if k.gso is lg.gso_limit:
        m = r.mask[0]
        assert bool(m[30, N - 1]) and bool(m[20, 21]) == (k.mode == lg.GNN) and bool(m[21, 20])
        assert all(int(m[i].sum()) == 1 + (loops and i != 7) for i in range(40, 45))
    if k.gso is tg.gso_full:
        assert rows == {N} and cols == {N}
    if k.gso is lg.gso_kdense:
        assert r.row_deg > 32 or N == 9                 # more edges than the tiled kernels' batched path holds
    if k.gso is lg.gso_kempty:
        assert not r.mask[:, : N // 2].any() or loops
        assert int(r.mask[:, : N // 2].sum()) == loops * k.B * (N // 2)
    if k.gso is tg.gso_edgeless:
        assert r.nnz == loops * k.B * N
    if k.gso is tg.gso_first_edgeless:
        assert int(r.mask[0].sum()) == loops * N and int(r.mask[1].sum()) > loops * N
    if k.gso is lg.gso_no_edge_row:
        assert k.mode == lg.GO and not r.mask[0, 4].any() and bool(r.mask[0, 6, 4]) and int(r.mask[1, 2].sum()) > 0
        assert not r.mask[1, 2, 2]
    if k.distinct:
        assert k.B in (9, 17)
        y = r.want["y"]
        for a in range(k.B):
            for b in range(a + 1, k.B):
                assert not torch.equal(r.S[a], r.S[b]) and not torch.equal(y[a], y[b]), (a, b)
    if k.tiny:
        for (b, n) in (lg.ZERO_ROW, lg.TINY_ROW):
            assert int(r.mask[b, n].sum()) > 1 and int(r.mask[b, :, n].sum()) > 1        # with edges, and someone's neighbour
        nx = r.x.double().norm(dim=1)
        W = r.state["weight"][0, 0].double()
        nq = torch.einsum("fg,bgn->bfn", W, r.x.double()).norm(dim=1)
        for n_ in (nx, nq):            # float32 and float64 agree on which rows the 1e-9 clamp touches
            assert bool(((n_ == 0) | (n_ <= 1e-11) | (n_ >= 1e-6)).all())
        assert float(nx[lg.ZERO_ROW]) == 0 and 0 < float(nx[lg.TINY_ROW]) <= 1e-11
    # the yardstick: finite, an attention tensor
    want = r.want
    assert want["y"].shape == (k.B, lg.out_width(k), N) and bool(torch.isfinite(want["y"]).all()) and float(want["y"].abs().max()) > 0
    if k.mode != lg.GNN:
        assert r.off_edges == 0.0 and want["att"].shape == (r.nnz, k.P)
        zero = torch.zeros_like(want["att"])
        a_abs, a_sum, a_rel = lg.attention_errors(want["att"], want["att"], r.rowid, k.B * N)
        assert (a_abs, a_rel) == (0.0, 0.0) and a_sum <= 1e-12
        if r.nnz:          # the per-row measure sees a row that lost everything, whatever its length
            assert lg.attention_errors(zero, want["att"], r.rowid, k.B * N)[2] == 1.0
    if k.train:
        for name, t in want.items():
            assert t is None or bool(torch.isfinite(t).all()), name
        assert float(want["dx"].abs().max()) > 0
    if k.bf16:
        assert r.emul_off_edges == 0.0 and r.emul["y"].shape == want["y"].shape
        scale = float(want["y"].abs().max())
        assert float((r.emul["y"].double() - want["y"]).abs().max()) <= lg.BF16_FP32 * scale
    # the float32 composite against the float64 one, in the measures of the device test; the gates that follow
    print("%s: float32 composite  y %.2e (gate %.2e)  attention abs %.2e  row sums %.2e  per row %.2e (gate %.2e)"
          % (cid, r.f32_y, r.y_gate, r.f32_att[0], r.f32_att[1], r.f32_att[2], r.att_gate))
    assert r.y_gate == max(lg.Y_GATE, 4 * r.f32_y) and r.att_gate == max(lg.ATT_ROW, 4 * r.f32_att[2])
    # both are float32 sums in another order: the composite stays two orders under what one dropped edge of a 300-edge row moves
    assert r.f32_y <= 2e-5 and r.f32_att[0] <= lg.ATT_ABS and r.f32_att[1] <= lg.ATT_SUM and r.f32_att[2] <= 2e-5


def test_structure_route_changes_hands_at_1024_agents():
    """CsrStructure.supported: the one-pass builder takes 1024 agents and declines 1025 - the size at which the cases assume the
    layers go to dense_gso_to_csr (a host-side answer of the library: no device is touched)."""
    from magat_pathplanning_amd.graphml import CsrStructure
    assert CsrStructure.supported(1, 1024) and CsrStructure.supported(2, 1024)
    assert not CsrStructure.supported(1, 1025) and not CsrStructure.supported(1, lg.MAX_N)


@pytest.mark.parametrize("N", [1025, 2048])
@pytest.mark.parametrize("rule,mode", [(0, lg.KQ), (1, lg.GO), (2, lg.GNN)])
def test_structure_inputs_have_their_rows(N, rule, mode):
    S = lg.gso_of(lg.gso_structure, 1, N, 6000 + N, True)
    m = lg.edge_mask(S, mode)[0]
    loops = 1 if rule == 1 else 0
    assert int(m[3].sum()) == N and int(m[:, 7].sum()) == N - 5
    assert all(int(m[i].sum()) == loops for i in range(40, 45))
    assert bool(m[30, N - 1]) and bool(m[21, 20]) and bool(m[20, 21]) == (rule == 2)
