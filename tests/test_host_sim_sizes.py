"""Host: the inputs of tests/test_gpu_sim_sizes.py, and the lambda_max rule of gso_kernel above 128 agents restated in numpy
(tests/gso_lanczos_restatement.py) against numpy.linalg.eigvalsh on those inputs at the project's gate, 1e-9 - the rule meets the
gate, not luck.  The rule cut off at 160 steps, which the kernel used to be, misses it on the long paths."""
import functools

import numpy as np
import pytest

import gso_lanczos_restatement as gl

EPS = float(np.finfo(np.float64).eps)
GATE = 1e-9


# ---- GSO inputs -----------------------------------------------------------------------------------------------------------------
def gso_sizes():
    """Either side of steps >= N against the 160 rows of the one-wave layout, 300, either side of the 64 KiB dynamic-LDS limit,
    1000, either side of the bit rows' 160 KiB limit (both from the restated formula), and the largest size accepted."""
    dyn, mask = gl.last_size_within(gl.DYN_LDS), gl.last_size_within(gl.LDS_LIMIT)
    return [129, 160, 161, 300, dyn, dyn + 1, 1000, mask, mask + 1, gl.MAX_AGENTS]


# per size, in the order of gso_sizes(): (graph, radius) of each instance; radii that differ go through the `radii` tensor
GSO_GRAPHS = [(("path", 4.0), ("random", 7.0), ("clusters", 7.0)),
              (("path", 7.0), ("lattice", 7.0), ("random", 7.0)),
              (("path", 4.0), ("clusters", 7.0)),
              (("clusters", 7.0), ("path", 7.0), ("random", 7.0)),
              (("path", 4.0), ("random", 7.0)),
              (("random", 7.0), ("path", 7.0), ("lattice", 7.0)),
              (("path", 4.0), ("random", 7.0), ("path", 7.0)),
              (("random", 7.0), ("clusters", 4.0)),
              (("path", 4.0), ("random", 7.7)),
              (("path", 4.0), ("random", 7.0))]


def gso_graph(kind, N, rng):
    k = np.arange(N)
    if kind == "path":          # pitch 3: a chain at R = 4, a band of two neighbours either side at R = 7
        return np.stack([3 * k, np.zeros(N, np.int64)], 1)
    if kind == "lattice":       # pitch 8: no edge at all at R = 7
        return np.stack([8 * (k % 64), 8 * (k // 64)], 1)
    if kind == "random":        # uniform at the density of 1000 agents on 160 x 160
        return rng.integers(0, int(round(160.0 * np.sqrt(N / 1000.0))), size=(N, 2))
    assert kind == "clusters"   # two far clusters, about one agent a cell: stacked agents included
    side = int(np.ceil(np.sqrt(N)))
    pos = rng.integers(0, side, size=(N, 2))
    pos[N // 2:] += 500
    return pos


@functools.lru_cache(maxsize=None)
def gso_case(index):
    """(N, pos (B,N,2) int32, radii (B,) float64, graph names)."""
    N = gso_sizes()[index]
    rng = np.random.default_rng(1000 + N)
    pos = np.stack([gso_graph(kind, N, rng) for kind, _ in GSO_GRAPHS[index]]).astype(np.int32)
    pos.setflags(write=False)
    return N, pos, np.array([r for _, r in GSO_GRAPHS[index]], np.float64), [kind for kind, _ in GSO_GRAPHS[index]]


def well_conditioned(N, lam):
    """The float64 eigvalsh reference is good to about N eps lambda_max absolute: below 1e-11 it is two digits inside the gate."""
    return N * EPS * lam < 1e-11


def test_gso_sizes_straddle_both_lds_limits():
    sizes = gso_sizes()
    dyn, mask = sizes[4], sizes[7]
    assert gl.gso_lds_bytes(dyn, True) <= gl.DYN_LDS < gl.gso_lds_bytes(dyn + 1, True)
    assert gl.gso_lds_bytes(mask, True) <= gl.LDS_LIMIT < gl.gso_lds_bytes(mask + 1, True)
    assert gl.uses_mask(mask) and not gl.uses_mask(mask + 1) and not gl.uses_mask(1000)
    assert gl.gso_lds_bytes(mask + 1, False) <= gl.DYN_LDS < gl.gso_lds_bytes(gl.MAX_AGENTS, False) <= gl.LDS_LIMIT
    assert len(set(sizes)) == len(GSO_GRAPHS) == 10
    kinds = {(N, kind) for N, graphs in zip(sizes, GSO_GRAPHS) for kind, _ in graphs}
    assert {(1000, "path"), (1000, "random"), (2048, "path"), (2048, "random")} <= kinds
    assert any(len({r for _, r in graphs}) > 1 for graphs in GSO_GRAPHS)          # per-instance radii
    assert any(kind == "lattice" for graphs in GSO_GRAPHS for kind, _ in graphs)   # an instance without an edge


@pytest.mark.parametrize("index", range(10))
def test_restated_rule_meets_the_gate(index):
    N, pos, radii, kinds = gso_case(index)
    for b, kind in enumerate(kinds):
        for sym in (False, True):
            lam, steps = gl.lambda_max(pos[b], radii[b], sym)
            M = gl.adjacency(pos[b], radii[b], sym)[3]
            if kind == "lattice":
                assert not M.any() and lam == 0.0
                continue
            ref = float(np.linalg.eigvalsh(M)[-1])
            assert well_conditioned(N, ref), (N, kind, sym, ref)
            print("rule N=%d %s R=%g sym=%d: %d steps, relative error %.2e" % (N, kind, radii[b], sym, steps, abs(lam - ref) / ref))
            assert steps <= N and abs(lam - ref) <= GATE * ref, (N, kind, sym, steps, lam, ref)


def test_rule_cut_off_at_160_steps_misses_the_gate_on_long_paths():
    """What the kernel did before it walked on: 3e-6 of lambda_max on the chain of 1000 agents, all 160 steps used."""
    for N in (1000, 2048):
        pos = gso_graph("path", N, None)
        lam, steps = gl.lambda_max(pos, 4.0, False, cap=160)
        ref = 2.0 * np.cos(np.pi / (N + 1))          # the chain's largest eigenvalue
        assert steps == 160 and 1e-7 < abs(lam - ref) / ref < 1e-5, (N, steps, lam, ref)


# ---- the crowded scene of the narrow move test -------------------------------------------------------------------------------------
def crowd_scene(H, W, N, side, seed):
    """One instance, N agents: one at each corner (agents 0..3, as tests/test_host_wide_loop.py's move_scene has them), the rest
    on the free cells of a side x side block in the middle, a tenth of whose cells are obstacles; goals in the block too."""
    rng = np.random.default_rng(seed)
    m = (rng.random((H, W)) < 0.02).astype(np.uint8)
    r0, c0 = (H - side) // 2, (W - side) // 2
    m[r0:r0 + side, c0:c0 + side] = rng.random((side, side)) < 0.1
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for r, c in corners:
        m[r, c] = 0
    cells = np.argwhere(m[r0:r0 + side, c0:c0 + side] == 0) + (r0, c0)
    assert len(cells) >= N - 4
    pos, goal = np.zeros((1, N, 2), np.int32), np.zeros((1, N, 2), np.int32)
    pos[0, :4], goal[0, :4] = corners, corners[::-1]
    pos[0, 4:] = cells[rng.permutation(len(cells))[:N - 4]]
    goal[0, 4:] = cells[rng.permutation(len(cells))[:N - 4]]
    return m, pos, goal


def test_crowd_scene_is_a_valid_start():
    m, pos, goal = crowd_scene(60, 64, 1100, 48, 6064)
    assert len({tuple(p) for p in pos[0]}) == 1100 and (m[pos[0, :, 0], pos[0, :, 1]] == 0).all()
    assert (m[goal[0, :, 0], goal[0, :, 1]] == 0).all()
