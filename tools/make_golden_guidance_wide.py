"""Generates tests/golden/guidw_<guidance>_<case>.npz: state tensors of GlobalG_S|SD and SemiLG_S|SD on maps beyond the narrow
kernel's 54 x 54, made by the REAL reference (AgentState.toInputTensor with its own offlineExpert/a_star.py, imported from the
reference tree through oracle/make_golden_sim.load_reference_frontend; build machine only).  TEST INFRASTRUCTURE, beside
tools/make_golden_guidance.py, whose scenario builder, random walk, situation counts and writer it uses.

    python tools/make_golden_guidance_wide.py      # rewrites every guidw_* fixture; a second run gives identical files

Data only, the layout of the guid_* fixtures: map (B,H,W) uint8, goal (B,N,2) int32, and
    GlobalG_*:  pos (B,N,2) int32,    x (B,N,3,11,11) uint8
    SemiLG_*:   pos (B,T,N,2) int32,  x (B,T,N,3,11,11) uint8     T = 8 steps through ONE AgentState per instance
Scenario n24_map65: 65 x 65 (the reference's published test set's size; search canvas 75 x 75, two 64-bit words a row), 24 agents,
density 0.10, two instances, all four strings, the planted situations of make_golden_guidance.scenario - asserted from the
reference's output as there.
Scenario n12_map70x130: 70 x 130 (canvas 80 x 140, three words a row), 12 agents, GlobalG_SD and SemiLG_SD.  Agents 0 .. 5 stand
next to a word boundary of the canvas - columns 63 | 64 and 127 | 128, row 63 | 64 (map column / row = canvas - 5) - with their
goals on the far side, one in each direction; the generator ASSERTS from the reference's channel 1 that each of those paths has
a cell on both sides of its boundary, next to each other.
The reference raises IndexError when a path is longer than its max_localPath (rows + columns of the padded map): it did not,
and the path lengths of tests/guidance_restatement.py on the same inputs are asserted to stay below it as well."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guidance_restatement as gr  # noqa: E402
from make_golden_guidance import FOV, T, count_situations, random_walk, reference_states, save_npz, scenario  # noqa: E402
from oracle.make_golden_sim import OUT, load_reference_frontend  # noqa: E402

HALF = FOV // 2
SIZE_LIMIT = 4 * 50592 // 2          # "well under" four times the largest guid_* file
# (agent, axis, map coordinate a of the boundary a | a + 1, start, goal): canvas 63 | 64 and 127 | 128 are map 58 | 59 and 122 | 123
CROSSINGS = [(0, 1, 58, (10, 56), (10, 75)), (1, 1, 58, (30, 61), (30, 40)),
             (2, 1, 122, (20, 120), (20, 128)), (3, 1, 122, (45, 125), (45, 100)),
             (4, 0, 58, (56, 30), (68, 30)), (5, 0, 58, (61, 90), (40, 90))]


def crossing_scenario(rng):
    H, W, N = 70, 130, 12
    m = (rng.random((H, W)) < 0.05).astype(np.int64)
    pos, goal = np.zeros((N, 2), np.int64), np.zeros((N, 2), np.int64)
    for n, axis, a, s, g in CROSSINGS:
        pos[n], goal[n] = s, g
        lo, hi = sorted((s[axis], g[axis]))
        if axis == 1:
            m[s[0], lo:hi + 1] = 0           # a free straight line: the path crosses where the agent can see it
        else:
            m[lo:hi + 1, s[1]] = 0
    taken = {tuple(p) for p in pos[:6]} | {tuple(g) for g in goal[:6]}
    free = [tuple(c) for c in np.argwhere(m == 0) if tuple(c) not in taken]
    idx = rng.permutation(len(free))
    for k, n in enumerate(range(6, N)):
        pos[n], goal[n] = free[idx[2 * k]], free[idx[2 * k + 1]]
    assert len({tuple(p) for p in pos}) == N and all(m[tuple(p)] == 0 for p in pos)
    return m, pos, goal


def walk(rng, m, pos, steps):
    """make_golden_guidance.random_walk for a map that is not square."""
    moves = np.array([[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]])
    seq = [pos.copy()]
    for _ in range(steps - 1):
        cur = seq[-1].copy()
        occupied = {tuple(p) for p in cur}
        for n in rng.permutation(len(cur)):
            q = cur[n] + moves[rng.integers(5)]
            if 0 <= q[0] < m.shape[0] and 0 <= q[1] < m.shape[1] and m[tuple(q)] == 0 and tuple(q) not in occupied:
                occupied.discard(tuple(cur[n]))
                occupied.add(tuple(q))
                cur[n] = q
        seq.append(cur)
    return np.stack(seq)


def assert_crossings(x, pos):
    """x (N,3,11,11) of the reference at positions pos: window cell (a, q) of agent n is canvas cell (pos[n] + (a, q))."""
    for n, axis, a, _, _ in CROSSINGS:
        ca = a + HALF + 1                                   # canvas index of the cell before the boundary
        w = ca - int(pos[n][axis])
        assert 0 <= w and w + 1 < FOV + 2, (n, w)
        p = x[n, 1] if axis == 0 else x[n, 1].T             # rows = the crossed axis
        assert (p[w] & p[w + 1]).any(), "agent %d: no path cell on both sides of canvas %d | %d" % (n, ca, ca + 1)


def assert_path_lengths(m, pos_seq, goal, guidance):
    limit = m.shape[0] + m.shape[1] + 4 * HALF              # rows + columns of the padded map
    view = gr.new_agent_view(len(goal), m.shape[0], m.shape[1], FOV) if guidance.startswith("SemiLG") else None
    longest = 0
    for pos in pos_seq:
        stats = []
        gr.guided_states(m, pos, goal, guidance, FOV, view, stats)
        longest = max(longest, max(len(s["path"]) for s in stats))
    assert longest < limit, (guidance, longest, limit)
    return longest


def write(name, guidance, scen, xs):
    semi = guidance.startswith("SemiLG")
    arrays = dict(map=np.stack([s[0] for s in scen]).astype(np.uint8), goal=np.stack([s[2] for s in scen]).astype(np.int32),
                  pos=np.stack([s[1] if semi else s[1][0] for s in scen]).astype(np.int32),
                  x=np.stack(xs if semi else [x[0] for x in xs]))
    path = os.path.join(OUT, "guidw_%s_%s.npz" % (guidance, name))
    save_npz(path, **arrays)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")
    assert os.path.getsize(path) < SIZE_LIMIT


def main():
    AgentState, _ = load_reference_frontend()
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261018)
    # ---- 65 x 65
    scen = []
    for _ in range(2):
        m, pos, goal = scenario(rng, 24, 65, 0.10)
        scen.append((m, random_walk(rng, m, pos, T), goal))
    out = {}
    for g in ("GlobalG_S", "GlobalG_SD", "SemiLG_S", "SemiLG_SD"):
        semi = g.startswith("SemiLG")
        out[g] = [reference_states(AgentState, g, m, seq if semi else seq[:1], goal) for m, seq, goal in scen]
        total = {}
        for (m, seq, goal), x in zip(scen, out[g]):
            for key, v in count_situations(m, seq[0], goal, x[0], g).items():
                total[key] = total.get(key, 0) + v
            print(g, "longest path", assert_path_lengths(m, seq if semi else seq[:1], goal, g))
        print(g, total)
        for key in ("goal_in_fov", "goal_projected", "on_own_goal", "other_on_goal", "corner", "no_path"):
            assert total[key] > 0, (g, key)
        write("n24_map65", g, scen, out[g])
    differ = sum(int((a[0][:, 1] != b[0][:, 1]).any(axis=(1, 2)).sum()) for a, b in zip(out["GlobalG_S"], out["GlobalG_SD"]))
    print("agents whose GlobalG_S and GlobalG_SD paths differ:", differ)
    assert differ > 0
    # ---- 70 x 130
    m, pos, goal = crossing_scenario(rng)
    scen = [(m, walk(rng, m, pos, T), goal)]
    for g in ("GlobalG_SD", "SemiLG_SD"):
        semi = g.startswith("SemiLG")
        x = reference_states(AgentState, g, m, scen[0][1] if semi else scen[0][1][:1], goal)
        assert_crossings(x[0], pos)
        print(g, "longest path", assert_path_lengths(m, scen[0][1] if semi else scen[0][1][:1], goal, g))
        write("n12_map70x130", g, scen, [x])


if __name__ == "__main__":
    main()
