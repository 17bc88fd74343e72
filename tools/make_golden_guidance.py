"""Generates tests/golden/guid_<guidance>_<case>.npz: state tensors of the A*-guided encodings made by the REAL reference
(AgentState.toInputTensor of dataloader/statetransformer_Guidance.py with its own offlineExpert/a_star.py, imported from the
reference tree through oracle/make_golden_sim.load_reference_frontend; build machine only).  TEST INFRASTRUCTURE.

    python tools/make_golden_guidance.py         # rewrites every guid_* fixture; a second run gives identical files

Data only: map (B,H,W) uint8, goal (B,N,2) int32, and
    LocalG_* / GlobalG_*:  pos (B,N,2) int32,    x (B,N,3,11,11) uint8
    SemiLG_*:              pos (B,T,N,2) int32,  x (B,T,N,3,11,11) uint8     T = 8 steps through ONE AgentState per instance
                                                                            (its memory of the map grows from step to step)
The same scenarios serve all six guidance strings.  Every instance is seeded with the situations the device form must get right,
and the generator ASSERTS from the reference's own output that each of them occurs (counts are printed):
    goal inside the FOV / goal projected onto the window's border / an agent on its own goal / another agent on the goal cell /
    an agent at a map corner / a LocalG path that runs along the free border ring / an agent whose '_S' and '_SD' paths differ (LocalG, GlobalG; SemiLG's two strings agree by construction) /
    a search without a path (channel 1 = the start cell, plus the goal marker for LocalG) / for SemiLG an agent whose step-7
    path differs from what an empty memory gives.
"No path" is produced by a goal on an obstacle cell inside the FOV (LocalG; GlobalG / SemiLG clear a goal cell of value 1) and
by a walled-in agent (all modes).  A PROJECTED goal can never be blocked: projectedgoal always lands on the window's border ring,
which the reference pads with free cells.
The reference raises IndexError when a path is longer than its max_localPath; no fixture case gets there (asserted)."""
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden_sim import OUT, load_reference_frontend  # noqa: E402

GUIDANCE = ("LocalG_S", "LocalG_SD", "GlobalG_S", "GlobalG_SD", "SemiLG_S", "SemiLG_SD")
CASES = [("n10_map20", 10, 20, 0.10, 4), ("n100_map50", 100, 50, 0.08, 3), ("n12_map10_dense", 12, 10, 0.25, 4)]
FOV, T = 9, 8
MOVES = np.array([[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]])


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, arr in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(arr), allow_pickle=False)


def scenario(rng, N, size, density):
    """Map, start positions and goals with the special situations planted on agents 0..6."""
    m = (rng.random((size, size)) < density).astype(np.int64)
    m[0, 0] = 0                                              # agent 0 stands at a map corner
    m[0, 1] = m[1, 0] = 0
    free = np.argwhere(m == 0)
    free = free[(free[:, 0] + free[:, 1]) > 1]              # (not the corner and its two neighbours)
    idx = rng.permutation(len(free))
    pos, goal = free[idx[:N]].copy(), free[idx[N:2 * N]].copy()
    pos[0] = (0, 0)
    goal[1] = pos[1]                                         # on its own goal
    goal[2] = pos[3]                                         # agent 3 stands on agent 2's goal ...
    near = np.argwhere((m == 0) & (np.abs(np.arange(size)[:, None] - pos[3][0]) <= 3) &
                       (np.abs(np.arange(size)[None, :] - pos[3][1]) <= 3))
    taken = {tuple(p) for p in pos}
    for cand in near[rng.permutation(len(near))]:
        if tuple(cand) not in taken:
            pos[2] = cand                                    # ... inside agent 2's FOV
            break
    # agent 4: its goal lies on an obstacle cell inside its FOV (made one if the window holds none)
    obst = np.argwhere((m == 1) & (np.abs(np.arange(size)[:, None] - pos[4][0]) <= 4) &
                       (np.abs(np.arange(size)[None, :] - pos[4][1]) <= 4))
    if len(obst) == 0:
        q = np.clip(pos[4] + np.array([2, 2]), 0, size - 1)
        assert tuple(q) not in {tuple(p) for p in pos} and tuple(q) not in {(0, 0), (0, 1), (1, 0)}
        m[tuple(q)] = 1
        obst = q[None]
    goal[4] = obst[rng.integers(len(obst))]
    # agent 5: walled in (its four neighbours are obstacles or lie outside the map), goal far away
    occupied = {tuple(p) for p in pos}
    for d in MOVES[:4]:
        q = pos[5] + d
        if 0 <= q[0] < size and 0 <= q[1] < size and tuple(q) not in occupied and tuple(q) not in {(0, 0), (0, 1), (1, 0)}:
            m[tuple(q)] = 1
    # agent 6: goal straight below / beside it, just outside the FOV where the map allows it
    for d in ([5, 0], [0, 5], [-5, 0], [0, -5]):
        q = pos[6] + np.array(d)
        if 0 <= q[0] < size and 0 <= q[1] < size and m[tuple(q)] == 0:
            goal[6] = q
            break
    for n in range(N):
        assert m[tuple(pos[n])] == 0
    assert len({tuple(p) for p in pos}) == N
    return m, pos.astype(np.int64), goal.astype(np.int64)


def random_walk(rng, m, pos, steps):
    """Seeded random walk over free cells; agents keep distinct cells."""
    size = m.shape[0]
    seq = [pos.copy()]
    for _ in range(steps - 1):
        cur = seq[-1].copy()
        occupied = {tuple(p) for p in cur}
        for n in rng.permutation(len(cur)):
            q = cur[n] + MOVES[rng.integers(5)]
            if 0 <= q[0] < size and 0 <= q[1] < size and m[tuple(q)] == 0 and tuple(q) not in occupied:
                occupied.discard(tuple(cur[n]))
                occupied.add(tuple(q))
                cur[n] = q
        seq.append(cur)
    return np.stack(seq)


def reference_states(AgentState, guidance, m, pos_seq, goal):
    """x (T,N,3,11,11) uint8 from ONE AgentState stepped through pos_seq (T,N,2)."""
    N = goal.shape[0]
    st = AgentState(types.SimpleNamespace(num_agents=N, FOV=FOV, guidance=guidance))
    st.setmap(m)
    out = []
    for pos in pos_seq:
        x = st.toInputTensor(goal.astype(np.float64), pos.astype(np.float64)).numpy()
        assert x.shape == (N, 3, FOV + 2, FOV + 2) and set(np.unique(x)) <= {0.0, 1.0}
        assert int(x[:, 1].sum(axis=(1, 2)).max()) < st.max_localPath, "a path reaches max_localPath"
        out.append(x.astype(np.uint8))
    return np.stack(out)


def count_situations(m, pos, goal, x, guidance):
    """Counted from the reference's tensors x (N,3,11,11) of one instance at positions pos."""
    half, c = FOV // 2, (FOV + 2) // 2
    size = m.shape[0]
    k = dict.fromkeys(("goal_in_fov", "goal_projected", "on_own_goal", "other_on_goal", "corner", "ring_path", "no_path"), 0)
    where = {tuple(p): n for n, p in enumerate(pos)}
    for n in range(len(pos)):
        d = goal[n] - pos[n]
        inside = bool(np.all(np.abs(d) <= half))
        k["goal_in_fov" if inside else "goal_projected"] += 1
        k["on_own_goal"] += int(np.all(d == 0))
        k["other_on_goal"] += int(where.get(tuple(goal[n]), n) != n)
        k["corner"] += int(tuple(pos[n]) in {(0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1)})
        p = x[n, 1].astype(bool)
        ring = p.copy()
        ring[1:-1, 1:-1] = False
        if guidance.startswith("LocalG"):
            k["ring_path"] += int(ring.sum() >= 2)           # the goal marker accounts for one ring cell at most
            # start + goal marker only, and the two are not neighbours: no path was drawn between them
            cells = np.argwhere(p)
            k["no_path"] += int(len(cells) == 2 and np.abs(cells[0] - cells[1]).sum() > 1)
        else:
            k["no_path"] += int(p.sum() == 1 and not np.all(d == 0))
    return k


def main():
    AgentState, _ = load_reference_frontend()
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    total = {g: {} for g in GUIDANCE}
    differ = dict(LocalG=0, GlobalG=0, SemiLG=0)
    semi_memory = 0
    for name, N, size, density, B in CASES:
        scen = []
        for _ in range(B):
            m, pos, goal = scenario(rng, N, size, density)
            scen.append((m, random_walk(rng, m, pos, T), goal))
        xs = {}
        for g in GUIDANCE:
            semi = g.startswith("SemiLG")
            xs[g] = [reference_states(AgentState, g, m, seq if semi else seq[:1], goal) for m, seq, goal in scen]
            for (m, seq, goal), x in zip(scen, xs[g]):
                for key, v in count_situations(m, seq[0], goal, x[0], g).items():
                    total[g][key] = total[g].get(key, 0) + v
            if semi:
                # what an EMPTY memory gives at the last step's positions: a fresh AgentState called once
                for (m, seq, goal), x in zip(scen, xs[g]):
                    fresh = reference_states(AgentState, g, m, seq[-1:], goal)[0]
                    semi_memory += int((fresh[:, 1] != x[-1][:, 1]).any(axis=(1, 2)).sum())
            arrays = dict(map=np.stack([s[0] for s in scen]).astype(np.uint8),
                          goal=np.stack([s[2] for s in scen]).astype(np.int32),
                          pos=np.stack([s[1] if semi else s[1][0] for s in scen]).astype(np.int32),
                          x=np.stack(xs[g] if semi else [x[0] for x in xs[g]]))
            path = os.path.join(OUT, "guid_%s_%s.npz" % (g, name))
            save_npz(path, **arrays)
            print("wrote", path, os.path.getsize(path) // 1024, "KB")
            assert os.path.getsize(path) < 700 * 1024
        for fam in differ:
            for a, b in zip(xs[fam + "_S"], xs[fam + "_SD"]):
                differ[fam] += int((a[0][:, 1] != b[0][:, 1]).any(axis=(1, 2)).sum())
    for g in GUIDANCE:
        print(g, total[g])
        for key in ("goal_in_fov", "goal_projected", "on_own_goal", "other_on_goal", "corner", "no_path"):
            assert total[g][key] > 0, (g, key)
        if g.startswith("LocalG"):
            assert total[g]["ring_path"] > 0, (g, "ring_path")
    print("agents whose _S and _SD paths differ:", differ)
    # SemiLG adds the agents in the FOV for '_S' and '_SD' alike (statetransformer_Guidance.py:359): its two strings agree
    assert differ["LocalG"] > 0 and differ["GlobalG"] > 0 and differ["SemiLG"] == 0, differ
    print("SemiLG agents whose step-%d path differs from an empty memory's:" % (T - 1), semi_memory)
    assert semi_memory > 0


if __name__ == "__main__":
    main()
