"""Generates tests/golden/expert_<case>.npz: imitation samples made from expert schedules by the REAL reference - its data
transformer (onlineExpert/DataTransformer_local_onlineExpert.py: obtainSchedule, getAdjacencyMatrix), its state encoder
(AgentState.setmap + toSeqInputTensor) and multiRobotSimNew.getPathTarget - imported from the reference tree at run time
(build machine only; easydict and hashids, which that module imports and never uses here, are stubbed in sys.modules).
TEST INFRASTRUCTURE.

    python tools/make_golden_expert.py           # rewrites every expert_* fixture; a second run gives identical files
    python tools/make_golden_expert.py --time    # also times the reference transformer, single thread, on the two packs of
                                                 # DESIGN.md section 4.10 (the same packs tools/expert_bench.py builds)

load_ExpertSolution is not called (no YAML): the schedules are made here.  Each agent follows the reference's own A* path
(offlineExpert/a_star.py) on the static map, random waits are inserted, lengths are ragged and some agents start on their
goals.  THE SCHEDULES ARE NOT COLLISION FREE and need not be: the transformer never checks collisions, it only decodes paths.

Every fixture holds C cases of one configuration (same agent count, map size, guidance, radius rule - what one call of
expert_samples takes), padded to T = max(makespan) + 1 steps; each case went through the reference ON ITS OWN.  Data only:
    in :  map (C,H,W) uint8, paths (C,N,Lmax,2) int32 padded with the last cell, lengths (C,N), goal (C,N,2), start (C,N,2),
          makespan (C,) int32, commR float64, dynamic_commR / symmetric_norm uint8, guidance str
    out:  pos (C,T,N,2) int32, target (C,T,N,5) uint8, valid (C,T) uint8, x (C,T,N,3,11,11) uint8, GSO (C,T,N,N) float64,
          radii (C,) float64, grow_steps (C,) int32 (multiplications by 1.1 behind commR), first_move / end_step (C,N) int32,
          makespanTarget / flowtimeTarget (C,) int32, expert_pos (C,T+1,N,2) int32 (rows behind a case's last step repeat it)"""
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FOV = 9
#        name                               N  size density C  guidance     dynamic symnorm
CASES = [("n10_map20_ProjectG_dyn",          10, 20, 0.10, 5, "Project_G",  True,  False),
         ("n10_map20_LocalG_SD_fixed",       10, 20, 0.10, 5, "LocalG_SD",  False, False),
         ("n12_map10_dense_SemiLG_S_fixed",  12, 10, 0.25, 5, "SemiLG_S",   False, False),
         ("n30_map40_GlobalG_S_dyn_symnorm", 30, 40, 0.05, 5, "GlobalG_S",  True,  True),
         ("n8_map10_idle",                    8, 10, 0.10, 5, "Project_G",  False, False)]
FIXED_R = {"n10_map20_LocalG_SD_fixed": 7.0, "n12_map10_dense_SemiLG_S_fixed": 3.0, "n8_map10_idle": 4.0}


def make_case(rng, astar, N, size, density, p_wait=0.15, on_goal=1, idle=0):
    """One case: map (size,size) int64, per-agent paths (list of (L,2) int64 arrays), goals (N,2).  astar(grid, start, goal) ->
    list of cells from start to goal ([start] when there is no path: that agent's goal becomes its start)."""
    m = (rng.random((size, size)) < density).astype(np.int64)
    free = np.argwhere(m == 0)
    idx = rng.permutation(len(free))
    pos, goal = free[idx[:N]].copy(), free[idx[N:2 * N]].copy()
    for n in range(min(N, on_goal + idle)):
        goal[n] = pos[n]                                     # already at the goal: a path of one cell
    paths = []
    for n in range(N):
        cells = [tuple(int(v) for v in c) for c in astar(m, pos[n], goal[n])]
        if cells[-1] != tuple(goal[n]):
            goal[n] = pos[n]
            cells = [tuple(int(v) for v in pos[n])]
        out = []
        for c in cells:
            out.append(c)
            while len(cells) > 1 and rng.random() < p_wait:  # a wait: the same cell again
                out.append(c)
        paths.append(np.asarray(out, dtype=np.int64).reshape(-1, 2))
    return m, paths, goal.astype(np.int64)


def pad_paths(cases):
    """[(map, paths, goal)] -> paths (C,N,Lmax,2) int32 padded with the last cell, lengths (C,N) int32."""
    Lmax = max(len(p) for _, ps, _ in cases for p in ps)
    C, N = len(cases), len(cases[0][1])
    arr, lengths = np.zeros((C, N, Lmax, 2), np.int32), np.zeros((C, N), np.int32)
    for c, (_, ps, _) in enumerate(cases):
        for n, p in enumerate(ps):
            arr[c, n, :len(p)], arr[c, n, len(p):], lengths[c, n] = p, p[-1], len(p)
    return arr, lengths


def timing_pack(astar, C, N, size, density, seed=7):
    """The packs of DESIGN.md section 4.10: C cases x N agents on a size x size map (tools/expert_bench.py builds the same)."""
    rng = np.random.default_rng(seed)
    return [make_case(rng, astar, N, size, density) for _ in range(C)]


def load_reference():
    for name in ("easydict", "hashids"):                     # imported by the transformer's module, not used on this path
        if name not in sys.modules:
            stub = types.ModuleType(name)
            stub.EasyDict, stub.Hashids = dict, object
            sys.modules[name] = stub
    from oracle.make_golden_sim import load_reference_frontend
    AgentState, Sim = load_reference_frontend()
    import importlib
    DT = importlib.import_module("onlineExpert.DataTransformer_local_onlineExpert").DataTransformer
    planner = importlib.import_module("offlineExpert.a_star").PathPlanner(False)
    return DT, Sim, lambda grid, s, g: planner.a_star(grid, [int(s[0]), int(s[1])], [int(g[0]), int(g[1])])[0]


def transformer(DT, N, size, guidance, commR, dynamic, symnorm):
    cfg = types.SimpleNamespace(num_agents=N, map_w=size, map_h=size, FOV=FOV, guidance=guidance, commR=commR,
                                dynamic_commR=dynamic, symmetric_norm=symnorm, failCases_dir="")
    return DT(cfg)


def reference_schedule(dt, paths, goal, makespan):
    N = len(paths)
    sched = [np.zeros([makespan + 1, N, 2]), np.zeros([makespan + 1, N, 5])]
    plan = {"agent%d" % n: [{"x": int(c[0]), "y": int(c[1])} for c in p] for n, p in enumerate(paths)}
    for n in range(N):
        sched = dt.obtainSchedule(n, plan, sched, goal.astype(np.float64), makespan + 1)
    return sched


def reference_samples(dt, m, paths, goal, makespan):
    """What pathtransformer_RelativeCoordinate puts into its file for one case: state, target, GSO, radius, inputTensor."""
    state, target = reference_schedule(dt, paths, goal, makespan)
    GSO, radius = dt.getAdjacencyMatrix(state, dt.communicationRadius)
    dt.AgentState.setmap(m)
    x = dt.AgentState.toSeqInputTensor(goal.astype(np.float64), state, makespan + 1).numpy()
    return state, target, GSO, float(radius), x


def grow_count(R, radius):
    r, k = float(R), 0
    while r != radius:
        r, k = r * 1.1, k + 1
        assert k < 200
    return k


def reference_stats(Sim, target, start, goal):
    """multiRobotSimNew.getPathTarget on the fields it reads (setup() :158-198 without the files)."""
    import torch
    N = start.shape[0]
    fake = types.SimpleNamespace(config=types.SimpleNamespace(num_agents=N), start_positions=start.astype(np.float64),
                                 goal_positions=goal.astype(np.float64), expert_path_list=[],
                                 List_MultiAgent_ActionVec_target=torch.from_numpy(target).permute(1, 0, 2),      # (N,T,5)
                                 up=np.array([-1, 0]), down=np.array([1, 0]), left=np.array([0, -1]), right=np.array([0, 1]),
                                 stop=np.array([0, 0]), up_keyValue=0, down_keyValue=2, left_keyValue=1, right_keyValue=3,
                                 stop_keyValue=4, expert_first_move=np.zeros(N), expert_end_step=np.zeros(N))
    Sim.getPathTarget(fake)
    return (fake.expert_first_move, fake.expert_end_step, int(fake.makespanTarget), int(fake.flowtimeTarget),
            fake.expert_path_matrix)


def main():
    from make_golden_guidance import save_npz
    from oracle.make_golden_sim import OUT
    DT, Sim, astar = load_reference()
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261017)
    for name, N, size, density, C, guidance, dynamic, symnorm in CASES:
        idle = name.endswith("idle")
        cases = [make_case(rng, astar, N, size, density, on_goal=2 if idle else 1, idle=(N if c == 3 else 2) if idle else 0)
                 for c in range(C)]
        makespan = np.array([max(len(p) for p in ps) - 1 for _, ps, _ in cases], dtype=np.int64)
        if idle:
            # the solver's makespan need not be the longest path: longer (everybody waits at the goal), shorter (the schedule is
            # cut: some agents never arrive), and a case in which nobody moves at all (makespan 0: one step)
            makespan[1] += 3
            makespan[2] = max(1, makespan[2] - 3)
            assert makespan[3] == 0 and len(set(makespan.tolist())) >= 3
        if dynamic:
            # a radius at which a step LATER than 0 triggers growth: k >= 1, and step 0 alone would give a smaller k
            commR, hits = None, 0
            for cand in np.arange(2.0, 12.01, 0.25):
                dt = transformer(DT, N, size, guidance, float(cand), True, symnorm)
                hits = 0
                for (m, ps, goal), mk in zip(cases, makespan):
                    state, _ = reference_schedule(dt, ps, goal, int(mk))
                    k = grow_count(cand, float(dt.computeAdjacencyMatrix(state, float(cand))[1]))
                    k0 = grow_count(cand, float(dt.computeAdjacencyMatrix(state[:1], float(cand))[1]))
                    hits += int(k >= 1 and k0 < k)
                if hits >= 2:
                    commR = float(cand)
                    break
            assert commR is not None, "no radius makes a later step grow the threshold"
        else:
            commR = FIXED_R[name]
        dt = transformer(DT, N, size, guidance, commR, dynamic, symnorm)
        T = int(makespan.max()) + 1
        paths, lengths = pad_paths(cases)
        out = dict(pos=np.zeros((C, T, N, 2), np.int32), target=np.zeros((C, T, N, 5), np.uint8), valid=np.zeros((C, T), np.uint8),
                   x=np.zeros((C, T, N, 3, FOV + 2, FOV + 2), np.uint8), GSO=np.zeros((C, T, N, N), np.float64),
                   radii=np.zeros(C, np.float64), grow_steps=np.zeros(C, np.int32), first_move=np.zeros((C, N), np.int32),
                   end_step=np.zeros((C, N), np.int32), makespanTarget=np.zeros(C, np.int32), flowtimeTarget=np.zeros(C, np.int32),
                   expert_pos=np.zeros((C, T + 1, N, 2), np.int32))
        later = 0
        for c, ((m, ps, goal), mk) in enumerate(zip(cases, makespan)):
            Tc = int(mk) + 1
            state, target, GSO, radius, x = reference_samples(dt, m, ps, goal, int(mk))
            assert x.shape == (Tc, N, 3, FOV + 2, FOV + 2) and set(np.unique(x)) <= {0.0, 1.0} and GSO.shape == (Tc, N, N)
            assert np.array_equal(state, np.round(state)) and (target.sum(-1) == 1).all()
            assert int(x[:, :, 1].sum(axis=(2, 3)).max()) < dt.AgentState.max_localPath or guidance == "Project_G"
            start = np.stack([p[0] for p in ps])
            fm, es, mkT, flT, epos = reference_stats(Sim, target, start, goal)
            out["pos"][c, :Tc], out["target"][c, :Tc], out["valid"][c, :Tc] = state, target, 1
            out["x"][c, :Tc], out["GSO"][c, :Tc], out["radii"][c] = x, GSO, radius
            out["grow_steps"][c] = grow_count(commR, radius)
            out["first_move"][c], out["end_step"][c], out["makespanTarget"][c], out["flowtimeTarget"][c] = fm, es, mkT, flT
            assert epos.shape == (Tc + 1, N, 2) and np.array_equal(epos, np.round(epos))
            out["expert_pos"][c, :Tc + 1], out["expert_pos"][c, Tc + 1:] = epos, epos[-1]
            if dynamic:
                k0 = grow_count(commR, float(dt.computeAdjacencyMatrix(state[:1], commR)[1]))
                later += int(out["grow_steps"][c] >= 1 and k0 < out["grow_steps"][c])
        if dynamic:
            assert later >= 1, name
        if idle:
            assert (out["first_move"] == 0).any() and (out["end_step"][2] == 0).any() and (out["first_move"][3] == 0).all()
        path = os.path.join(OUT, "expert_%s.npz" % name)
        save_npz(path, map=np.stack([m for m, _, _ in cases]).astype(np.uint8), paths=paths, lengths=lengths,
                 goal=np.stack([g for _, _, g in cases]).astype(np.int32), start=paths[:, :, 0].copy(),
                 makespan=makespan.astype(np.int32), commR=np.float64(commR), dynamic_commR=np.uint8(dynamic),
                 symmetric_norm=np.uint8(symnorm), guidance=np.array(guidance), **out)
        print("wrote", path, os.path.getsize(path) // 1024, "KB", "commR", commR, "makespan", makespan.tolist(), "grow_steps",
              out["grow_steps"].tolist(), "cases whose growth comes from a later step:", later)
        assert os.path.getsize(path) < 1000 * 1000
    if "--time" in sys.argv:
        for C, N, size, density in ((64, 10, 20, 0.10), (8, 100, 50, 0.08)):
            pack = timing_pack(astar, C, N, size, density)
            steps = sum(max(len(p) for p in ps) for _, ps, _ in pack)
            for guidance in ("Project_G", "LocalG_SD", "GlobalG_SD", "SemiLG_SD"):
                dt = transformer(DT, N, size, guidance, 7.0, True, False)
                t0 = time.perf_counter()
                for m, ps, goal in pack:
                    reference_samples(dt, m, ps, goal, max(len(p) for p in ps) - 1)
                dtm = time.perf_counter() - t0
                print("reference transformer, one CPU thread: %d cases x %d agents, %s: %.2f s for %d steps = %.3f ms per agent "
                      "and step" % (C, N, guidance, dtm, steps, 1e3 * dtm / (steps * N)), flush=True)


if __name__ == "__main__":
    main()
