"""Generates tests/golden/rollout_*.npz with the REAL reference (build container only; never imported by a test):
multiRobotSimNew.move driven through the agent's validation loop (agents/decentralplannerlocal_OnlineExpert_GAT.py:859-957:
currentStep = step + 1, break on allReachGoal or currentStep >= maxstep, then checkOptimality), every case with its own
maxstep = int(makespanTarget * rate) from the reference's getPathTarget on an expert schedule of tests/mapf_restatement.py, and the
per-case log_result fed into the real MonitoringMultiAgentPerformance (utils/metrics.py, loaded by file path).

    python tools/make_golden_rollout.py

random.choice and torch.multinomial are pinned as in oracle/make_golden_sim_episode.py (first element; inverse CDF over recorded
uniforms).  Fixtures hold data only: map, start, goal, the expert's one-hot targets, maxstep, per-step logits and uniforms (indexed
by currentStep), the log_result fields without the two wall-clock entries, and the monitor's summary numbers."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mapf_restatement as mr  # noqa: E402
from oracle._ref_import import REF_ROOT  # noqa: E402
from oracle.make_golden_sim import load_reference_frontend  # noqa: E402
from oracle.make_golden_sim_episode import Uniforms, make_sim, step_logits  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KEY_OF_MOVE = {m: k for k, m in enumerate(mr.MOVES)}


def load_monitor():
    spec = importlib.util.spec_from_file_location("reference_metrics", os.path.join(REF_ROOT, "utils", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MonitoringMultiAgentPerformance


def expert_targets(paths, T):
    """paths (N,T,2), padded with the last cell -> one-hot action targets (N,T-1,5) uint8."""
    N = paths.shape[0]
    out = np.zeros((N, T - 1, 5), np.uint8)
    for n in range(N):
        for t in range(T - 1):
            d = tuple(int(v) for v in paths[n, t + 1] - paths[n, t])
            out[n, t, KEY_OF_MOVE[d]] = 1
    return out


def path_target(Sim, N, start, goal, target):
    """The reference's getPathTarget on the one-hot targets: (makespanTarget, flowtimeTarget)."""
    cfg = types.SimpleNamespace(num_agents=N)
    s = types.SimpleNamespace(config=cfg, start_positions=start.astype(np.float64).copy(), goal_positions=goal.astype(np.float64).copy(),
                              expert_path_list=[], expert_first_move=np.zeros(N), expert_end_step=np.zeros(N),
                              List_MultiAgent_ActionVec_target=torch.from_numpy(target.astype(np.float32)),
                              up=np.array([-1, 0]), down=np.array([1, 0]), left=np.array([0, -1]), right=np.array([0, 1]),
                              stop=np.array([0, 0]), up_keyValue=0, down_keyValue=2, left_keyValue=1, right_keyValue=3, stop_keyValue=4)
    Sim.getPathTarget(s)
    return int(s.makespanTarget), int(s.flowtimeTarget)


def rollout(Sim, simmod, name, N, size, density, C, policy, rate, sharp, seed, need_timeout):
    rng = np.random.default_rng(seed)
    uni = Uniforms()
    simmod.random.choice = lambda l: l[0]
    real_multinomial = torch.multinomial
    torch.multinomial = uni.multinomial
    Monitor = load_monitor()
    mon = Monitor(types.SimpleNamespace(num_agents=N))
    mon.reset()
    rec = {k: [] for k in ("map", "start", "goal", "target", "maxstep", "makespanTarget", "flowtimeTarget", "logits", "uniforms",
                           "allReachGoal", "noReachGoalbyCollisionShielding", "findOptimalSolution", "check_collisionFreeSol",
                           "check_CollisionPredictedinLoop", "compare_makespan", "compare_flowtime", "num_agents_reachgoal",
                           "steps", "end_pos", "first_move", "end_step")}
    T = 4 * size
    try:
        for c in range(C):
            while True:
                m, start, goal = mr.random_case(rng, size, size, N, density)
                plan = mr.solve_with_retries(m, start, goal, T)
                if plan["solved"]:
                    break
            if c == 1:
                goal[0] = start[0]                        # an agent that starts on its goal
                plan = mr.solve_with_retries(m, start, goal, T)
                assert plan["solved"]
            target = expert_targets(np.asarray(plan["paths"]), T)
            mkT, ftT = path_target(Sim, N, start, goal, target)
            rate_maxstep = 3 if N >= 20 else rate         # setup(): new_simulator.py:204-210
            maxstep = int(torch.tensor(mkT).type(torch.int32) * rate_maxstep)
            s = make_sim(Sim, N, m, start.astype(np.int64), goal.astype(np.int64), maxstep, policy)
            s.makespanTarget, s.flowtimeTarget = mkT, ftT
            logits = np.zeros((maxstep + 1, N, 5), np.float32)
            us = np.zeros((maxstep + 1, N), np.float64)
            all_reach = predicted = happened = False
            current = 0
            for step in range(maxstep):                   # the agent's loop (:880-916)
                current = step + 1
                lg = step_logits(rng, s.current_positions.astype(np.int64), goal, policy, sharp)
                u = rng.random(N)
                uni.queue = list(u) if policy else []
                logits[current], us[current] = lg, u
                all_reach, move_collision, predict = Sim.move(s, [torch.from_numpy(lg[i:i + 1]) for i in range(N)], current)
                happened |= bool(move_collision)
                predicted |= bool(predict)
                if all_reach or current >= maxstep:
                    break
            num_reach = int(Sim.count_numAgents_ReachGoal(s))
            shield = free_sol = optimal = False           # the loop's epilogue (:918-936)
            cmp_mk, cmp_ft = [s.makespanPredict, mkT], [s.flowtimePredict, ftT]
            if all_reach and not happened:
                free_sol = True
                optimal, cmp_mk, cmp_ft = Sim.checkOptimality(s, True)
            if current >= maxstep:
                optimal, cmp_mk, cmp_ft = Sim.checkOptimality(s, False)
            if current >= maxstep and not all_reach and predicted and not happened:
                optimal, cmp_mk, cmp_ft = Sim.checkOptimality(s, False)
                shield = True
            mon.update(maxstep, [all_reach, shield, optimal, free_sol, predicted, cmp_mk, cmp_ft, num_reach, 0.0, []])
            for k, v in (("map", m.astype(np.uint8)), ("start", start.astype(np.int32)), ("goal", goal.astype(np.int32)),
                         ("target", target), ("maxstep", maxstep), ("makespanTarget", mkT), ("flowtimeTarget", ftT),
                         ("logits", logits), ("uniforms", us), ("allReachGoal", int(all_reach)),
                         ("noReachGoalbyCollisionShielding", int(shield)), ("findOptimalSolution", int(optimal)),
                         ("check_collisionFreeSol", int(free_sol)), ("check_CollisionPredictedinLoop", int(predicted)),
                         ("compare_makespan", [int(v) for v in cmp_mk]), ("compare_flowtime", [int(v) for v in cmp_ft]),
                         ("num_agents_reachgoal", num_reach), ("steps", current),
                         ("end_pos", s.current_positions.astype(np.int32).copy()), ("first_move", s.first_move.astype(np.int32).copy()),
                         ("end_step", s.end_step.astype(np.int32).copy())):
                rec[k].append(v)
    finally:
        torch.multinomial = real_multinomial
    writer = types.SimpleNamespace(add_scalar=lambda *a, **k: None)
    mon.summary("valid", writer, 0)
    timeouts = sum(1 for st, mx, ar in zip(rec["steps"], rec["maxstep"], rec["allReachGoal"]) if st >= mx and not ar)
    assert not need_timeout or timeouts >= 1, "no case timed out: raise the density or lower the rate"
    Tmax = max(rec["maxstep"]) + 1
    pad = lambda a: np.concatenate([a, np.zeros((Tmax - len(a),) + a.shape[1:], a.dtype)])      # noqa: E731
    rec["logits"] = [pad(a) for a in rec["logits"]]
    rec["uniforms"] = [pad(a) for a in rec["uniforms"]]
    summary = dict(count_validset=mon.count_validset, rateReachGoal=mon.rateReachGoal, rateFailedReachGoalSH=mon.rateFailedReachGoalSH,
                   ratefindOptimalSolution=mon.ratefindOptimalSolution, rateCollsionFreeSol=mon.rateCollsionFreeSol,
                   rateCollisionPredictedinLoop=mon.rateCollisionPredictedinLoop, avg_rate_deltaMP=mon.avg_rate_deltaMP,
                   std_rate_deltaMP=mon.std_rate_deltaMP, avg_rate_deltaFT=mon.avg_rate_deltaFT, std_rate_deltaFT=mon.std_rate_deltaFT)
    path = os.path.join(OUT, "rollout_%s.npz" % name)
    np.savez_compressed(path, policy=np.int32(policy), rate_maxstep=np.float64(rate),
                        rate_deltaMP=np.array(mon.list_rate_deltaMP, np.float64), rate_deltaFT=np.array(mon.list_rate_deltaFT, np.float64),
                        hist_numAgentReachGoal=np.array([mon.list_numAgentReachGoal.count(i) for i in range(N + 1)], np.int64),
                        **{"summary_" + k: np.float64(v) for k, v in summary.items()},
                        **{k: np.stack([np.asarray(x) for x in v]) for k, v in rec.items()})
    print("wrote", path, os.path.getsize(path) // 1024, "KB; maxstep", rec["maxstep"], "steps", rec["steps"], "all reach",
          rec["allReachGoal"], "timeouts", timeouts)


def main():
    _, Sim = load_reference_frontend()
    simmod = sys.modules["utils.new_simulator"]
    rollout(Sim, simmod, "n4_map8_softmax", 4, 8, 0.05, 6, 0, 2, 6.0, 88001, False)
    rollout(Sim, simmod, "n8_map10_dense_exp", 8, 10, 0.10, 5, 2, 2.5, 5.0, 88002, True)


if __name__ == "__main__":
    main()
