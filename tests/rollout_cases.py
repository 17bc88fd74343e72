"""Shared by tests/test_host_rollout.py and tests/test_gpu_rollout.py - TEST HELPER: the "pool equals alone" case set, the
deterministic policy both suites step it with, and readers of the committed fixtures."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROLLOUT = sorted(glob.glob(os.path.join(GOLDEN, "rollout_*.npz")))
EPISODE = sorted(glob.glob(os.path.join(GOLDEN, "simepisode_*.npz")))
ACTION_SELECT = {0: "soft_max", 1: "sum_multinorm", 2: "exp_multinorm"}

# the set: 7 maze cases of 10 x 10 / 4 agents; limits from 1 (the first call finalises) to 20; in cases 2 and 5 every goal is
# moved onto its start (all agents arrive with the first move's reach test - the episode ends by arrival at the second call)
ALONE = dict(C=7, H=10, W=10, N=4, density=0.3, complexity=0.05, seed=4242, maxstep=[3, 9, 5, 12, 1, 7, 20], on_start=(2, 5),
             comm_radius=2.0, pool_seed=99)
MOVES = np.array([[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]], np.int64)


def alone_cases_numpy():
    import cases_restatement as cr
    a = ALONE
    out = cr.generate("maze", a["C"], a["H"], a["W"], a["N"], density=a["density"], complexity=a["complexity"], seed=a["seed"])
    assert out["valid"].all()
    goal = out["goal"].copy()
    for c in a["on_start"]:
        goal[c] = out["start"][c]
    return out["map"], out["start"].astype(np.int32), goal.astype(np.int32)


def push_logits_numpy(pos, goal):
    """(B,N,5) float32: minus twice the Manhattan distance to the goal after each of the five moves - small integers, so that
    numpy and torch give the same floats."""
    nxt = np.asarray(pos, np.int64)[:, :, None, :] + MOVES[None, None]
    return (-2 * np.abs(nxt - np.asarray(goal, np.int64)[:, :, None, :]).sum(-1)).astype(np.float32)


def push_logits_torch(pos, goal):
    import torch
    mv = torch.from_numpy(MOVES).to(pos.device)
    nxt = pos.long()[:, :, None, :] + mv[None, None]
    return (-2 * (nxt - goal.long()[:, :, None, :]).abs().sum(-1)).float()


def episode_rows(z):
    """The state of every instance of a simepisode_* fixture at its first finalising call (currentstep from 0)."""
    maxstep = int(z["maxstep"])
    rows = []
    for b in range(z["pos0"].shape[0]):
        t = next(t for t in range(z["done"].shape[1]) if z["done"][b, t] or t >= maxstep)
        rows.append(dict(all_reach=int(z["done"][b, t]), num_reach=int(z["reach"][b, t].sum()), steps=t,
                         makespan=int(z["makespan"][b, t]), flowtime=int(z["flowtime"][b, t]),
                         predicted_collision=int(z["predict_collision"][b, :t + 1].any()), end_pos=z["pos"][b, t],
                         first_move=z["first_move"][b, t], end_step=z["end_step"][b, t]))
    return rows


def rollout_rows(z):
    """The rows a rollout_* fixture expects (first_step = 1)."""
    return [dict(all_reach=int(z["allReachGoal"][c]), num_reach=int(z["num_agents_reachgoal"][c]), steps=int(z["steps"][c]),
                 makespan=int(z["compare_makespan"][c, 0]), flowtime=int(z["compare_flowtime"][c, 0]),
                 predicted_collision=int(z["check_CollisionPredictedinLoop"][c]), end_pos=z["end_pos"][c],
                 first_move=z["first_move"][c], end_step=z["end_step"][c]) for c in range(len(z["steps"]))]


LOG_FIELDS = ("allReachGoal", "noReachGoalbyCollisionShielding", "findOptimalSolution", "check_collisionFreeSol",
              "check_CollisionPredictedinLoop", "compare_makespan", "compare_flowtime", "num_agents_reachgoal")
RATES = ("rateReachGoal", "rateFailedReachGoalSH", "ratefindOptimalSolution", "rateCollsionFreeSol", "rateCollisionPredictedinLoop",
         "avg_rate_deltaMP", "std_rate_deltaMP", "avg_rate_deltaFT", "std_rate_deltaFT")


def assert_rows_equal(got, want, what=""):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        for key, v in w.items():
            np.testing.assert_array_equal(np.asarray(g[key]), np.asarray(v), err_msg="%s case %d %s" % (what, c, key))


def assert_summary_equals_fixture(s, z, rtol=1e-12):
    """s: summarize_rollouts' dict (arrays per field) against the fixture's log_result fields and the monitor's numbers."""
    for key in LOG_FIELDS:
        np.testing.assert_array_equal(np.asarray(s[key]).astype(np.int64), z[key].astype(np.int64), err_msg=key)
    for key in RATES:
        np.testing.assert_allclose(s[key], float(z["summary_" + key]), rtol=rtol, atol=0, err_msg=key)
    np.testing.assert_allclose(s["rate_deltaMP"], z["rate_deltaMP"], rtol=rtol, atol=0)
    np.testing.assert_allclose(s["rate_deltaFT"], z["rate_deltaFT"], rtol=rtol, atol=0)
    np.testing.assert_array_equal(s["hist_numAgentReachGoal"], z["hist_numAgentReachGoal"])
    assert s["count_validset"] == int(z["summary_count_validset"])
