"""The case pool on the device (magat_pathplanning_amd/rollout.py, csrc/sim_pool.hip): against the reference's
fixtures, against the same cases run alone in BatchedEpisode (bit for bit), the SemiLG view across refills, the wide move step,
graph capture, and a model in the loop.  Integer results: every comparison is equality."""
import os

import numpy as np
import pytest
import torch

import rollout_cases as rc
import rollout_restatement as rr

pytestmark = pytest.mark.gpu


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def pool_rows(pool):
    res = {k: v.cpu().numpy() for k, v in pool.results().items()}
    assert (res["retired"] == 1).all()
    return [{k: res[k][c] for k in res} for c in range(pool.C)]


# ---- 1. the reference's fixtures ----------------------------------------------------------------------------------------------------------
def run_fixture_pool(z, start, slots, first_step, maxstep, dev):
    from magat_pathplanning_amd import EpisodePool
    policy = int(z["policy"])
    pool = EpisodePool(dv(z["map"], dev), dv(start, dev), dv(z["goal"], dev), maxstep, slots, 7.0,
                       action_select=rc.ACTION_SELECT[policy], first_step=first_step)
    N = pool.N
    for _ in range(pool.max_calls() + 1):
        case, step = pool.slot_case.cpu().numpy(), pool.slot_step.cpu().numpy()
        lg = np.stack([z["logits"][c, t] if c >= 0 else np.zeros((N, 5), np.float32) for c, t in zip(case, step)])
        u = np.stack([z["uniforms"][c, t] if c >= 0 else np.zeros(N) for c, t in zip(case, step)])
        pool.step(logits=dv(lg, dev), uniforms=dv(u, dev) if policy else None)
        if pool.finished():
            break
    assert pool.finished()
    return pool


@pytest.mark.parametrize("path", rc.EPISODE, ids=[os.path.basename(p)[:-4] for p in rc.EPISODE])
def test_pool_equals_the_episode_fixtures(gpu_device, path):
    z = np.load(path)
    B = z["pos0"].shape[0]
    pool = run_fixture_pool(z, z["pos0"], 2 if B > 2 else 1, 0, int(z["maxstep"]), gpu_device)
    rc.assert_rows_equal(pool_rows(pool), rc.episode_rows(z), os.path.basename(path))
    assert (pool.results()["flag_bits"].cpu().numpy() & 48 == 0).all()


@pytest.mark.parametrize("path", rc.ROLLOUT, ids=[os.path.basename(p)[:-4] for p in rc.ROLLOUT])
def test_pool_equals_the_rollout_fixtures_and_the_monitor(gpu_device, path):
    from magat_pathplanning_amd import summarize_rollouts
    z = np.load(path)
    pool = run_fixture_pool(z, z["start"], 2, 1, dv(z["maxstep"].astype(np.int32), gpu_device), gpu_device)
    rc.assert_rows_equal(pool_rows(pool), rc.rollout_rows(z), os.path.basename(path))
    s = summarize_rollouts(pool.results(), dv(z["makespanTarget"], gpu_device), dv(z["flowtimeTarget"], gpu_device))
    rc.assert_summary_equals_fixture(s, z)


# ---- 2. pool equals alone -------------------------------------------------------------------------------------------------------------------
def alone_cases(dev):
    from magat_pathplanning_amd import generate_cases
    a = rc.ALONE
    cases = generate_cases(a["C"], a["H"], a["W"], a["N"], density=a["density"], complexity=a["complexity"], kind="maze",
                           seed=a["seed"], device=dev)
    assert bool(cases["valid"].all())
    goal = cases["goal"].clone()
    for c in a["on_start"]:
        goal[c] = cases["start"][c]
    return cases["map"], cases["start"], goal


def case_uniforms(c, t, N, seed, dev):
    from magat_pathplanning_amd import _native as nat
    case = torch.tensor([c], dtype=torch.int32, device=dev)
    step = torch.tensor([t], dtype=torch.int32, device=dev)
    u = torch.empty(1, N, dtype=torch.float64, device=dev)
    nat.check(nat.lib().magat_sim_pool_uniforms(nat.ptr(case), nat.ptr(step), nat.ptr(u), seed, 1, N, nat.current_stream(dev)),
              "magat_sim_pool_uniforms")
    return u


_alone = {}


def run_alone(dev, action_select, guidance="Project_G"):
    """Every case of the set by itself in BatchedEpisode, currentstep 1 before the first step, to its finalising call."""
    key = (action_select, guidance)
    if key in _alone:
        return _alone[key]
    from magat_pathplanning_amd import BatchedEpisode
    maps, start, goal = alone_cases(dev)
    a = rc.ALONE
    rows = []
    for c in range(a["C"]):
        M = a["maxstep"][c]
        ep = BatchedEpisode(maps[c:c + 1], start[c:c + 1], goal[c:c + 1], M, a["comm_radius"], action_select=action_select,
                            guidance=guidance)
        ep.gso()
        ep.currentstep = 1
        sticky, traj = 0, [ep.pos[0].cpu().numpy().copy()]
        for t in range(1, M + 1):
            u = case_uniforms(c, t, a["N"], a["pool_seed"], dev) if ep.policy else None
            done = int(ep.step(logits=rc.push_logits_torch(ep.pos, ep.goal), uniforms=u)[0])
            sticky |= int(ep.flags[0])
            if done or t >= M:
                break
            traj.append(ep.pos[0].cpu().numpy().copy())
        rows.append(dict(retired=1, all_reach=done, num_reach=int(ep.reach_goal.sum()), steps=t, makespan=int(ep.makespan[0]),
                         flowtime=int(ep.flowtime[0]), predicted_collision=int(sticky & 15 != 0), flag_bits=sticky, status=0,
                         radius=float(ep.radii[0]), end_pos=ep.pos[0].cpu().numpy(), first_move=ep.first_move[0].cpu().numpy(),
                         end_step=ep.end_step[0].cpu().numpy(), traj=np.stack(traj)))
    _alone[key] = rows
    return rows


@pytest.mark.parametrize("action_select", ["soft_max", "exp_multinorm"])
@pytest.mark.parametrize("slots", [1, 3, 7])
def test_pool_equals_alone(gpu_device, slots, action_select):
    from magat_pathplanning_amd import EpisodePool, audit_schedules
    maps, start, goal = alone_cases(gpu_device)
    a = rc.ALONE
    alone = run_alone(gpu_device, action_select)
    assert alone[4]["steps"] == 1 and {r["all_reach"] for r in alone} == {0, 1} and any(r["radius"] > a["comm_radius"] for r in alone)
    pool = EpisodePool(maps, start, goal, torch.tensor(a["maxstep"], dtype=torch.int32, device=gpu_device), slots, a["comm_radius"],
                       action_select=action_select, seed=a["pool_seed"], first_step=1, record=True)
    for _ in range(pool.max_calls() + 1):
        pool.step(logits=rc.push_logits_torch(pool.pos, pool.goal))
        if pool.finished():
            break
    got = pool_rows(pool)
    for c in range(a["C"]):
        for key in rr.COLUMNS:                               # every column, the radius bit for bit
            np.testing.assert_array_equal(got[c][key], alone[c][key], err_msg="case %d %s" % (c, key))
    pack = pool.trajectory_pack()
    paths, lengths = pack["paths"].cpu().numpy(), pack["lengths"].cpu().numpy()
    for c in range(a["C"]):
        L = len(alone[c]["traj"])
        assert (lengths[c] == L).all()
        np.testing.assert_array_equal(paths[c, :, :L], alone[c]["traj"].transpose(1, 0, 2))
    audit = audit_schedules(maps, pack)
    assert (audit["status"].cpu().numpy() == 0).all(), audit["fault"].cpu().numpy()
    # the restatement tells the same story
    ref = rr.Pool(maps.cpu().numpy(), start.cpu().numpy(), goal.cpu().numpy(), a["maxstep"], slots, a["comm_radius"],
                  policy=pool.policy, seed=a["pool_seed"], first_step=1)
    rr.run(ref, lambda p: rc.push_logits_numpy(p.pos(), p.slot_goal()))
    for c in range(a["C"]):
        for key in rr.COLUMNS:
            np.testing.assert_array_equal(got[c][key], ref.rows[c][key], err_msg="restatement, case %d %s" % (c, key))


def test_idle_slots_keep_their_positions_and_status_reports_a_disconnected_case(gpu_device):
    from magat_pathplanning_amd import EpisodePool
    m = torch.zeros(8, 8, dtype=torch.uint8, device=gpu_device)
    start = torch.tensor([[[0, 0], [0, 2]], [[1, 0], [7, 7]], [[3, 3], [3, 5]]], dtype=torch.int32, device=gpu_device)
    goal = torch.tensor([[[5, 5], [5, 3]]] * 3, dtype=torch.int32, device=gpu_device)
    # radius 1e-3: 64 growth steps reach 1e-3 * 1.1^63 = 0.4 < 1, no pair ever connects
    pool = EpisodePool(m, start, goal, 2, 2, 1e-3, first_step=1)
    stop = torch.full((2, 2), 4, dtype=torch.int32, device=gpu_device)
    for _ in range(4):
        pool.step(actions=stop)
    assert pool.finished() and pool.slot_case.tolist() == [-1, -1]
    res = pool.results()
    assert res["status"].tolist() == [2, 2, 2] and res["steps"].tolist() == [2, 2, 2]
    r = 1e-3 / 1.1
    for _ in range(64):
        r = r * 1.1
    assert res["radius"].tolist() == [r] * 3 and r < 1.0
    np.testing.assert_array_equal(pool.pos.cpu().numpy(), [[[3, 3], [3, 5]], [[1, 0], [7, 7]]])      # the last cases' cells
    before = (pool.pos.clone(), pool.slot_step.clone())
    pool.step(actions=stop)                                   # an idle pool: nothing moves, states() and gso() stay defined
    assert torch.equal(pool.pos, before[0]) and torch.equal(pool.slot_step, before[1])
    assert pool.states().shape == (2, 2, 3, 11, 11) and pool.gso().shape == (2, 2, 2)


# ---- 3. SemiLG: the view is reset on refill ---------------------------------------------------------------------------------------------------
def test_semilg_states_equal_alone_across_refills(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, EpisodePool
    maps, start, goal = alone_cases(gpu_device)
    idx = torch.tensor([0, 1, 3], device=gpu_device)
    maps, start, goal = maps[idx], start[idx], goal[idx]
    pool = EpisodePool(maps, start, goal, 3, 1, 7.0, guidance="SemiLG_S", first_step=1)
    seen, ep, last = [], None, -1
    for _ in range(9):
        c = int(pool.slot_case[0])
        if c < 0:
            break
        if c != last:
            ep = BatchedEpisode(maps[c:c + 1], start[c:c + 1], goal[c:c + 1], 3, 7.0, guidance="SemiLG_S")
            ep.currentstep = 1
            last = c
        x = pool.states()
        assert torch.equal(x, ep.states()), "case %d step %d" % (c, int(pool.slot_step[0]))
        assert torch.equal(pool.agent_view, ep.agent_view)
        seen.append(c)
        lg = rc.push_logits_torch(pool.pos, pool.goal)
        ep.step(logits=lg.clone())
        pool.step(logits=lg)
    assert seen == [0, 0, 0, 1, 1, 1, 2, 2, 2] and pool.finished()


# ---- 4. the wide move step --------------------------------------------------------------------------------------------------------------------
def test_wide_pool_equals_wide_alone(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, EpisodePool
    from magat_pathplanning_amd.simulator import move_needs_wide
    H = W = 208
    assert move_needs_wide(H, W, 4)
    m = torch.zeros(H, W, dtype=torch.uint8, device=gpu_device)
    start = torch.tensor([[[0, 0], [0, 1], [207, 207], [100, 100]], [[5, 5], [5, 7], [206, 0], [0, 206]]], dtype=torch.int32,
                         device=gpu_device)
    goal = torch.tensor([[[3, 0], [0, 0], [207, 205], [100, 101]], [[5, 6], [5, 6], [207, 0], [0, 207]]], dtype=torch.int32,
                        device=gpu_device)
    pool = EpisodePool(m, start, goal, 4, 1, 300.0, wide=True, first_step=1)
    for _ in range(pool.max_calls()):
        pool.step(logits=rc.push_logits_torch(pool.pos, pool.goal))
    assert pool.finished()
    got = pool_rows(pool)
    for c in range(2):
        ep = BatchedEpisode(m, start[c:c + 1], goal[c:c + 1], 4, 300.0, wide=True)
        ep.currentstep = 1
        sticky = 0
        for t in range(1, 5):
            done = int(ep.step(logits=rc.push_logits_torch(ep.pos, ep.goal))[0])
            sticky |= int(ep.flags[0])
            if done or t >= 4:
                break
        want = dict(all_reach=done, num_reach=int(ep.reach_goal.sum()), steps=t, makespan=int(ep.makespan[0]),
                    flowtime=int(ep.flowtime[0]), flag_bits=sticky, end_pos=ep.pos[0].cpu().numpy(),
                    first_move=ep.first_move[0].cpu().numpy(), end_step=ep.end_step[0].cpu().numpy())
        for key, v in want.items():
            np.testing.assert_array_equal(got[c][key], v, err_msg="case %d %s" % (c, key))
    assert got[0]["flag_bits"] & 8 or got[1]["flag_bits"] & 8     # agents 0 / 1 of case 1 claim one cell


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_step_is_capturable(gpu_device):
    from magat_pathplanning_amd import EpisodePool
    maps, start, goal = alone_cases(gpu_device)
    a = rc.ALONE
    maxstep = torch.tensor(a["maxstep"], dtype=torch.int32, device=gpu_device)
    keys = torch.tensor([[0, 1, 2, 3], [2, 2, 4, 1], [3, 0, 1, 2]], dtype=torch.int32, device=gpu_device)
    new = lambda: EpisodePool(maps, start, goal, maxstep, 3, a["comm_radius"], first_step=1, record=True)      # noqa: E731
    k = 12
    eager = new()
    for _ in range(k):
        eager.step(actions=keys)
    warm = new()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        warm.step(actions=keys)
    torch.cuda.current_stream().wait_stream(side)
    pool = new()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pool.step(actions=keys)
    for _ in range(k):
        graph.replay()
    torch.cuda.synchronize()
    assert int(eager.results()["retired"].sum()) >= 4         # refills happened inside the replays
    for name in ("pos", "goal", "map", "reach_goal", "first_move", "end_step", "actions", "moves", "flags", "radii", "slot_case",
                 "slot_step", "counters", "sticky"):
        assert torch.equal(getattr(pool, name), getattr(eager, name)), name
    for key, v in eager.results().items():
        assert torch.equal(pool.results()[key], v), key
    assert torch.equal(pool._traj, eager._traj) and torch.equal(pool._traj_len, eager._traj_len)


# ---- 6. a model in the loop -------------------------------------------------------------------------------------------------------------------
def test_evaluate_cases_with_a_model(gpu_device):
    from magat_pathplanning_amd import DecentralPlannerGATNet, evaluate_cases, generate_cases, summarize_rollouts
    from magat_pathplanning_amd.synthetic import make_config
    from oracle import magat_oracle as orc
    cfg = make_config(num_agents=4, nGraphFilterTaps=2, nAttentionHeads=1, device=str(gpu_device), bottleneckMode="BottomNeck_only")
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(orc.init_state_dict(cfg, seed=7))
    net = net.to(gpu_device).eval()
    cases = generate_cases(6, 10, 10, 4, density=0.2, complexity=0.05, seed=31, device=gpu_device)
    assert bool(cases["valid"].all())
    maxstep = torch.tensor([4, 9, 6, 12, 3, 8], dtype=torch.int32, device=gpu_device)
    res = evaluate_cases(net, cases["map"], cases["start"], cases["goal"], maxstep, 2, 7.0, poll=4, action_select="exp_multinorm", seed=5)
    r = {k: v.cpu().numpy() for k, v in res.items()}
    assert (r["retired"] == 1).all() and (r["steps"] <= r["maxstep"]).all() and (r["steps"] >= 1).all() and (r["status"] == 0).all()
    goal = cases["goal"].cpu().numpy()
    assert ((r["num_reach"] >= 0) & (r["num_reach"] <= 4)).all()
    for c in range(6):
        at_goal = (r["end_pos"][c] == goal[c]).all(axis=1)
        assert at_goal.sum() <= r["num_reach"][c] <= 4        # whoever stands on its goal has reached it (the flag is sticky)
        if r["all_reach"][c]:
            assert r["num_reach"][c] == 4 and r["steps"][c] >= 2 and (r["end_step"][c] < r["steps"][c]).all()
        else:
            assert r["steps"][c] == r["maxstep"][c]
        assert (r["first_move"][c] <= r["steps"][c]).all() and (r["end_step"][c] <= r["steps"][c]).all()
        assert r["makespan"][c] == r["end_step"][c].max() - r["first_move"][c].min() + 1
        assert r["flowtime"][c] == (r["end_step"][c] - r["first_move"][c] + 1).sum()
        assert r["predicted_collision"][c] == int(r["flag_bits"][c] & 15 != 0)
    mkT, ftT = np.array([3, 5, 4, 7, 2, 5]), np.array([9, 15, 12, 20, 6, 14])
    s = summarize_rollouts(res, torch.from_numpy(mkT).to(gpu_device), torch.from_numpy(ftT).to(gpu_device))
    rows = [{k: r[k][c] for k in r} for c in range(6)]
    log, want = rr.summary(rows, r["maxstep"], mkT, ftT, 4)
    for key in rc.LOG_FIELDS:
        np.testing.assert_array_equal(np.asarray(s[key]).astype(np.int64), np.array([l[key] for l in log]).astype(np.int64), err_msg=key)
    for key in rc.RATES:
        np.testing.assert_allclose(s[key], want[key], rtol=1e-12, atol=0, err_msg=key)
    np.testing.assert_array_equal(s["hist_numAgentReachGoal"], want["hist_numAgentReachGoal"])
