"""GPU: the path-finding expert (csrc/sim_mapf.hip through magat_pathplanning_amd/mapf.py) EQUALS its cell-by-cell
restatement (tests/mapf_restatement.py, pinned on the CPU by tests/test_host_mapf.py) - paths, lengths, makespan, solved and
failed_agent, unsolved cases included - on hand cases, seeded random batches and the edges of the word / lane / LDS layout;
solve_cases equals solve_with_retries; the schedules replay through BatchedEpisode and feed expert_samples."""
import functools

import numpy as np
import pytest
import torch

import mapf_restatement as mr
from test_host_mapf import SEED_10x10

pytestmark = pytest.mark.gpu
PLAN_KEYS = ("paths", "lengths", "makespan", "solved", "failed_agent")


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf"]))


def ring64():
    """64 x 64 with only the outermost ring free: four agents walk it clockwise along row 0, column 63, row 63 and column 0
    into the four corners (bit 63, lane 63).  A shift that wrapped around a word or the wave would arrive in 2 steps, not 62."""
    m = np.ones((64, 64), dtype=np.uint8)
    m[0, :] = m[63, :] = m[:, 0] = m[:, 63] = 0
    start = np.array([[[0, 1], [1, 63], [63, 62], [62, 0]]], dtype=np.int32)
    goal = np.array([[[0, 63], [63, 63], [63, 0], [0, 0]]], dtype=np.int32)
    return m, start, goal


def serpentine16():
    """16 x 16, even rows free, odd rows a wall with one gap at alternating ends: ONE path of 134 steps from (0, 0) to (14, 0)."""
    m = np.zeros((16, 16), dtype=np.uint8)
    m[15, :] = 1
    for r in range(1, 15, 2):
        m[r, :] = 1
        m[r, 15 if (r // 2) % 2 == 0 else 0] = 0
    start = np.array([[[0, 1], [0, 0]]], dtype=np.int32)      # agent 0 leads, agent 1 follows it to the cell before the end
    goal = np.array([[[14, 0], [14, 1]]], dtype=np.int32)
    return m, start, goal


def hand_batch():
    cases = list(mr.hand_cases().values())
    return (np.stack([k["map"] for k in cases]), np.stack([k["start"] for k in cases]), np.stack([k["goal"] for k in cases]))


@functools.lru_cache(maxsize=None)
def batch(name):
    """name -> (map, start, goal, order or None, T): the inputs of one batch, made once."""
    if name == "hand":
        return hand_batch() + (None, 24)
    if name == "r10":
        return mr.random_batch(SEED_10x10, 40, 10, 10, 8, 0.2) + (None, 48)
    if name == "r20":
        return mr.random_batch(11, 16, 20, 20, 10, 0.1) + (None, 64)
    if name == "maps_and_order":      # a map per case, non-square, and a priority order per case
        m, s, g = mr.random_batch(23, 8, 12, 9, 5, 0.15, batched_map=True)
        rng = np.random.default_rng(24)
        return m, s, g, np.stack([rng.permutation(5) for _ in range(8)]).astype(np.int32), 40
    if name == "ring64":
        return ring64() + (None, 80)
    if name == "wide5x64":
        return mr.random_batch(31, 3, 5, 64, 4, 0.1) + (None, 96)
    if name == "tall64x5":
        return mr.random_batch(32, 3, 64, 5, 4, 0.1) + (None, 96)
    if name == "w33":
        return mr.random_batch(33, 4, 9, 33, 5, 0.15) + (None, 60)
    if name == "serpentine_T256":      # C = 1, paths longer than 128 steps: the upper half of the LDS layer range
        return serpentine16() + (None, 256)
    if name == "c300":                 # more cases than compute units
        return mr.random_batch(34, 300, 6, 6, 3, 0.25) + (None, 20)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected_plan(name):
    m, s, g, order, T = batch(name)
    return mr.plan_batch(m, s, g, order, T)


@functools.lru_cache(maxsize=None)
def expected_solve(name):
    m, s, g, _, T = batch(name)
    return mr.solve_batch(m, s, g, T, retries=8)


def assert_equal_results(got, want, keys, what):
    for key in keys:
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key], err_msg="%s: %s" % (what, key))


def run_plan(name, device):
    from magat_pathplanning_amd import plan_prioritized
    m, s, g, order, T = batch(name)
    return plan_prioritized(dev(m, device), dev(s, device), dev(g, device), None if order is None else dev(order, device), T)


@pytest.mark.parametrize("name", ["hand", "r10", "r20", "maps_and_order", "ring64", "wide5x64", "tall64x5", "w33",
                                  "serpentine_T256", "c300"])
def test_plan_equals_restatement(gpu_device, name):
    want = expected_plan(name)
    got = run_plan(name, gpu_device)
    assert got["paths"].dtype == torch.int32 and got["solved"].dtype == torch.uint8
    assert tuple(got["paths"].shape) == want["paths"].shape
    assert_equal_results(got, want, PLAN_KEYS, name)
    # what the batch is there for
    if name == "hand":
        assert want["solved"].tolist() == [1, 0, 1, 1, 0] and want["failed_agent"].tolist() == [-1, 1, -1, -1, 1]
    if name == "r10":
        assert 0 < int(want["solved"].sum()) < 40                      # unsolved cases are compared too
    if name == "ring64":
        assert want["solved"].tolist() == [1] and want["lengths"].tolist() == [[63, 63, 63, 63]]
    if name == "serpentine_T256":
        assert want["solved"].tolist() == [1] and want["lengths"].min() - 1 > 128
    if name in ("wide5x64", "tall64x5", "w33", "c300", "r20", "maps_and_order"):
        assert int(want["solved"].sum()) > 0


@pytest.mark.parametrize("name", ["hand", "r10", "r20", "maps_and_order"])
def test_solve_cases_equals_solve_with_retries(gpu_device, name):
    from magat_pathplanning_amd import solve_cases
    m, s, g, _, T = batch(name)
    want = expected_solve(name)
    got = solve_cases(dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device), horizon=T, retries=8)
    assert_equal_results(got, want, PLAN_KEYS + ("order", "rounds"), name)
    done = want["makespan"][want["solved"] != 0]
    assert got["T"] == int(done.max()) + 1
    if name == "r10":
        assert int(got["solved"].sum()) == 40 and int(got["rounds"].max()) > 1
    if name == "hand":                                                 # the closed corridor stays unsolved, the dead end needs one promotion
        assert got["solved"].tolist() == [1, 0, 1, 1, 1] and got["rounds"].tolist() == [1, 9, 1, 1, 2]
    for c in np.nonzero(want["solved"])[0]:
        mc = m if m.ndim == 2 else m[c]
        assert mr.check_schedule(mc, s[c], g[c], got["paths"][c].cpu().numpy(), got["lengths"][c].cpu().numpy()) is None, c


def test_closed_loop_replay_and_samples(gpu_device):
    """The solved 20 x 20 batch: its action keys replayed through BatchedEpisode.step collide nowhere and end at the goals
    with the expert's makespan; expert_samples takes the schedule as **pack."""
    from magat_pathplanning_amd import (BatchedEpisode, expert_samples, expert_schedule, expert_stats, flatten_samples,
                                        solve_cases, solved_pack)
    m, s, g, _, T = batch("r20")
    md = dev(m, gpu_device)
    res = solve_cases(md, dev(s, gpu_device), dev(g, gpu_device), horizon=T)
    assert int(res["solved"].sum()) == len(s)
    pack = solved_pack(res)
    assert sorted(pack) == ["T", "goal", "lengths", "makespan", "paths", "start"] and pack["T"] == res["T"]
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=pack["T"], check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)                   # (C,T,N)
    keys[sched["valid"] == 0] = 4                                       # behind a case's last step: stop
    stats = expert_stats(sched["target"], pack["start"], pack["goal"], sched["valid"])
    ep = BatchedEpisode(md, pack["start"], pack["goal"], maxstep=pack["T"] + 2, comm_radius=7.0)
    ep.currentstep = 1                                                  # the reference counts its steps from 1
    for t in range(pack["T"]):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
    ep.step(actions=torch.full_like(keys[:, 0], 4))                     # everybody has arrived: the episode is closed
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    assert torch.equal(ep.makespan, stats["makespanTarget"])
    samples = expert_samples(md, comm_radius=7, **pack)
    flat = flatten_samples(samples)
    assert flat["inputTensor"].shape[0] == int((pack["makespan"] + 1).sum())
    assert flat["target"].shape[0] == flat["GSO"].shape[0] == flat["inputTensor"].shape[0]


def test_re_solve_from_a_running_episode(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, solve_cases
    m, s, g, _, T = batch("r20")
    ep = BatchedEpisode(dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device), maxstep=100, comm_radius=7.0)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        ep.step(actions=torch.randint(0, 5, (len(s), s.shape[1]), generator=gen, dtype=torch.int32).to(gpu_device))
    now = ep.pos.cpu().numpy()
    assert (now != s).any()
    res = solve_cases(ep.map, ep.pos, ep.goal, horizon=T)
    solved = res["solved"].cpu().numpy()
    assert solved.sum() > 0
    paths, lengths = res["paths"].cpu().numpy(), res["lengths"].cpu().numpy()
    np.testing.assert_array_equal(paths[:, :, 0], now)                  # the schedules start where the agents stand now
    for c in np.nonzero(solved)[0]:
        assert mr.check_schedule(m, now[c], g[c], paths[c], lengths[c]) is None, c


def test_bad_cases_come_back_unsolved_and_harm_nobody(gpu_device):
    from magat_pathplanning_amd import plan_prioritized
    m, s, g, _, T = batch("r10")
    s, g = s[:6].copy(), g[:6].copy()
    order = np.tile(np.arange(8, dtype=np.int32), (6, 1))
    s[1, 3] = np.argwhere(m != 0)[0]                                    # a start on an obstacle
    g[3, 5] = g[3, 2]                                                   # two agents with one goal
    order[4] = [0, 0, 1, 2, 3, 4, 5, 6]                                 # no permutation
    s[5, 2] = [3, 10]                                                   # a start off the map
    want = mr.plan_batch(m, s, g, order, T)
    got = plan_prioritized(dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device), dev(order, gpu_device), T)
    torch.cuda.synchronize()
    assert_equal_results(got, want, PLAN_KEYS, "bad cases")
    assert got["solved"].cpu()[[1, 3, 4, 5]].tolist() == [0, 0, 0, 0]
    assert got["failed_agent"].cpu()[[1, 3, 4, 5]].tolist() == [3, 5, -2, 2]
    # the neighbours are the cases of the clean batch, untouched by the order argument
    clean = expected_plan("r10")
    for c in (0, 2):
        assert_equal_results({k: got[k][c] for k in PLAN_KEYS}, {k: clean[k][c] for k in PLAN_KEYS}, PLAN_KEYS, "case %d" % c)


def test_one_counted_launch_per_call_and_no_host_synchronisation(gpu_device, tag_counts):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import plan_prioritized
    m, s, g, _, T = batch("r10")
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    before = form_count()
    with tag_counts() as tc:
        eager = plan_prioritized(md, sd, gd, horizon=T)
        assert form_count() == before + 1
        plan_prioritized(md, sd, gd, horizon=T)
        assert form_count() == before + 2
    assert tc["sim_mapf"] == 2
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # beyond the limits: refused, nothing launched
        plan_prioritized(torch.zeros(65, 10, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=T)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        plan_prioritized(md, sd, gd, horizon=257)
    assert form_count() == before + 2
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan_prioritized(md, sd, gd, horizon=T)
    torch.cuda.current_stream().wait_stream(side)
    ss = sd.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan_prioritized(md, ss, gd, horizon=T)
    ss.copy_(sd.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    flipped = plan_prioritized(md, sd.flip(0).contiguous(), gd, horizon=T)
    assert_equal_results(out, {k: flipped[k].cpu().numpy() for k in PLAN_KEYS}, PLAN_KEYS, "replay on new starts")
    ss.copy_(sd)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, {k: eager[k].cpu().numpy() for k in PLAN_KEYS}, PLAN_KEYS, "replay")
