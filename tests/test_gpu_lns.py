"""GPU: the schedule improver (csrc/sim_mapf_lns.hip through magat_pathplanning_amd/mapf.py improve_schedules) EQUALS its
restatement (tests/lns_restatement.py, pinned on the CPU by tests/test_host_lns.py) - paths, lengths, makespan, both flowtimes,
accepted and status - on the random batches, the hand case, the edge cases and the edges of the word / lane / LDS layout; the
interface around it: inputs untouched, solve_cases(improve=), replay through BatchedEpisode, graph capture, limits."""
import functools

import numpy as np
import pytest
import torch

import lns_restatement as lr
import mapf_restatement as mr
from test_gpu_mapf import assert_equal_results, batch, dev, expected_solve, serpentine16

pytestmark = pytest.mark.gpu
KEYS = ("paths", "lengths", "makespan", "flowtime_before", "flowtime_after", "accepted", "status")
RES_KEYS = ("paths", "lengths", "makespan", "solved")


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf_lns"]))


def corner64():
    """64 x 64, a ring two cells thick: agent 0 comes down column 62 and turns into row 63, agent 1 starts in the corner
    (63, 63) - lane 63, bit 63 - two steps from its goal and, planned second, is held up by agent 0; the improver lets it go
    first (lengths 6, 6 -> 6, 3)."""
    m = np.ones((64, 64), dtype=np.uint8)
    m[0:2, :] = m[62:64, :] = 0
    m[:, 0:2] = m[:, 62:64] = 0
    return m, np.array([[[60, 62], [63, 63]]], dtype=np.int32), np.array([[[63, 60], [63, 61]]], dtype=np.int32)


def crowd70(seeds=(41, 44)):
    """20 x 20 maps of their own with 70 agents - more agents than lanes - each going to a cell at most 4 steps away."""
    maps, starts, goals = [], [], []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        m = (rng.random((20, 20)) < 0.05).astype(np.uint8)
        cells = mr.largest_component(m == 0)
        start = cells[rng.permutation(len(cells))[:70]]
        taken, goal = set(), []
        for a in range(70):
            near = [tuple(c) for c in cells if abs(c[0] - start[a][0]) + abs(c[1] - start[a][1]) <= 4
                    and tuple(c) not in taken and tuple(c) != tuple(start[a])]
            goal.append(near[rng.integers(len(near))])
            taken.add(goal[-1])
        maps.append(m), starts.append(start), goals.append(goal)
    return np.stack(maps), np.asarray(starts, dtype=np.int32), np.asarray(goals, dtype=np.int32)


def _stack_res(outs):
    return {key: np.stack([np.asarray(o[key]) for o in outs]).astype(np.uint8 if key == "solved" else np.int32) for key in RES_KEYS}


def edge_inputs():
    """One (C,2,3) batch of 2-agent cases with T = 8: the hand case, unsolved (solved = 0), and refused inputs - an off-map
    cell, a length of 0, a length of T + 1, a diagonal step, a cell on an obstacle (a map per case)."""
    h = lr.hand_case()
    first = mr.plan(h["map"], h["start"], h["goal"], None, h["T"])
    maps, outs = [], []
    for what in ("hand", "unsolved", "off_map", "length_0", "length_T+1", "diagonal", "obstacle"):
        o = {key: np.array(first[key]) for key in RES_KEYS}
        m = h["map"].copy()
        if what == "unsolved":
            o["solved"] = np.array(0)
        elif what == "off_map":
            o["paths"][1, 5] = (0, 3)
        elif what == "length_0":
            o["lengths"][0] = 0
        elif what == "length_T+1":
            o["lengths"][1] = h["T"] + 1
        elif what == "diagonal":
            o["paths"][0, 1] = (1, 0)
            o["paths"][0, 2:] = (0, 1)
        elif what == "obstacle":
            m[0, 1] = 1
        maps.append(m), outs.append(o)
    return np.stack(maps), _stack_res(outs)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (map, the schedules going in (a solve_batch / plan_batch dict), iterations, k, the restatement's result)."""
    if name in lr.BATCHES:
        m, _, _, res, want = lr.solved_and_improved(name)
        return m, res, lr.BATCHES[name]["iterations"], lr.BATCHES[name]["k"], want
    it, k = 4, 3
    if name.startswith("newcomers_"):           # two newcomers in one step of the seed's free path (lr.newcomer_case), 8 x 20
        c, _, _, _, k = lr.newcomer_named(name, 8)
        m, res, it = c["map"], c["res"], 1
    elif name == "edges":
        m, res = edge_inputs()
        it, k = 2, 2
    elif name == "hand_k1":
        m, res = edge_inputs()
        it, k = 4, 1
    elif name == "hand_k8_no_iterations":
        m, res = edge_inputs()
        it, k = 0, 8
    elif name == "hand_k8":                     # k > N
        m, res = edge_inputs()
        it, k = 3, 8
    elif name == "start_is_goal":
        h = mr.hand_cases()["start_is_goal"]
        m, res = h["map"], mr.plan_batch(h["map"], h["start"][None], h["goal"][None], None, h["T"])
    elif name == "corner64":
        m, s, g = corner64()
        res, it, k = mr.plan_batch(m, s, g, None, 16), 2, 2
    elif name == "w33":
        m, s, g = mr.random_batch(33, 4, 9, 33, 5, 0.15)
        res = mr.solve_batch(m, s, g, 60, retries=8)
    elif name == "crowd70":
        m, s, g = crowd70()
        res, it, k = mr.solve_batch(m, s, g, 40, retries=8), 8, 4
    elif name == "serpentine_T256":             # C = 1, the whole LDS layer range
        m, s, g = serpentine16()
        res, it, k = mr.plan_batch(m, s, g, None, 256), 2, 2
    elif name == "c300":                        # more cases than compute units; the unsolved ones are skipped
        m, s, g = mr.random_batch(34, 300, 6, 6, 3, 0.25)
        res, it, k = mr.plan_batch(m, s, g, None, 20), 3, 2
    elif name == "map_per_case":
        m, s, g = mr.random_batch(23, 8, 12, 9, 5, 0.15, batched_map=True)
        res, it, k = mr.solve_batch(m, s, g, 40, retries=8), 6, 3
    else:
        raise KeyError(name)
    return m, res, it, k, lr.improve_batch(m, res, it, k)


def run(name, device):
    from magat_pathplanning_amd import improve_schedules
    m, res, it, k, want = case(name)
    given = {key: dev(res[key], device) for key in RES_KEYS}
    kept = {key: value.clone() for key, value in given.items()}
    got = improve_schedules(dev(m, device), given, iterations=it, neighbourhood=k)
    for key in RES_KEYS:                                                # the input tensors are not modified
        assert torch.equal(given[key], kept[key]), key
    assert got["paths"].data_ptr() != given["paths"].data_ptr() and got["solved"] is given["solved"]
    return got, want


NEWCOMER_NAMES = lr.newcomer_names(("one_wave", "two_chunks64"))


@pytest.mark.parametrize("name", ["10x10", "12x12", "edges", "hand_k1", "hand_k8_no_iterations", "hand_k8", "start_is_goal",
                                  "corner64", "w33", "crowd70", "serpentine_T256", "c300", "map_per_case"] + NEWCOMER_NAMES)
def test_improve_equals_restatement(gpu_device, name):
    got, want = run(name, gpu_device)
    for key in KEYS:
        assert got[key].dtype == torch.int32, key
    assert_equal_results(got, want, KEYS, name)
    # what the case is there for
    if name in lr.BATCHES:
        assert int(want["flowtime_after"].sum()) < int(want["flowtime_before"].sum())
    if name == "edges":
        assert want["status"].tolist() == [0, 1, 2, 2, 2, 2, 2] and want["accepted"].tolist() == [1, 0, 0, 0, 0, 0, 0]
        assert want["lengths"][0].tolist() == [3, 3]
    if name == "hand_k1" or name == "hand_k8_no_iterations":
        assert want["accepted"][0] == 0
    if name == "hand_k8":
        assert want["accepted"][0] == 1
    if name == "corner64":
        assert want["lengths"].tolist() == [[6, 3]] and want["flowtime_before"].tolist() == [10]
    if name == "crowd70":
        assert want["paths"].shape[1] == 70 and int(want["accepted"].min()) >= 1
    if name == "serpentine_T256":
        assert want["paths"].shape[2] == 256 and want["lengths"].min() - 1 > 128 and want["status"].tolist() == [0]
    if name == "c300":
        assert 0 < int((want["status"] == 1).sum()) < 300 and int(want["accepted"].sum()) >= 1
    if name in ("w33", "map_per_case"):
        assert int(want["accepted"].sum()) >= 1
    if name in NEWCOMER_NAMES:
        import test_host_lns as th
        th.check_newcomers(name, 8, want)


def test_solve_cases_with_improve_is_solve_cases_then_improve_schedules(gpu_device):
    from magat_pathplanning_amd import improve_schedules, solve_cases
    m, s, g, _, T = batch("r20")
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    plain = solve_cases(md, sd, gd, horizon=T)
    assert_equal_results(plain, expected_solve("r20"), ("paths", "lengths", "makespan", "solved", "failed_agent", "order", "rounds"),
                         "solve_cases without the keyword")
    assert "flowtime_after" not in plain
    before = form_count()
    both = solve_cases(md, sd, gd, horizon=T, improve=16)
    assert form_count() == before + 1
    after = improve_schedules(md, plain, iterations=16)
    assert sorted(both) == sorted(list(after) + ["T"]) and "T" not in after
    for key in after:
        assert torch.equal(both[key], after[key]), key
    assert both["T"] == int(both["makespan"].max()) + 1
    assert int(both["flowtime_after"].sum()) <= int(both["flowtime_before"].sum())
    for c in range(len(s)):
        assert mr.check_schedule(m, s[c], g[c], both["paths"][c].cpu().numpy(), both["lengths"][c].cpu().numpy()) is None, c


def test_improved_batch_replays_and_feeds_expert_samples(gpu_device):
    """The improved 10 x 10 batch: its action keys replayed through BatchedEpisode.step collide nowhere and end at the goals
    with the improved makespan; expert_samples takes it as **pack."""
    from magat_pathplanning_amd import (BatchedEpisode, expert_samples, expert_schedule, expert_stats, flatten_samples,
                                        improve_schedules, solved_pack)
    m, s, g, res, want = lr.solved_and_improved("10x10")
    md = dev(m, gpu_device)
    given = {key: dev(res[key], gpu_device) for key in RES_KEYS}
    given.update(start=dev(s, gpu_device), goal=dev(g, gpu_device))
    got = improve_schedules(md, given, iterations=lr.BATCHES["10x10"]["iterations"], neighbourhood=lr.BATCHES["10x10"]["k"])
    assert int(got["makespan"].sum()) == int(want["makespan"].sum())
    pack = solved_pack(got)
    assert sorted(pack) == ["T", "goal", "lengths", "makespan", "paths", "start"]
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=pack["T"], check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)
    keys[sched["valid"] == 0] = 4
    stats = expert_stats(sched["target"], pack["start"], pack["goal"], sched["valid"])
    ep = BatchedEpisode(md, pack["start"], pack["goal"], maxstep=pack["T"] + 2, comm_radius=7.0)
    ep.currentstep = 1
    prev, last_move = pack["start"].clone(), torch.zeros(len(s), dtype=torch.int32, device=gpu_device)
    for t in range(pack["T"]):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
        assert torch.equal(ep.pos, pack["paths"][:, :, min(t + 1, pack["paths"].shape[2] - 1)]), t      # the improved schedule, cell for cell
        last_move[(ep.pos != prev).flatten(1).any(1)] = t + 1
        prev = ep.pos.clone()
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    # (ep.makespan counts as the reference does, from the first move of a case: one more where an agent never moves)
    assert torch.equal(ep.makespan, stats["makespanTarget"])
    np.testing.assert_array_equal(last_move.cpu().numpy(), want["makespan"])      # the last move of the replay: the improved makespan
    flat = flatten_samples(expert_samples(md, comm_radius=7, **pack))
    assert flat["inputTensor"].shape[0] == int((pack["makespan"] + 1).sum())


def test_one_counted_launch_graph_capture_and_limits(gpu_device, tag_counts):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import improve_schedules
    m, res, it, k, want = case("10x10")
    md = dev(m, gpu_device)
    given = {key: dev(res[key], gpu_device) for key in RES_KEYS}
    before = form_count()
    with tag_counts() as tc:
        eager = improve_schedules(md, given, iterations=it, neighbourhood=k)
    assert form_count() == before + 1 and form_count() >= 1 and tc["sim_mapf_lns"] == 1 and tc["sim_mapf"] == 0
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        improve_schedules(md, given, iterations=it, neighbourhood=k)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = improve_schedules(md, given, iterations=it, neighbourhood=k)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, want, KEYS, "replay")
    assert_equal_results(eager, want, KEYS, "eager")
    # beyond the limits: refused, nothing launched
    count = form_count()
    big = dict(paths=torch.zeros(1, 2, 16, 2, dtype=torch.int32, device=gpu_device),
               lengths=torch.ones(1, 2, dtype=torch.int32, device=gpu_device),
               makespan=torch.zeros(1, dtype=torch.int32, device=gpu_device),
               solved=torch.ones(1, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):
        improve_schedules(torch.zeros(65, 65, dtype=torch.uint8, device=gpu_device), big)
    long = dict(big, paths=torch.zeros(1, 2, 257, 2, dtype=torch.int32, device=gpu_device))
    with pytest.raises(nat.MagatNativeError, match="horizons up to 256"):
        improve_schedules(md, long)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        improve_schedules(md, given, neighbourhood=9)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        improve_schedules(md, given, iterations=4097)
    assert form_count() == count
