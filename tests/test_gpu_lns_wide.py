"""GPU: the wide form of the schedule improver (csrc/sim_mapf_lns_wide.hip through improve_schedules(..., wide=True)) EQUALS the
restatement (tests/lns_restatement.py; its answers to these inputs are pinned on the CPU by tests/test_host_lns_wide.py, where
the inputs live) - paths, lengths, makespan, both flowtimes, accepted and status, integer equality everywhere - at the word and
wave boundaries, with paths longer than 256 cells, at T = 1024, in batches up to 256 x 256, with more agents than threads and
on skipped and refused inputs; and the interface around it: inputs untouched, the 64 form inside the old limits,
solve_cases(wide=True, improve=), replay through BatchedEpisode, expert_samples, graph capture, counts and limits."""
import numpy as np
import pytest
import torch

import mapf_restatement as mr
from test_host_lns_wide import ALL_NAMES, KEYS, RES_KEYS, case, check_what_the_case_is_there_for

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf_lns"]))


def assert_equal_results(got, want, keys, what):
    for key in keys:
        assert tuple(got[key].shape) == np.asarray(want[key]).shape, (what, key)
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key], err_msg="%s: %s" % (what, key))


def given_on(name, device):
    m, s, g, res, it, k, want = case(name)
    given = {key: dev(res[key], device) for key in RES_KEYS}
    given.update(start=dev(s, device), goal=dev(g, device))
    return dev(m, device), given, it, k, want


@pytest.mark.parametrize("name", ALL_NAMES)
def test_wide_improve_equals_restatement(gpu_device, name):
    from magat_pathplanning_amd import improve_schedules
    check_what_the_case_is_there_for(name)
    md, given, it, k, want = given_on(name, gpu_device)
    kept = {key: value.clone() for key, value in given.items()}
    before = form_count()
    got = improve_schedules(md, given, iterations=it, neighbourhood=k, wide=True)
    assert form_count() == before + 1
    for key in kept:                                                    # the input tensors are not modified
        assert torch.equal(given[key], kept[key]), key
    assert got["paths"].data_ptr() != given["paths"].data_ptr() and got["solved"] is given["solved"] and got["goal"] is given["goal"]
    for key in KEYS:
        assert got[key].dtype == torch.int32, key
    assert_equal_results(got, want, KEYS, name)


def narrow_names():
    import test_gpu_lns as tg
    return ["10x10", "12x12", "edges", "hand_k1", "hand_k8_no_iterations", "hand_k8", "start_is_goal"] + tg.NEWCOMER_NAMES


@pytest.mark.parametrize("name", narrow_names())
def test_wide_entry_on_the_narrow_inputs(gpu_device, name):
    """improve_schedules(..., wide=True) sends a shape inside 64 x 64 to the 64 form, so the wide kernel is reached here through its
    entry, with a workspace of exactly the size it asks for: every output equals the 64 form's and the restatement's."""
    import test_gpu_lns as tg
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import improve_schedules
    m, res, it, k, want = tg.case(name)
    md = dev(np.asarray(m, dtype=np.uint8), gpu_device)
    given = {key: dev(res[key], gpu_device) for key in RES_KEYS}
    narrow = improve_schedules(md, given, iterations=it, neighbourhood=k)
    solved = given["solved"].to(torch.uint8).contiguous()
    C, N, T, _ = given["paths"].shape
    H, W = md.shape[-2:]
    lib = nat.lib()
    out = {key: given[key].to(torch.int32).clone() for key in ("paths", "lengths", "makespan")}
    out.update({key: torch.full((C,), -7, dtype=torch.int32, device=gpu_device) for key in KEYS[3:]})
    ws = torch.empty(lib.magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T), dtype=torch.uint8, device=gpu_device)
    with torch.cuda.device(gpu_device):
        rc = lib.magat_sim_mapf_improve_wide(nat.ptr(md), int(md.dim() == 3), H, W, nat.ptr(solved), nat.ptr(out["paths"]),
                                             nat.ptr(out["lengths"]), nat.ptr(out["makespan"]), nat.ptr(out["flowtime_before"]),
                                             nat.ptr(out["flowtime_after"]), nat.ptr(out["accepted"]), nat.ptr(out["status"]), nat.ptr(ws),
                                             ws.numel(), C, N, T, it, k, nat.current_stream(gpu_device))
    nat.check(rc, "magat_sim_mapf_improve_wide")
    for key in KEYS:
        assert torch.equal(out[key], narrow[key]), (name, key)
    assert_equal_results(out, want, KEYS, name)


def test_inside_the_old_limits_wide_gives_the_bits_of_the_64_form(gpu_device, tag_counts):
    from magat_pathplanning_amd import improve_schedules, solve_cases
    m, s, g = mr.random_batch(11, 16, 20, 20, 10, 0.1)
    md = dev(m, gpu_device)
    res = solve_cases(md, dev(s, gpu_device), dev(g, gpu_device), horizon=64)
    narrow = improve_schedules(md, res, iterations=16, neighbourhood=4)
    before = form_count()
    with tag_counts() as tc:
        wide = improve_schedules(md, res, iterations=16, neighbourhood=4, wide=True)
    assert form_count() == before + 1 and tc["sim_mapf_lns"] == 1 and tc["sim_mapf"] == 0      # one launch of the 64 form's kernel
    assert sorted(wide) == sorted(narrow)
    for key in narrow:
        assert torch.equal(wide[key], narrow[key]), key
    assert int(narrow["accepted"].sum()) > 0


def test_wide_solve_cases_with_improve_is_solve_cases_then_improve_schedules(gpu_device):
    from magat_pathplanning_amd import improve_schedules, solve_cases
    m, s, g, res, it, k, want = case("clusters65")
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    plain = solve_cases(md, sd, gd, horizon=40, wide=True)
    assert_equal_results(plain, res, RES_KEYS, "solve_cases(wide=True)")
    assert "flowtime_after" not in plain
    before = form_count()
    both = solve_cases(md, sd, gd, horizon=40, wide=True, improve=12)
    assert form_count() == before + 1
    after = improve_schedules(md, plain, iterations=12, wide=True)
    assert sorted(both) == sorted(list(after) + ["T"]) and "T" not in after
    for key in after:
        assert torch.equal(both[key], after[key]), key
    assert_equal_results(both, want, KEYS, "solve_cases(wide=True, improve=12)")      # (the default neighbourhood is this batch's k = 4)
    assert both["T"] == int(both["makespan"].max()) + 1


def test_improved_wide_batch_replays_and_feeds_expert_samples(gpu_device):
    """The improved 65 x 65 cluster batch: its action keys replayed through BatchedEpisode(..., wide=True).step collide nowhere
    and end at the goals with the improved makespan; expert_samples(..., wide=True) takes it as **pack."""
    from magat_pathplanning_amd import (BatchedEpisode, expert_samples, expert_schedule, flatten_samples, improve_schedules,
                                        solved_pack)
    md, given, it, k, want = given_on("clusters65", gpu_device)
    got = improve_schedules(md, given, iterations=it, neighbourhood=k, wide=True)
    assert_equal_results(got, want, KEYS, "clusters65")
    pack = solved_pack(got)
    assert sorted(pack) == ["T", "goal", "lengths", "makespan", "paths", "start"] and pack["paths"].shape[0] == 8
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=pack["T"], check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)
    keys[sched["valid"] == 0] = 4
    ep = BatchedEpisode(md, pack["start"], pack["goal"], maxstep=pack["T"] + 2, comm_radius=7.0, wide=True)
    ep.currentstep = 1
    prev, last_move = pack["start"].clone(), torch.zeros(8, dtype=torch.int32, device=gpu_device)
    for t in range(pack["T"]):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
        assert torch.equal(ep.pos, pack["paths"][:, :, min(t + 1, pack["paths"].shape[2] - 1)]), t      # the improved schedule, cell for cell
        last_move[(ep.pos != prev).flatten(1).any(1)] = t + 1
        prev = ep.pos.clone()
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    np.testing.assert_array_equal(last_move.cpu().numpy(), want["makespan"])      # the last move of the replay: the improved makespan
    flat = flatten_samples(expert_samples(md, comm_radius=7, wide=True, **pack))
    assert flat["inputTensor"].shape[0] == int((pack["makespan"] + 1).sum())


def test_wide_improve_graph_capture_counts_and_limits(gpu_device, tag_counts):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import improve_schedules
    md, given, it, k, want = given_on("clusters65", gpu_device)
    before = form_count()
    with tag_counts() as tc:
        eager = improve_schedules(md, given, iterations=it, neighbourhood=k, wide=True)
    assert form_count() == before + 1 and tc["sim_mapf_lns"] == 1 and tc["sim_mapf"] == 0
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        improve_schedules(md, given, iterations=it, neighbourhood=k, wide=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = improve_schedules(md, given, iterations=it, neighbourhood=k, wide=True)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, want, KEYS, "replay")
    assert_equal_results(eager, want, KEYS, "eager")
    # refused calls: nothing launched, nothing counted
    count = form_count()
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):          # without the keyword 65 x 65 is refused as before
        improve_schedules(md, given, iterations=it, neighbourhood=k)
    small = dict(paths=torch.zeros(1, 2, 16, 2, dtype=torch.int32, device=gpu_device),
                 lengths=torch.ones(1, 2, dtype=torch.int32, device=gpu_device),
                 makespan=torch.zeros(1, dtype=torch.int32, device=gpu_device),
                 solved=torch.ones(1, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(nat.MagatNativeError, match="horizons up to 256"):
        improve_schedules(torch.zeros(20, 20, dtype=torch.uint8, device=gpu_device),
                          dict(small, paths=torch.zeros(1, 2, 257, 2, dtype=torch.int32, device=gpu_device)))
    with pytest.raises(nat.MagatNativeError):                           # beyond the wide limits
        improve_schedules(torch.zeros(257, 10, dtype=torch.uint8, device=gpu_device), small, wide=True)
    with pytest.raises(nat.MagatNativeError):
        improve_schedules(md, dict(small, paths=torch.zeros(1, 2, 1025, 2, dtype=torch.int32, device=gpu_device)), wide=True)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        improve_schedules(md, given, neighbourhood=9, wide=True)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        improve_schedules(md, given, iterations=4097, wide=True)
    assert form_count() == count
