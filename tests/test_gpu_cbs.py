"""GPU: conflict-based search (csrc/sim_mapf_cbs.hip through magat_pathplanning_amd/mapf.py cbs_cases) EQUALS its restatement
(tests/cbs_restatement.py, pinned on the CPU by tests/test_host_cbs.py) in every output - paths, lengths, makespan, solved, status,
flowtime, lower_bound, nodes, expanded, horizon_hit - unsolved cases included: hand cases, seeded random batches, every budget,
the edges of the word / lane / LDS layout; the interface around it: inputs untouched, one counted launch, determinism, graph
capture, refusals, the audit and a closed-loop replay of its schedules, solve_cases(optimal=).  The inputs and the
restatement's answers are tests/test_host_cbs.py's, made once per session."""
import numpy as np
import pytest
import torch

import mapf_restatement as mr
import test_host_cbs as hc
from test_gpu_mapf import PLAN_KEYS, assert_equal_results, dev

pytestmark = pytest.mark.gpu
EXTRA = ("status", "flowtime", "lower_bound", "nodes", "expanded", "horizon_hit")


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf_cbs"]))


def given(k, device):
    return dev(k["map"], device), dev(k["start"], device), dev(k["goal"], device)


def run(k, device):
    from magat_pathplanning_amd import cbs_cases
    md, sd, gd = given(k, device)
    kept = [t.clone() for t in (md, sd, gd)]
    before = form_count()
    got = cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
    assert form_count() == before + 1                                    # one counted launch per call
    for t, was in zip((md, sd, gd), kept):                               # the inputs are not modified
        assert torch.equal(t, was)
    assert sorted(got) == sorted(hc.KEYS + ("start", "goal"))
    assert got["paths"].dtype == torch.int32 and got["solved"].dtype == torch.uint8
    assert tuple(got["paths"].shape) == k["want"]["paths"].shape
    for key in EXTRA + ("lengths", "makespan"):
        assert got[key].dtype == torch.int32 and got[key].device == md.device and got[key].is_contiguous(), key
    return got


@pytest.mark.parametrize("name", hc.ALL_NAMES)
def test_cbs_equals_restatement(gpu_device, name):
    hc.check_what_the_case_is_there_for(name)
    k = hc.case(name)
    assert_equal_results(run(k, gpu_device), k["want"], hc.KEYS, name)


def test_more_cases_than_compute_units(gpu_device):
    k = hc.tiled("r8", 300)
    assert_equal_results(run(k, gpu_device), k["want"], hc.KEYS, "r8 tiled to 300 cases")


def test_the_root_cost_is_the_sum_of_the_free_distances(gpu_device):
    """max_nodes = 1: the search stops at the root, whose cost is what the audit calls flowtime_bound."""
    from magat_pathplanning_amd import audit_schedules
    k = hc.case("r8_m1")
    got = run(k, gpu_device)
    audit = audit_schedules(dev(k["map"], gpu_device), got)
    assert bool((got["status"] <= 1).all()) and int((got["status"] == 1).sum()) > 0
    assert torch.equal(got["lower_bound"], audit["flowtime_bound"])
    assert got["nodes"].tolist() == [1] * 24 and got["expanded"].tolist() == [0] * 24


def test_refusals_launch_nothing(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import cbs_cases, solve_cases
    k = hc.case("r8")
    md, sd, gd = given(k, gpu_device)
    before = form_count()
    for wide in (False, True):
        with pytest.raises(nat.MagatNativeError, match="64 x 64"):
            solve_cases(torch.zeros(65, 10, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=40, wide=wide, optimal=16)
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):
        cbs_cases(torch.zeros(10, 65, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=40)
    with pytest.raises(nat.MagatNativeError, match="horizons up to 256"):
        cbs_cases(md, sd, gd, horizon=257)
    with pytest.raises(nat.MagatNativeError, match="nodes"):
        cbs_cases(md, sd, gd, horizon=40, max_nodes=0)
    with pytest.raises(nat.MagatNativeError):
        cbs_cases(md.cpu(), sd.cpu(), gd.cpu())                          # CPU tensors
    # the entry itself: the limits, and a workspace one byte short
    lib = nat.lib()
    C, N = sd.shape[:2]
    need = int(lib.magat_sim_mapf_cbs_workspace_bytes(C, N, 40, 64))
    assert need == hc.documented_bytes(C, N, 40, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    paths = torch.full((C, N, 40, 2), -7, dtype=torch.int32, device=gpu_device)
    lengths = torch.empty(C, N, dtype=torch.int32, device=gpu_device)
    solved = torch.empty(C, dtype=torch.uint8, device=gpu_device)
    extra = torch.empty(7, C, dtype=torch.int32, device=gpu_device)

    def call(H=8, W=8, T=40, ws_bytes=need):
        return lib.magat_sim_mapf_cbs(nat.ptr(md), 1, H, W, nat.ptr(sd), nat.ptr(gd), nat.ptr(paths), nat.ptr(lengths), nat.ptr(extra[0]),
                                      nat.ptr(solved), *[nat.ptr(extra[i]) for i in range(1, 7)], nat.ptr(ws), ws_bytes, C, N, T, 64,
                                      nat.current_stream(sd.device))

    assert call(H=65) == -2 and call(T=257) == -2 and call(ws_bytes=need - 1) == -2
    torch.cuda.synchronize()
    assert form_count() == before and int(paths.max()) == -7             # nothing was launched, nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert form_count() == before + 1
    want = hc.case("r8")["want"]      # (at 64 nodes the cases solved inside 64 nodes come out as at 512)
    early = want["nodes"] <= 64
    np.testing.assert_array_equal(paths.cpu().numpy()[early], want["paths"][early])


def test_determinism_profiling_tag_and_graph_capture(gpu_device, tag_counts):
    from magat_pathplanning_amd import cbs_cases
    k = hc.case("r10")
    md, sd, gd = given(k, gpu_device)
    with tag_counts() as tc:
        first = cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
        second = cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
    assert tc["sim_mapf_cbs"] == 2 and tc["sim_mapf"] == 0 and tc["sim_mapf_audit"] == 0
    for key in hc.KEYS:
        assert torch.equal(first[key], second[key]), key
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, k["want"], hc.KEYS, "replay")
    assert_equal_results(first, k["want"], hc.KEYS, "eager")


@pytest.mark.parametrize("name", ["pocket", "hand", "small", "r8", "r10", "r20", "corner64"])
def test_status_0_schedules_pass_the_audit(gpu_device, name):
    from magat_pathplanning_amd import audit_schedules
    k = hc.case(name)
    got = run(k, gpu_device)
    audit = audit_schedules(dev(k["map"], gpu_device), got)
    done = got["status"] == 0
    assert int(done.sum()) > 0
    assert bool((audit["status"][done] == 0).all()) and bool((audit["status"][~done] == 1).all())
    assert torch.equal(audit["flowtime"][done], got["flowtime"][done]) and torch.equal(audit["makespan"][done], got["makespan"][done])
    known = (got["status"] <= 1) & (audit["flowtime_bound"] >= 0)
    assert bool((got["lower_bound"][known] >= audit["flowtime_bound"][known]).all())      # never weaker than the audit's bound


def test_closed_loop_replay(gpu_device):
    """The 20 x 20 batch, every case proven optimal: its action keys replayed through BatchedEpisode.step collide nowhere and
    end at the goals."""
    from magat_pathplanning_amd import BatchedEpisode, cbs_cases, expert_schedule, solved_pack
    k = hc.case("r20")
    md, sd, gd = given(k, gpu_device)
    res = cbs_cases(md, sd, gd, horizon=k["T"], max_nodes=k["max_nodes"])
    assert int(res["solved"].sum()) == len(k["start"])
    pack = solved_pack(res)
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=pack["T"], check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)                   # (C,T,N)
    keys[sched["valid"] == 0] = 4                                       # behind a case's last step: stop
    ep = BatchedEpisode(md, pack["start"], pack["goal"], maxstep=pack["T"] + 2, comm_radius=7.0)
    ep.currentstep = 1
    for t in range(pack["T"]):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])


def test_solve_cases_with_optimal(gpu_device):
    from magat_pathplanning_amd import audit_schedules, certified, improve_schedules, solve_cases
    # the pocket swap comes back solved
    k = hc.case("pocket")
    md, sd, gd = given(k, gpu_device)
    plain = solve_cases(md, sd, gd, horizon=k["T"])
    got = solve_cases(md, sd, gd, horizon=k["T"], optimal=512)
    assert plain["solved"].tolist() == [0] and got["solved"].tolist() == [1] and got["optimal"].tolist() == [True]
    assert got["failed_agent"].tolist() == [-1] and got["T"] == int(k["want"]["makespan"][0]) + 1
    assert_equal_results(got, k["want"], ("paths", "lengths", "makespan"), "pocket through solve_cases")
    # the 8 x 8 batch
    k = hc.case("r8")
    want = k["want"]
    md, sd, gd = given(k, gpu_device)
    ref = mr.solve_batch(k["map"], k["start"], k["goal"], k["T"], retries=8)
    plain = solve_cases(md, sd, gd, horizon=k["T"])
    # optimal=None: the keys and the bits of the solver as it was
    assert sorted(plain) == sorted(PLAN_KEYS + ("start", "goal", "order", "rounds", "T"))
    assert_equal_results(plain, ref, PLAN_KEYS + ("order", "rounds"), "optimal=None")
    before = form_count()
    got = solve_cases(md, sd, gd, horizon=k["T"], optimal=512, certify=1.0)
    assert form_count() == before + 1
    assert set(got) == set(plain) | {"cbs_status", "cbs_bound", "cbs_nodes", "optimal", "certified"} | (set(hc_audit_keys()) - {"makespan"})
    done = want["status"] == 0
    np.testing.assert_array_equal(got["optimal"].cpu().numpy(), done)
    np.testing.assert_array_equal(got["cbs_status"].cpu().numpy(), want["status"])
    np.testing.assert_array_equal(got["cbs_nodes"].cpu().numpy(), want["nodes"])
    np.testing.assert_array_equal(got["cbs_bound"].cpu().numpy(), np.where(want["horizon_hit"] == 0, want["lower_bound"], -1))
    for key in ("paths", "lengths", "makespan"):      # CBS's where it proved the optimum, the planner's everywhere else
        np.testing.assert_array_equal(got[key].cpu().numpy()[done], want[key][done], err_msg=key)
        np.testing.assert_array_equal(got[key].cpu().numpy()[~done], ref[key][~done], err_msg=key)
    np.testing.assert_array_equal(got["solved"].cpu().numpy(), (ref["solved"] != 0) | done)
    both = torch.from_numpy((ref["solved"] != 0)).to(gpu_device)
    flow_plain, flow_got = (plain["lengths"] - 1).sum(1), (got["lengths"] - 1).sum(1)
    assert bool((flow_got[both] <= flow_plain[both]).all()) and bool((flow_got[both] < flow_plain[both]).any())
    # certified at w = 1: the cases proven optimal, and those the audit certifies alone
    alone = certified(audit_schedules(md, plain), 1.0)
    assert torch.equal(got["certified"], got["optimal"] | alone)
    assert int(got["certified"].sum()) > int(alone.sum())
    audit = audit_schedules(md, got)
    assert torch.equal(got["flowtime_bound"], torch.maximum(audit["flowtime_bound"], got["cbs_bound"]))
    assert bool((got["flowtime"][got["status"] == 0] >= got["flowtime_bound"][got["status"] == 0]).all())
    # the result is a result: the improver and the audit take it
    better = improve_schedules(md, got, iterations=4)
    assert bool((better["flowtime_after"][got["optimal"]] == better["flowtime_before"][got["optimal"]]).all())


def hc_audit_keys():
    from magat_pathplanning_amd import mapf
    return mapf.AUDIT_KEYS
