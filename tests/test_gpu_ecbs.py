"""GPU: bounded-suboptimal conflict-based search (csrc/sim_mapf_ecbs.hip through magat_pathplanning_amd/mapf.py ecbs_cases)
EQUALS its restatement (tests/ecbs_restatement.py, pinned on the CPU by tests/test_host_ecbs.py) in every output - paths, lengths,
makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit - unsolved cases included: hand cases, seeded
random batches at several (w, levels, budget), the edges of the word / lane layout, T = 256; the interface around it: inputs
untouched, one counted launch, determinism, graph capture, refusals, the audit and a closed-loop replay of its schedules,
solve_cases(bounded=).  The inputs and the restatement's answers are tests/test_host_ecbs.py's, made once per session."""
import numpy as np
import pytest
import torch

import mapf_restatement as mr
import test_host_ecbs as he
from test_gpu_mapf import PLAN_KEYS, assert_equal_results, dev

pytestmark = pytest.mark.gpu
EXTRA = ("status", "flowtime", "lower_bound", "nodes", "expanded", "horizon_hit")


def form_count(form="sim_mapf_ecbs"):
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS[form]))


def given(k, device):
    return dev(k["map"], device), dev(k["start"], device), dev(k["goal"], device)


def call(k, md, sd, gd):
    from magat_pathplanning_amd import ecbs_cases
    return ecbs_cases(md, sd, gd, w=k["w_milli"] / 1000.0, horizon=k["T"], max_nodes=k["max_nodes"], levels=k["levels"])


def run(k, device):
    md, sd, gd = given(k, device)
    kept = [t.clone() for t in (md, sd, gd)]
    before, cbs_before = form_count(), form_count("sim_mapf_cbs")
    got = call(k, md, sd, gd)
    assert form_count() == before + 1 and form_count("sim_mapf_cbs") == cbs_before      # one counted launch per call
    for t, was in zip((md, sd, gd), kept):                               # the inputs are not modified
        assert torch.equal(t, was)
    assert sorted(got) == sorted(he.KEYS + ("start", "goal"))
    assert got["paths"].dtype == torch.int32 and got["solved"].dtype == torch.uint8
    assert tuple(got["paths"].shape) == k["want"]["paths"].shape
    for key in EXTRA + ("lengths", "makespan"):
        assert got[key].dtype == torch.int32 and got[key].device == md.device and got[key].is_contiguous(), key
    return got


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", he.GPU_INPUTS)
def test_ecbs_equals_restatement(gpu_device, name, w_milli, levels, max_nodes):
    k = he.case(name, w_milli, levels, max_nodes)
    assert_equal_results(run(k, gpu_device), k["want"], he.KEYS, "%s at %r" % (name, (w_milli, levels, max_nodes)))


def test_more_cases_than_compute_units(gpu_device):
    k = he.tiled(he.case("r8", 1500, 4, 64), 300)
    assert_equal_results(run(k, gpu_device), k["want"], he.KEYS, "r8 tiled to 300 cases")


def test_refusals_launch_nothing(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import ecbs_cases, solve_cases
    k = he.case("r8", 1500, 4, 64)
    md, sd, gd = given(k, gpu_device)
    before, plans = form_count(), form_count("sim_mapf")
    for wide in (False, True):
        with pytest.raises(nat.MagatNativeError, match="64 x 64"):
            solve_cases(torch.zeros(65, 10, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=40, wide=wide, bounded=1.5)
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):
        ecbs_cases(torch.zeros(10, 65, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=40)
    with pytest.raises(nat.MagatNativeError, match="horizons up to 256"):
        ecbs_cases(md, sd, gd, horizon=257)
    with pytest.raises(nat.MagatNativeError, match="nodes"):
        ecbs_cases(md, sd, gd, horizon=40, max_nodes=0)
    with pytest.raises(nat.MagatNativeError, match="levels"):
        ecbs_cases(md, sd, gd, horizon=40, levels=5)
    with pytest.raises(ValueError):
        ecbs_cases(md, sd, gd, w=0.5, horizon=40)
    with pytest.raises(ValueError):
        solve_cases(md, sd, gd, horizon=40, optimal=16, bounded=1.5)
    with pytest.raises(nat.MagatNativeError):
        ecbs_cases(md.cpu(), sd.cpu(), gd.cpu())                          # CPU tensors
    assert form_count("sim_mapf") == plans                                # refused before anything was planned
    # the entry itself: the limits, and a workspace one byte short
    lib = nat.lib()
    C, N = sd.shape[:2]
    need = int(lib.magat_sim_mapf_ecbs_workspace_bytes(C, N, 40, 64, 4))
    assert need == he.documented_bytes(C, N, 40, 64, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    paths = torch.full((C, N, 40, 2), -7, dtype=torch.int32, device=gpu_device)
    lengths = torch.empty(C, N, dtype=torch.int32, device=gpu_device)
    solved = torch.empty(C, dtype=torch.uint8, device=gpu_device)
    extra = torch.empty(7, C, dtype=torch.int32, device=gpu_device)

    def entry(H=8, W=8, T=40, ws_bytes=need, w=1500, K=4):
        return lib.magat_sim_mapf_ecbs(nat.ptr(md), 1, H, W, nat.ptr(sd), nat.ptr(gd), nat.ptr(paths), nat.ptr(lengths), nat.ptr(extra[0]),
                                       nat.ptr(solved), *[nat.ptr(extra[i]) for i in range(1, 7)], nat.ptr(ws), ws_bytes, C, N, T, 64,
                                       w, K, nat.current_stream(sd.device))

    assert entry(H=65) == -2 and entry(T=257) == -2 and entry(ws_bytes=need - 1) == -2 and entry(K=5) == -2 and entry(K=0) == -1
    assert entry(w=999) == -1 and entry(w=(1 << 20) + 1) == -2
    torch.cuda.synchronize()
    assert form_count() == before and int(paths.max()) == -7             # nothing was launched, nothing was written
    assert entry() == 0
    torch.cuda.synchronize()
    assert form_count() == before + 1
    np.testing.assert_array_equal(paths.cpu().numpy(), k["want"]["paths"])


def test_determinism_profiling_tag_and_graph_capture(gpu_device, tag_counts):
    k = he.case("r10", 1500, 4, 64)
    md, sd, gd = given(k, gpu_device)
    with tag_counts() as tc:
        first = call(k, md, sd, gd)
        second = call(k, md, sd, gd)
    assert tc["sim_mapf_ecbs"] == 2 and tc["sim_mapf_cbs"] == 0 and tc["sim_mapf"] == 0 and tc["sim_mapf_audit"] == 0
    for key in he.KEYS:
        assert torch.equal(first[key], second[key]), key
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call(k, md, sd, gd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(k, md, sd, gd)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, k["want"], he.KEYS, "replay")
    assert_equal_results(first, k["want"], he.KEYS, "eager")


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", [g for g in he.GPU_INPUTS if g[0] in ("pocket", "hand", "small", "r8", "r10", "r20", "corner64")])
def test_status_0_schedules_pass_the_audit(gpu_device, name, w_milli, levels, max_nodes):
    from magat_pathplanning_amd import audit_schedules
    k = he.case(name, w_milli, levels, max_nodes)
    md, sd, gd = given(k, gpu_device)
    got = call(k, md, sd, gd)
    audit = audit_schedules(md, got)
    done = got["status"] == 0
    assert int(done.sum()) > 0
    assert bool((audit["status"][done] == 0).all()) and bool((audit["status"][~done] == 1).all())
    assert torch.equal(audit["flowtime"][done], got["flowtime"][done]) and torch.equal(audit["makespan"][done], got["makespan"][done])
    assert bool((1000 * got["flowtime"][done].to(torch.int64) <= w_milli * got["lower_bound"][done].to(torch.int64)).all())
    known = (got["status"] <= 1) & (audit["flowtime_bound"] >= 0)
    assert bool((got["lower_bound"][known] >= audit["flowtime_bound"][known]).all())      # never weaker than the audit's bound


def test_closed_loop_replay(gpu_device):
    """The 20 x 20 batch, every case solved within 1.2 of its bound: its action keys replayed through BatchedEpisode.step collide
    nowhere and end at the goals."""
    from magat_pathplanning_amd import BatchedEpisode, expert_schedule, solved_pack
    k = he.case("r20", 1200, 4, 64)
    md, sd, gd = given(k, gpu_device)
    res = call(k, md, sd, gd)
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


def test_solve_cases_with_bounded(gpu_device):
    from magat_pathplanning_amd import audit_schedules, certified, improve_schedules, mapf, solve_cases
    # the pocket swap comes back solved
    k = he.case("pocket", 1500, 4, 64)
    md, sd, gd = given(k, gpu_device)
    plain = solve_cases(md, sd, gd, horizon=k["T"])
    got = solve_cases(md, sd, gd, horizon=k["T"], bounded=1.5, bounded_nodes=64)
    assert plain["solved"].tolist() == [0] and got["solved"].tolist() == [1] and got["bounded"].tolist() == [True]
    assert got["failed_agent"].tolist() == [-1] and got["T"] == int(k["want"]["makespan"][0]) + 1
    assert_equal_results(got, k["want"], ("paths", "lengths", "makespan"), "pocket through solve_cases")
    # the 8 x 8 batch
    k = he.case("r8", 1500, 4, 64)
    want = k["want"]
    md, sd, gd = given(k, gpu_device)
    ref = mr.solve_batch(k["map"], k["start"], k["goal"], k["T"], retries=8)
    plain = solve_cases(md, sd, gd, horizon=k["T"])
    # bounded=None: the keys and the bits of the solver as it was
    assert sorted(plain) == sorted(PLAN_KEYS + ("start", "goal", "order", "rounds", "T"))
    assert_equal_results(plain, ref, PLAN_KEYS + ("order", "rounds"), "bounded=None")
    before, cbs_before = form_count(), form_count("sim_mapf_cbs")
    got = solve_cases(md, sd, gd, horizon=k["T"], bounded=1.5, bounded_nodes=64, certify=1.5)
    assert form_count() == before + 1 and form_count("sim_mapf_cbs") == cbs_before
    assert set(got) == set(plain) | {"ecbs_status", "ecbs_bound", "ecbs_nodes", "bounded", "certified"} | (set(mapf.AUDIT_KEYS) - {"makespan"})
    done = want["status"] == 0
    np.testing.assert_array_equal(got["bounded"].cpu().numpy(), done)
    np.testing.assert_array_equal(got["ecbs_status"].cpu().numpy(), want["status"])
    np.testing.assert_array_equal(got["ecbs_nodes"].cpu().numpy(), want["nodes"])
    np.testing.assert_array_equal(got["ecbs_bound"].cpu().numpy(), np.where(want["horizon_hit"] == 0, want["lower_bound"], -1))
    # the replacement rule: a status-0 case replaces the plan only where the plan is unsolved or has a larger flowtime
    flow_ref = (ref["lengths"].astype(np.int64) - 1).sum(1)
    take = done & ((ref["solved"] == 0) | (flow_ref > want["flowtime"]))
    assert take.any()
    for key in ("paths", "lengths", "makespan"):
        np.testing.assert_array_equal(got[key].cpu().numpy()[take], want[key][take], err_msg=key)
        np.testing.assert_array_equal(got[key].cpu().numpy()[~take], ref[key][~take], err_msg=key)
    np.testing.assert_array_equal(got["solved"].cpu().numpy(), (ref["solved"] != 0) | take)
    np.testing.assert_array_equal(got["failed_agent"].cpu().numpy(), np.where(take, -1, ref["failed_agent"]))
    flow_got = (got["lengths"] - 1).sum(1).cpu().numpy()
    solved = got["solved"].cpu().numpy() != 0
    assert (flow_got[solved] <= np.where(ref["solved"] != 0, flow_ref, 1 << 30)[solved]).all()
    # certified at w = 1.5: every case the search bounded, since flowtime <= ECBS's flowtime <= 1.5 * ecbs_bound
    audit = audit_schedules(md, got)
    assert torch.equal(got["flowtime_bound"], torch.maximum(audit["flowtime_bound"], got["ecbs_bound"]))
    assert bool(got["certified"][got["bounded"]].all())
    alone = certified(audit_schedules(md, plain), 1.5)
    assert bool((got["certified"] | ~alone).all())                      # nothing the audit certifies alone is lost
    assert bool((got["flowtime"][got["status"] == 0] >= got["flowtime_bound"][got["status"] == 0]).all())
    # the result is a result: the improver and the audit take it
    better = improve_schedules(md, got, iterations=4)
    ok = got["solved"] != 0
    assert bool((better["flowtime_after"][ok] <= better["flowtime_before"][ok]).all())
