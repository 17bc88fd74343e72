"""GPU: the wide form of ECBS (csrc/sim_mapf_ecbs_wide.hip through magat_pathplanning_amd/mapf.py ecbs_cases_wide) EQUALS the
restatement (tests/ecbs_restatement.py, unchanged) in every output, unsolved cases included: two and three wavefronts, two and four
words per row, the corners of a 65 x 65 map, a horizon of 400, trees at several (w, levels, budget), the statuses 2 and 3; the
interface around it: inputs untouched, one counted launch of the narrow form's name, the narrow routing, determinism, graph capture,
refusals, the wide audit, adopt_bounded behind solve_cases(wide=True) and a closed-loop replay.  The inputs and the restatement's
answers are tests/test_host_ecbs_wide.py's, made once per session."""
import numpy as np
import pytest
import torch

import test_host_ecbs as he
import test_host_ecbs_wide as hw
from test_gpu_ecbs import EXTRA, form_count, given
from test_gpu_ecbs import call as he_call
from test_gpu_mapf import assert_equal_results

pytestmark = pytest.mark.gpu
STRIPS = tuple(g for g in hw.GPU_INPUTS if g[0] in ("tall65x8", "wide8x65", "wide8x129", "tall129x6", "corner65"))


def call(k, md, sd, gd):
    from magat_pathplanning_amd import ecbs_cases_wide
    return ecbs_cases_wide(md, sd, gd, w=k["w_milli"] / 1000.0, horizon=k["T"], max_nodes=k["max_nodes"], levels=k["levels"])


def run(k, device):
    md, sd, gd = given(k, device)
    kept = [t.clone() for t in (md, sd, gd)]
    before = {form: form_count(form) for form in ("sim_mapf_ecbs", "sim_mapf_cbs", "sim_mapf", "sim_mapf_audit")}
    got = call(k, md, sd, gd)
    assert form_count() == before["sim_mapf_ecbs"] + 1                       # one counted launch per call, of the narrow form's name
    for form in ("sim_mapf_cbs", "sim_mapf", "sim_mapf_audit"):
        assert form_count(form) == before[form], form
    for t, was in zip((md, sd, gd), kept):                                   # the inputs are not modified
        assert torch.equal(t, was)
    assert sorted(got) == sorted(he.KEYS + ("start", "goal"))
    assert got["paths"].dtype == torch.int32 and got["solved"].dtype == torch.uint8
    assert tuple(got["paths"].shape) == k["want"]["paths"].shape
    for key in EXTRA + ("lengths", "makespan"):
        assert got[key].dtype == torch.int32 and got[key].device == md.device and got[key].is_contiguous(), key
    return got


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", hw.GPU_INPUTS)
def test_wide_ecbs_equals_restatement(gpu_device, name, w_milli, levels, max_nodes):
    k = hw.case(name, w_milli, levels, max_nodes)
    assert_equal_results(run(k, gpu_device), k["want"], he.KEYS, "%s at %r" % (name, (w_milli, levels, max_nodes)))


def test_a_narrow_shape_goes_to_the_narrow_kernel(gpu_device):
    from magat_pathplanning_amd import ecbs_cases
    k = he.case("r8", 1500, 4, 64)
    got = run(k, gpu_device)
    assert_equal_results(got, k["want"], he.KEYS, "r8 through ecbs_cases_wide")
    md, sd, gd = given(k, gpu_device)
    narrow = ecbs_cases(md, sd, gd, w=1.5, horizon=k["T"], max_nodes=64, levels=4)
    for key in he.KEYS:
        assert torch.equal(got[key], narrow[key]), key


# narrow shapes, all four K: the wide entry itself takes them (it refuses only above 256; mapf.py does the routing)
BOTH_FORMS = (("pocket", 1500, 4, 64), ("hand", 1500, 4, 64), ("small", 1500, 4, 64), ("r8", 1500, 4, 64), ("r8", 1200, 2, 64),
              ("r8", 1500, 1, 64), ("r8", 1500, 3, 8))


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", BOTH_FORMS)
def test_the_forms_agree_where_both_apply(gpu_device, name, w_milli, levels, max_nodes):
    """One walk, two forms: magat_sim_mapf_ecbs_wide called directly on a narrow shape, with a workspace of its own size, gives
    what ecbs_cases gives and what the restatement gives, in every output."""
    from magat_pathplanning_amd import _native as nat
    k = he.case(name, w_milli, levels, max_nodes)
    md, sd, gd = given(k, gpu_device)
    narrow = he_call(k, md, sd, gd)
    lib = nat.lib()
    C, N = sd.shape[:2]
    H, W = md.shape[-2:]
    T = k["T"]
    need = int(lib.magat_sim_mapf_ecbs_wide_workspace_bytes(C, H, W, N, T, max_nodes, levels))
    assert need == hw.documented_bytes(C, H, W, N, T, max_nodes, levels)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    got = dict(paths=torch.full((C, N, T, 2), -7, dtype=torch.int32, device=gpu_device),
               lengths=torch.full((C, N), -7, dtype=torch.int32, device=gpu_device),
               solved=torch.full((C,), 9, dtype=torch.uint8, device=gpu_device))
    got.update({key: torch.full((C,), -7, dtype=torch.int32, device=gpu_device) for key in ("makespan",) + EXTRA})
    rc = lib.magat_sim_mapf_ecbs_wide(nat.ptr(md), int(md.dim() == 3), H, W, nat.ptr(sd), nat.ptr(gd), nat.ptr(got["paths"]),
                                      nat.ptr(got["lengths"]), nat.ptr(got["makespan"]), nat.ptr(got["solved"]),
                                      *[nat.ptr(got[key]) for key in EXTRA], nat.ptr(ws), need, C, N, T, max_nodes, w_milli, levels,
                                      nat.current_stream(sd.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert set(he.KEYS) == set(got)
    for key in he.KEYS:
        assert torch.equal(got[key], narrow[key]), key
    assert_equal_results(got, k["want"], he.KEYS, "%s at %r through the wide entry" % (name, (w_milli, levels, max_nodes)))


def test_more_cases_than_compute_units(gpu_device):
    k = he.tiled(hw.case("crowd66x5", 1500, 3, 8), 300)
    assert_equal_results(run(k, gpu_device), k["want"], he.KEYS, "crowd66x5 tiled to 300 cases")


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", STRIPS)
def test_status_0_schedules_pass_the_wide_audit(gpu_device, name, w_milli, levels, max_nodes):
    from magat_pathplanning_amd import audit_schedules
    k = hw.case(name, w_milli, levels, max_nodes)
    md, sd, gd = given(k, gpu_device)
    got = call(k, md, sd, gd)
    audit = audit_schedules(md, got, wide=True)
    done = got["status"] == 0
    assert int(done.sum()) > 0
    assert bool((audit["status"][done] == 0).all()) and bool((audit["status"][~done] == 1).all())
    assert torch.equal(audit["flowtime"][done], got["flowtime"][done]) and torch.equal(audit["makespan"][done], got["makespan"][done])
    assert bool((1000 * got["flowtime"][done].to(torch.int64) <= w_milli * got["lower_bound"][done].to(torch.int64)).all())
    known = (got["status"] <= 1) & (audit["flowtime_bound"] >= 0)
    assert bool((got["lower_bound"][known] >= audit["flowtime_bound"][known]).all())      # never weaker than the audit's bound


def test_determinism_profiling_tag_and_graph_capture(gpu_device, tag_counts):
    k = hw.case("crowd66x5", 1200, 2, 64)
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


def test_refusals_launch_nothing(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import ecbs_cases, ecbs_cases_wide
    k = hw.case("crowd66x5", 1500, 3, 8)
    md, sd, gd = given(k, gpu_device)
    before = form_count()
    with pytest.raises(nat.MagatNativeError, match="256 x 256"):
        ecbs_cases_wide(torch.zeros(257, 5, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=120)
    with pytest.raises(nat.MagatNativeError, match="horizons up to 1024"):
        ecbs_cases_wide(md, sd, gd, horizon=1025)
    for nodes in (0, 4097):
        with pytest.raises(nat.MagatNativeError, match="nodes"):
            ecbs_cases_wide(md, sd, gd, horizon=120, max_nodes=nodes)
    with pytest.raises(nat.MagatNativeError, match="levels"):
        ecbs_cases_wide(md, sd, gd, horizon=120, levels=5)
    with pytest.raises(ValueError):
        ecbs_cases_wide(md, sd, gd, w=0.5, horizon=120)
    with pytest.raises(nat.MagatNativeError):
        ecbs_cases_wide(md.cpu(), sd.cpu(), gd.cpu())                      # CPU tensors
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):            # the narrow name still refuses a 65-row map
        ecbs_cases(md, sd, gd, horizon=120)
    # the entry itself: the limits, and a workspace one byte short
    lib = nat.lib()
    C, N = sd.shape[:2]
    H, W = md.shape
    need = int(lib.magat_sim_mapf_ecbs_wide_workspace_bytes(C, H, W, N, 120, 8, 3))
    assert need == hw.documented_bytes(C, H, W, N, 120, 8, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    paths = torch.full((C, N, 120, 2), -7, dtype=torch.int32, device=gpu_device)
    lengths = torch.empty(C, N, dtype=torch.int32, device=gpu_device)
    solved = torch.empty(C, dtype=torch.uint8, device=gpu_device)
    extra = torch.empty(7, C, dtype=torch.int32, device=gpu_device)

    def entry(H=H, ws_bytes=need, w=1500):
        return lib.magat_sim_mapf_ecbs_wide(nat.ptr(md), 0, H, W, nat.ptr(sd), nat.ptr(gd), nat.ptr(paths), nat.ptr(lengths),
                                            nat.ptr(extra[0]), nat.ptr(solved), *[nat.ptr(extra[i]) for i in range(1, 7)], nat.ptr(ws),
                                            ws_bytes, C, N, 120, 8, w, 3, nat.current_stream(sd.device))

    assert entry(ws_bytes=need - 1) == -2 and entry(H=257) == -2 and entry(w=999) == -1
    torch.cuda.synchronize()
    assert form_count() == before and int(paths.max()) == -7              # nothing was launched, nothing was written
    assert entry() == 0
    torch.cuda.synchronize()
    assert form_count() == before + 1
    np.testing.assert_array_equal(paths.cpu().numpy(), k["want"]["paths"])


def test_adopt_bounded_behind_the_wide_solver(gpu_device):
    from magat_pathplanning_amd import adopt_bounded, audit_schedules, certified, solve_cases
    k = hw.case("crowd66x5", 1000, 4, 64)
    want = k["want"]
    md, sd, gd = given(k, gpu_device)
    res = solve_cases(md, sd, gd, horizon=k["T"], wide=True)
    sub = call(k, md, sd, gd)
    got = adopt_bounded(res, sub)
    assert set(got) == (set(res) - {"T"}) | {"ecbs_status", "ecbs_bound", "ecbs_nodes", "bounded"}
    done = want["status"] == 0
    np.testing.assert_array_equal(got["bounded"].cpu().numpy(), done)
    np.testing.assert_array_equal(got["ecbs_status"].cpu().numpy(), want["status"])
    np.testing.assert_array_equal(got["ecbs_nodes"].cpu().numpy(), want["nodes"])
    np.testing.assert_array_equal(got["ecbs_bound"].cpu().numpy(), np.where(want["horizon_hit"] == 0, want["lower_bound"], -1))
    # the replacement rule, case by case: a status-0 case replaces the plan only where the plan is unsolved or has a larger flowtime
    plan = {key: res[key].cpu().numpy() for key in ("paths", "lengths", "makespan", "solved", "failed_agent")}
    flow_plan = (plan["lengths"].astype(np.int64) - 1).sum(1)
    take = done & ((plan["solved"] == 0) | (flow_plan > want["flowtime"]))
    assert take.any()
    for key in ("paths", "lengths", "makespan"):
        np.testing.assert_array_equal(got[key].cpu().numpy()[take], want[key][take], err_msg=key)
        np.testing.assert_array_equal(got[key].cpu().numpy()[~take], plan[key][~take], err_msg=key)
    np.testing.assert_array_equal(got["solved"].cpu().numpy(), (plan["solved"] != 0) | take)
    np.testing.assert_array_equal(got["failed_agent"].cpu().numpy(), np.where(take, -1, plan["failed_agent"]))
    with pytest.raises(ValueError, match="horizon"):
        adopt_bounded(res, call(dict(k, T=k["T"] + 1), md, sd, gd))
    # certified at its w: every case the search bounded, since flowtime <= ECBS's flowtime <= w * ecbs_bound
    audit = audit_schedules(md, got, wide=True)
    audit["flowtime_bound"] = torch.maximum(audit["flowtime_bound"], got["ecbs_bound"])
    assert int(got["bounded"].sum()) > 0 and bool(certified(audit, 1.0)[got["bounded"]].all())


def test_closed_loop_replay_and_expert_samples(gpu_device):
    """wide8x129: the action keys of its schedules replayed through BatchedEpisode(..., wide=True).step collide nowhere and end at
    the goals; expert_samples(..., wide=True) takes the result as **pack."""
    from magat_pathplanning_amd import BatchedEpisode, expert_samples, expert_schedule, flatten_samples, solved_pack
    k = hw.case("wide8x129", 1500, 4, 64)
    md, sd, gd = given(k, gpu_device)
    res = call(k, md, sd, gd)
    assert int(res["solved"].sum()) == len(k["start"])
    pack = solved_pack(res)
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=pack["T"], check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)                   # (C,T,N)
    keys[sched["valid"] == 0] = 4                                       # behind a case's last step: stop
    ep = BatchedEpisode(md, pack["start"], pack["goal"], maxstep=pack["T"] + 2, comm_radius=7.0, wide=True)
    ep.currentstep = 1
    for t in range(pack["T"]):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    flat = flatten_samples(expert_samples(md, comm_radius=7, wide=True, **pack))
    assert flat["inputTensor"].shape[0] == int((pack["makespan"] + 1).sum())
