"""GPU: the schedule audit (csrc/sim_mapf_audit.hip and csrc/sim_mapf_audit_wide.hip through magat_pathplanning_amd/mapf.py
audit_schedules) EQUALS its restatement (tests/audit_restatement.py, pinned on the CPU by tests/test_host_audit.py) - status,
fault, dist, both bounds, flowtime and makespan - on the solver's output, on corrupted schedules, on the edges of the word /
lane / wavefront layout of both forms; the interface around it: inputs untouched, one counted launch, graph capture,
certified / certified_pack / solve_cases(certify=), limits.  The inputs and the restatement's answers are
tests/test_host_audit.py's, made once per session."""
import numpy as np
import pytest
import torch

import audit_restatement as ar
import mapf_restatement as mr
import test_host_audit as ha
from test_gpu_mapf import assert_equal_results, dev

pytestmark = pytest.mark.gpu
IN_KEYS = ("paths", "lengths", "start", "goal", "solved")


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf_audit"]))


def given(name, device):
    k = ha.case(name)
    return dev(k["map"], device), {key: dev(k[key], device) for key in IN_KEYS if k[key] is not None}


def run(name, device, wide=None):
    from magat_pathplanning_amd import audit_schedules
    k = ha.case(name)
    md, res = given(name, device)
    kept = {key: value.clone() for key, value in res.items()}
    kept_map = md.clone()
    before = form_count()
    got = audit_schedules(md, res, wide=k["wide"] if wide is None else wide)
    assert form_count() == before + 1                                    # one counted launch per call
    for key in res:                                                      # the inputs are not modified
        assert torch.equal(res[key], kept[key]), key
    assert torch.equal(md, kept_map)
    assert sorted(got) == sorted(ar.KEYS)
    for key in ar.KEYS:
        assert got[key].dtype == torch.int32 and got[key].device == md.device, key
    return got, k["want"]


@pytest.mark.parametrize("name", ha.ALL_NAMES)
def test_audit_equals_restatement(gpu_device, name):
    ha.check_what_the_case_is_there_for(name)
    got, want = run(name, gpu_device)
    assert_equal_results(got, want, ar.KEYS, name)


@pytest.mark.parametrize("name", ha.NAMES_64)
def test_wide_entry_on_the_64_forms_inputs(gpu_device, name):
    """audit_schedules(..., wide=True) sends a shape inside 64 x 64 to the 64 form, so the wide kernel is reached here through its
    entry, with a workspace of exactly the size it asks for: every output equals the 64 form's and the restatement's."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import audit_schedules
    k = ha.case(name)
    md, res = given(name, gpu_device)
    narrow = audit_schedules(md, res)
    C, N, T, _ = res["paths"].shape
    H, W = md.shape[-2:]
    lib = nat.lib()
    out = {key: torch.full_like(narrow[key], -7) for key in ar.KEYS}
    ws = torch.empty(lib.magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T), dtype=torch.uint8, device=gpu_device)
    with torch.cuda.device(gpu_device):
        rc = lib.magat_sim_mapf_audit_wide(nat.ptr(md), int(md.dim() == 3), H, W, nat.ptr(res.get("solved")), nat.ptr(res["paths"]),
                                           nat.ptr(res["lengths"]), nat.ptr(res["start"]), nat.ptr(res["goal"]), nat.ptr(out["status"]),
                                           nat.ptr(out["fault"]), nat.ptr(out["dist"]), nat.ptr(out["flowtime_bound"]),
                                           nat.ptr(out["makespan_bound"]), nat.ptr(out["flowtime"]), nat.ptr(out["makespan"]), nat.ptr(ws),
                                           ws.numel(), C, N, T, nat.current_stream(gpu_device))
    nat.check(rc, "magat_sim_mapf_audit_wide")
    for key in ar.KEYS:
        assert torch.equal(out[key], narrow[key]), (name, key)
    assert_equal_results(out, k["want"], ar.KEYS, name)


def test_hand_cases_planned_on_the_device(gpu_device):
    """The five hand cases as one (5,5,7) batch with a map per case, planned on the device: the unsolved ones come back skipped
    and still carry dist."""
    from magat_pathplanning_amd import audit_schedules, plan_prioritized
    k = ha.case("hand")
    md = dev(k["map"], gpu_device)
    res = plan_prioritized(md, dev(k["start"], gpu_device), dev(k["goal"], gpu_device), None, 24)
    assert_equal_results(res, k, ("paths", "lengths", "solved"), "the plan")
    got = audit_schedules(md, res)
    assert_equal_results(got, k["want"], ar.KEYS, "hand, planned on the device")
    skipped = got["status"] == 1
    assert 0 < int(skipped.sum()) < 5 and int(got["dist"][skipped].min()) >= 0 and bool((got["flowtime"][skipped] == -1).all())


@pytest.mark.parametrize("improve", [0, 8])
def test_seed7_through_solve_cases(gpu_device, improve):
    from magat_pathplanning_amd import audit_schedules, solve_cases
    m, s, g, _ = ha.seed7()
    md = dev(m, gpu_device)
    res = solve_cases(md, dev(s, gpu_device), dev(g, gpu_device), horizon=90, improve=improve)
    got = audit_schedules(md, res)
    paths, lengths = res["paths"].cpu().numpy(), res["lengths"].cpu().numpy()
    want = ha.case("seed7")["want"] if improve == 0 else ar.audit_batch(m, s, g, paths, lengths, res["solved"].cpu().numpy())
    assert_equal_results(got, want, ar.KEYS, "solve_cases(improve=%d)" % improve)
    assert got["status"].tolist() == [0] * 16 and bool((got["flowtime"] >= got["flowtime_bound"]).all())
    if improve:
        assert torch.equal(got["flowtime"], res["flowtime_after"])
        assert int(got["flowtime"].sum()) <= int(ha.case("seed7")["want"]["flowtime"].sum())
        assert torch.equal(got["flowtime_bound"].cpu(), torch.from_numpy(ha.case("seed7")["want"]["flowtime_bound"]))


def test_wide_keyword_at_a_64_shape_and_refusals(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import audit_schedules
    narrow, want = run("seed7", gpu_device, wide=False)
    wide, _ = run("seed7", gpu_device, wide=True)
    for key in ar.KEYS:
        assert torch.equal(narrow[key], wide[key]), key
    assert_equal_results(wide, want, ar.KEYS, "wide=True at 20 x 20")
    count = form_count()
    md, res = given("open65", gpu_device)
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):
        audit_schedules(md, res)
    md, res = given("hand_T300", gpu_device)
    long = dict(res, paths=res["paths"][:, :, :257].contiguous())
    with pytest.raises(nat.MagatNativeError, match="horizons up to 256"):
        audit_schedules(md, long)
    with pytest.raises(nat.MagatNativeError):
        audit_schedules(md.cpu(), {key: value.cpu() for key, value in res.items()}, wide=True)      # CPU tensors
    assert form_count() == count


def test_profiling_tag_and_graph_capture(gpu_device, tag_counts):
    from magat_pathplanning_amd import audit_schedules
    want = ha.case("corrupted")["want"]
    md, res = given("corrupted", gpu_device)
    with tag_counts() as tc:
        eager = audit_schedules(md, res)
    assert tc["sim_mapf_audit"] == 1 and tc["sim_mapf"] == 0 and tc["sim_mapf_lns"] == 0
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        audit_schedules(md, res)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = audit_schedules(md, res)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_results(out, want, ar.KEYS, "replay")
    assert_equal_results(eager, want, ar.KEYS, "eager")


def test_certified_and_certified_pack(gpu_device):
    from magat_pathplanning_amd import audit_schedules, certified, certified_pack, expert_samples, flatten_samples, solved_pack
    k = ha.case("seed7")
    md, res = given("seed7", gpu_device)
    res["makespan"] = (res["lengths"].max(1).values - 1).to(torch.int32)
    audit = audit_schedules(md, res)
    for w in (1, 1.05, 2):
        ok = certified(audit, w)
        assert ok.dtype == torch.bool and ok.device == md.device
        np.testing.assert_array_equal(ok.cpu().numpy(), ar.certified(k["want"], w), err_msg="w = %r" % w)
    with pytest.raises(ValueError):
        certified(audit, 0.9)
    keep = ar.certified(k["want"], 1.05)
    assert 0 < int(keep.sum()) < 16
    pack = certified_pack(res, audit, 1.05)
    assert sorted(pack) == sorted(solved_pack(res))
    idx = torch.from_numpy(np.nonzero(keep)[0]).to(gpu_device)
    for key in ("paths", "lengths", "goal", "start", "makespan"):
        assert torch.equal(pack[key], res[key].index_select(0, idx)), key
    assert pack["T"] == int(pack["makespan"].max()) + 1
    flat = flatten_samples(expert_samples(md, comm_radius=7, **pack))
    assert flat["inputTensor"].shape[0] == int((pack["makespan"] + 1).sum())
    # the other component: bound -1, certified at no w; and nothing left is an error
    md, res = given("other_component", gpu_device)
    res["makespan"] = (res["lengths"].max(1).values - 1).to(torch.int32)
    audit = audit_schedules(md, res)
    assert not bool(certified(audit, 100).any())
    with pytest.raises(ValueError):
        certified_pack(res, audit, 100)


def test_solve_cases_with_certify(gpu_device):
    from magat_pathplanning_amd import audit_schedules, certified, solve_cases
    m, s, g, _ = ha.seed7()
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    plain = solve_cases(md, sd, gd, horizon=90)
    before = form_count()
    both = solve_cases(md, sd, gd, horizon=90, certify=1.05)
    assert form_count() == before + 1
    audit = audit_schedules(md, plain)
    assert sorted(both) == sorted(set(plain) | set(ar.KEYS) | {"certified"})
    for key in plain:                                  # what was there stays what it was (makespan: the solver's, equal here)
        if key != "T":
            assert torch.equal(both[key], plain[key]), key
    assert both["T"] == plain["T"]
    for key in ar.KEYS:
        assert torch.equal(both[key], audit[key]), key
    assert torch.equal(both["certified"], certified(audit, 1.05))
    np.testing.assert_array_equal(both["certified"].cpu().numpy(), ar.certified(ha.case("seed7")["want"], 1.05))
