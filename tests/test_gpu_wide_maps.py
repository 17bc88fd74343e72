"""GPU: the wide forms of the solver and the case generator (csrc/sim_mapf_wide.hip, csrc/sim_cases_wide.hip through
`wide=True`; maps up to 256 x 256, horizons up to 1024) EQUAL the cell-by-cell restatements (tests/mapf_restatement.py,
tests/cases_restatement.py) - every output an integer equality, unsolved and invalid cases included - at the word and wave
boundaries, the edges, long horizons and in batches; where both forms take a shape they give the same result; the call is
stream ordered; and the 65 x 65 / 100-robot pipeline runs from the generator to the samples.  Inputs and expected results:
tests/test_host_wide_maps.py."""
import numpy as np
import pytest
import torch

import mapf_restatement as mr
from test_host_wide_maps import (GEN_NAMES, PLAN_NAMES, SOLVE_NAMES, batch, expected_cases, expected_plan, expected_solve,
                                 gen_case)

pytestmark = pytest.mark.gpu
PLAN_KEYS = ("paths", "lengths", "makespan", "solved", "failed_agent")
CASE_KEYS = ("map", "start", "goal", "free_cells", "valid")


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def assert_equal(got, want, keys, what):
    for key in keys:
        w = want[key].cpu().numpy() if isinstance(want[key], torch.Tensor) else np.asarray(want[key])
        assert tuple(got[key].shape) == w.shape, (what, key)
        np.testing.assert_array_equal(got[key].cpu().numpy(), w, err_msg="%s: %s" % (what, key))


def run_plan(name, device, **kw):
    from magat_pathplanning_amd import plan_prioritized
    m, s, g, order, T = batch(name)
    return plan_prioritized(dev(m, device), dev(s, device), dev(g, device), None if order is None else dev(order, device), T,
                            wide=True, **kw)


def run_generate(name, device, **over):
    from magat_pathplanning_amd import generate_cases
    kind, C, H, W, N, density, complexity, seed, maps = gen_case(name)
    kw = dict(density=density, complexity=complexity, kind=kind, seed=seed, device=device, wide=True,
              obstacle_map=None if maps is None else dev(maps, device))
    kw.update(over)
    return generate_cases(kw.pop("C", C), H, W, N, **kw)


@pytest.mark.parametrize("name", PLAN_NAMES)
def test_wide_plan_equals_restatement(gpu_device, name):
    want = expected_plan(name)
    got = run_plan(name, gpu_device)
    assert got["paths"].dtype == torch.int32 and got["solved"].dtype == torch.uint8
    assert_equal(got, want, PLAN_KEYS, name)
    # what the batch is there for
    if name.startswith("hops") or name.startswith("ring"):
        assert want["solved"].tolist() == [1]
    if name == "ring256":
        assert want["lengths"].tolist() == [[255] * 4]
    if name == "corridors":
        assert want["solved"].tolist() == [1, 1, 0, 0, 1, 0]
    if name == "serpentine_T1024":
        assert want["solved"].tolist() == [1] and want["lengths"].min() - 1 > 256
    if name == "serpentine_one_short":
        assert want["solved"].tolist() == [0] and want["failed_agent"].tolist() == [0]
    if name == "clusters65":
        assert 0 < int(want["solved"].sum()) < 40
    if name == "bad_cases":
        assert want["failed_agent"].tolist()[1:3] == [-2, 4]


@pytest.mark.parametrize("name", SOLVE_NAMES)
def test_wide_solve_cases_equals_solve_with_retries(gpu_device, name):
    from magat_pathplanning_amd import solve_cases
    m, s, g, _, T = batch(name)
    want = expected_solve(name)
    got = solve_cases(dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device), horizon=T, retries=8, wide=True)
    assert_equal(got, want, PLAN_KEYS + ("order", "rounds"), name)
    done = want["makespan"][want["solved"] != 0]
    assert got["T"] == int(done.max()) + 1
    assert int(want["rounds"].max()) == 9 and 2 in want["rounds"].tolist()      # promotions that help, and cases that stay unsolved
    for c in np.nonzero(want["solved"])[0]:
        mc = m if m.ndim == 2 else m[c]
        assert mr.check_schedule(mc, s[c], g[c], got["paths"][c].cpu().numpy(), got["lengths"][c].cpu().numpy()) is None, c


@pytest.mark.parametrize("name", GEN_NAMES)
def test_wide_generated_cases_equal_the_restatement(gpu_device, name):
    want = expected_cases(name)
    got = run_generate(name, gpu_device)
    assert got["map"].dtype == torch.uint8 and got["start"].dtype == torch.int32
    assert_equal(got, want, CASE_KEYS, name)
    if name == "given70x130":
        assert got["valid"].tolist() == [1, 0, 0] and got["free_cells"].tolist()[1:] == [1, 4]
    elif name == "uni256":
        assert got["valid"].tolist() == [1] and len({int(r) // 64 for r in want["start"][0, :, 0]}) == 4
    else:
        assert bool(got["valid"].all())
    if name.startswith("uni"):      # the last column and the last row are on the map: free somewhere, an obstacle somewhere
        H, W = gen_case(name)[2:4]
        assert 0 < int(got["map"][:, :, W - 1].sum()) < got["map"][:, :, W - 1].numel()
        assert 0 < int(got["map"][:, H - 1, :].sum()) < got["map"][:, H - 1, :].numel()


def test_wide_split_batches_are_equal(gpu_device):
    whole = run_generate("uni65", gpu_device)
    a, b = run_generate("uni65", gpu_device, C=3), run_generate("uni65", gpu_device, C=3, first_case=3)
    assert_equal({k: torch.cat([a[k], b[k]]) for k in CASE_KEYS}, whole, CASE_KEYS, "3 + 3")
    assert not torch.equal(a["map"], b["map"])


def test_both_forms_agree_where_both_apply(gpu_device):
    """20 x 20: wide=True goes to the 64 x 64 kernels (no count of a wide launch could tell: the form is shared), and the wide
    entry points themselves, called directly at that shape, give the same bytes."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import generate_cases, plan_prioritized, solve_cases
    m, s, g = mr.random_batch(11, 16, 20, 20, 10, 0.1)
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    for fn, kw in ((plan_prioritized, dict(horizon=64)), (solve_cases, dict(horizon=64))):
        a, b = fn(md, sd, gd, wide=False, **kw), fn(md, sd, gd, wide=True, **kw)
        assert sorted(a) == sorted(b)
        assert_equal(b, a, [k for k in a if k != "T"], fn.__name__)
        assert a.get("T") == b.get("T")
    narrow = None
    for kind in ("maze", "uniform"):
        a = generate_cases(8, 20, 20, 10, density=0.2, complexity=0.05, kind=kind, seed=5, device=gpu_device)
        b = generate_cases(8, 20, 20, 10, density=0.2, complexity=0.05, kind=kind, seed=5, device=gpu_device, wide=True)
        assert_equal(b, a, CASE_KEYS, kind)
        narrow = a
    # the wide kernels at a shape of the 64 x 64 form (one wave, one word): the same plan, the same cases
    lib = nat.lib()
    a = plan_prioritized(md, sd, gd, horizon=64)
    out = {k: torch.empty_like(a[k]) for k in PLAN_KEYS}
    ws = torch.empty(int(lib.magat_sim_mapf_wide_workspace_bytes(16, 20, 20, 64)), dtype=torch.uint8, device=gpu_device)
    with torch.cuda.device(gpu_device):
        nat.check(lib.magat_sim_mapf_plan_wide(nat.ptr(md), 0, 20, 20, nat.ptr(sd), nat.ptr(gd), None, nat.ptr(out["paths"]),
                                               nat.ptr(out["lengths"]), nat.ptr(out["makespan"]), nat.ptr(out["solved"]),
                                               nat.ptr(out["failed_agent"]), nat.ptr(ws), ws.numel(), 16, 10, 64,
                                               nat.current_stream(gpu_device)), "magat_sim_mapf_plan_wide")
        gen = {k: torch.empty_like(narrow[k]) for k in CASE_KEYS}
        nat.check(lib.magat_sim_cases_generate_wide(1, None, 0, 20, 20, 0, 0, int(0.2 * 4294967296.0), 5, 0, nat.ptr(gen["map"]),
                                                    nat.ptr(gen["start"]), nat.ptr(gen["goal"]), nat.ptr(gen["free_cells"]),
                                                    nat.ptr(gen["valid"]), 8, 10, nat.current_stream(gpu_device)),
                  "magat_sim_cases_generate_wide")
    assert_equal(out, a, PLAN_KEYS, "wide kernel at 20 x 20")
    assert_equal(gen, narrow, CASE_KEYS, "wide generator at 20 x 20")


def test_wide_call_is_counted_once_and_stream_ordered(gpu_device, tag_counts):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import plan_prioritized
    m, s, g, _, T = batch("clusters65")
    md, sd, gd = dev(m, gpu_device), dev(s, gpu_device), dev(g, gpu_device)
    lib = nat.lib()
    before = int(lib.magat_form_count(nat.FORMS["sim_mapf"]))
    with tag_counts() as tc:
        eager = plan_prioritized(md, sd, gd, horizon=T, wide=True)
        run_generate("uni65", gpu_device)
    assert int(lib.magat_form_count(nat.FORMS["sim_mapf"])) == before + 2 and tc["sim_mapf"] == 2
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # beyond the wide limits: refused, nothing launched
        plan_prioritized(torch.zeros(257, 10, dtype=torch.uint8, device=gpu_device), sd, gd, horizon=T, wide=True)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        plan_prioritized(md, sd, gd, horizon=1025, wide=True)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # and without the keyword 65 is refused as before
        plan_prioritized(md, sd, gd, horizon=T)
    assert int(lib.magat_form_count(nat.FORMS["sim_mapf"])) == before + 2
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        plan_prioritized(md, sd, gd, horizon=T, wide=True)
    torch.cuda.current_stream().wait_stream(side)
    ss = sd.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan_prioritized(md, ss, gd, horizon=T, wide=True)
    ss.copy_(sd.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    flipped = plan_prioritized(md, sd.flip(0).contiguous(), gd, horizon=T, wide=True)
    assert_equal(out, flipped, PLAN_KEYS, "replay on new starts")
    ss.copy_(sd)
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(out, eager, PLAN_KEYS, "replay")
    assert_equal(eager, expected_plan("clusters65"), PLAN_KEYS, "eager")


def test_pipeline_at_65x65_with_100_robots(gpu_device):
    """The reference's largest in-distribution shape, two cases: generate, solve, check every solved schedule, replay it
    through BatchedEpisode.step with no collision flag and the expert's makespan, and make samples of it."""
    from magat_pathplanning_amd import (BatchedEpisode, expert_samples, expert_schedule, expert_stats, generate_cases, pack_cases,
                                        solve_cases, solved_pack)
    C, N = 2, 100
    cases = generate_cases(C, 65, 65, N, density=0.1, complexity=0.01, seed=61, device=gpu_device, wide=True)
    assert bool(cases["valid"].all())
    res = solve_cases(cases["map"], cases["start"], cases["goal"], wide=True)
    assert res["paths"].shape[2] == 360
    idx = pack_cases(res)
    assert idx.numel() > 0
    pack = solved_pack(res)
    maps = cases["map"].index_select(0, idx)
    T = pack["T"]
    mh, sh, gh = maps.cpu().numpy(), pack["start"].cpu().numpy(), pack["goal"].cpu().numpy()
    ph, lh = pack["paths"][:, :, :T + 1].cpu().numpy(), pack["lengths"].cpu().numpy()      # behind T every path is padding
    assert bool((pack["paths"][:, :, T:] == pack["paths"][:, :, T - 1:T]).all())
    for c in range(len(idx)):
        assert mr.check_schedule(mh[c], sh[c], gh[c], ph[c], lh[c]) is None, c
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=T, check=True)
    assert int(sched["bad"].max()) == -1
    keys = sched["target"].argmax(-1).to(torch.int32)
    keys[sched["valid"] == 0] = 4
    stats = expert_stats(sched["target"], pack["start"], pack["goal"], sched["valid"])
    ep = BatchedEpisode(maps, pack["start"], pack["goal"], maxstep=T + 2, comm_radius=7.0)
    ep.currentstep = 1
    for t in range(T):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    assert torch.equal(ep.makespan, stats["makespanTarget"])
    samples = expert_samples(maps, comm_radius=7, **pack)
    steps = samples["valid"].bool()
    assert tuple(samples["target"].shape) == (len(idx), T, N, 5)
    assert int(steps.sum()) == int((pack["makespan"] + 1).sum())
    assert bool((samples["target"].sum(-1)[steps] == 1).all())
