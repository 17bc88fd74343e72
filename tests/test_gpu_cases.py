"""GPU: the case generator (csrc/sim_cases.hip through magat_pathplanning_amd/cases.py) EQUALS its cell-by-cell restatement
(tests/cases_restatement.py, pinned on the CPU by tests/test_host_cases.py) - map, start, goal, free_cells and valid, invalid
cases included - on the three kinds of raw map, the edges of the word / lane layout and hand maps with known answers; a case
depends on its global index only; and its output runs through solve_cases, expert_samples and BatchedEpisode."""
import numpy as np
import pytest
import torch

import cases_restatement as cr
import mapf_restatement as mr
from test_host_cases import ALL_VALID, HAND, HAND_SEED, TABLE, expected, expected_hand

pytestmark = pytest.mark.gpu
KEYS = ("map", "start", "goal", "free_cells", "valid")


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_mapf"]))


def run(name, device, **over):
    from magat_pathplanning_amd import generate_cases
    kind, C, H, W, N, density, complexity, seed = TABLE[name]
    kw = dict(density=density, complexity=complexity, kind=kind, seed=seed, device=device)
    kw.update(over)
    return generate_cases(kw.pop("C", C), H, W, N, **kw)


def assert_equal_cases(got, want, what):
    assert got["map"].dtype == torch.uint8 and got["valid"].dtype == torch.uint8
    assert got["start"].dtype == got["goal"].dtype == got["free_cells"].dtype == torch.int32
    for key in KEYS:
        w = want[key].cpu().numpy() if isinstance(want[key], torch.Tensor) else want[key]
        assert tuple(got[key].shape) == w.shape, (what, key)
        np.testing.assert_array_equal(got[key].cpu().numpy(), w, err_msg="%s: %s" % (what, key))


@pytest.mark.parametrize("name", list(TABLE))
def test_generated_cases_equal_the_restatement(gpu_device, name):
    want = expected(name)
    got = run(name, gpu_device)
    assert_equal_cases(got, want, name)
    if name in ALL_VALID:
        assert bool(got["valid"].all())
    if name == "c300_dense":                                              # invalid cases are compared too
        assert 0 < int(got["valid"].sum()) < 300
    if name in ("wide5x64", "full64"):                                    # column 63 is on the map: free somewhere, an obstacle somewhere
        assert 0 < int(got["map"][:, :, 63].sum()) < got["map"][:, :, 63].numel()
    if name in ("tall64x5", "full64"):
        assert 0 < int(got["map"][:, 63, :].sum()) < got["map"][:, 63, :].numel()


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_maps_as_given(gpu_device, name, batched):
    from magat_pathplanning_amd import generate_cases
    k = HAND[name]
    want = expected_hand(name, batched)
    if batched:
        maps = np.stack([HAND["serpentine"]["map"], k["map"], HAND["corner_obstacle"]["map"]])
        got = generate_cases(3, 6, 8, k["N"], obstacle_map=torch.from_numpy(maps).to(gpu_device), seed=HAND_SEED, device=gpu_device)
    else:      # any non-zero value is an obstacle
        got = generate_cases(2, 6, 8, k["N"], obstacle_map=torch.from_numpy(k["map"] * 200).to(gpu_device), kind="given",
                             seed=HAND_SEED, device=gpu_device)
    assert_equal_cases(got, want, name)
    c = 1 if batched else 0
    assert int(got["free_cells"][c]) == k["free_cells"] and int(got["valid"][c]) == k["valid"]


def test_a_full_width_serpentine_and_a_ring_through_the_corners(gpu_device):
    """64 x 64: ONE corridor through every row over the full width (the flood has to turn at bit 0 and bit 63 of every other
    row, down to lane 63), and the outermost ring only (the kept region holds all four corners and nothing wraps around)."""
    from magat_pathplanning_amd import generate_cases
    snake = cr.serpentine(64, 64)
    ring = np.ones((64, 64), dtype=np.uint8)
    ring[0, :] = ring[63, :] = ring[:, 0] = ring[:, 63] = 0
    ring[20:30, 20:30] = 0                                                # a 100-cell room inside: smaller than the ring's 252
    maps = np.stack([snake, ring])
    want = cr.generate("given", 2, 64, 64, 6, seed=21, maps=maps)
    got = generate_cases(2, 64, 64, 6, obstacle_map=torch.from_numpy(maps).to(gpu_device), seed=21, device=gpu_device)
    assert_equal_cases(got, want, "serpentine + ring")
    assert got["free_cells"].tolist() == [int((snake == 0).sum()), 252] and got["valid"].tolist() == [1, 1]
    assert torch.equal(got["map"][0].cpu(), torch.from_numpy(snake))


def test_split_batches_and_repeated_calls_are_equal(gpu_device):
    from magat_pathplanning_amd import valid_cases
    for name in ("maze10", "uni10", "c300_dense"):
        whole = run(name, gpu_device)
        again = run(name, gpu_device)
        half = TABLE[name][1] // 2
        a, b = run(name, gpu_device, C=half), run(name, gpu_device, C=TABLE[name][1] - half, first_case=half)
        assert_equal_cases(again, whole, name + " twice")
        assert_equal_cases({k: torch.cat([a[k], b[k]]) for k in KEYS}, whole, name + " split")
        other = run(name, gpu_device, seed=TABLE[name][7] + 1)
        assert not torch.equal(other["map"], whole["map"])
    ok = valid_cases(whole)                                               # c300_dense
    idx = torch.nonzero(whole["valid"]).flatten()
    assert torch.equal(ok["index"], idx) and 0 < len(idx) < 300 and bool(ok["valid"].all()) and int(ok["start"].min()) >= 0
    for key in KEYS:
        assert torch.equal(ok[key], whole[key][idx])


def test_one_counted_launch_per_call_and_no_host_synchronisation(gpu_device, tag_counts):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import generate_cases
    want = expected("maze10")
    before = form_count()
    with tag_counts() as tc:
        run("maze10", gpu_device)
        assert form_count() == before + 1
        run("uni10", gpu_device)
        assert form_count() == before + 2
    assert tc["sim_mapf"] == 2
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # beyond the limits: refused, nothing launched
        generate_cases(4, 65, 10, 3, kind="uniform", device=gpu_device)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        generate_cases(4, 3, 10, 3, kind="maze", device=gpu_device)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        generate_cases(4, 4, 4, 17, kind="uniform", device=gpu_device)
    assert form_count() == before + 2
    # a call that waited for the device could not be captured into a graph
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run("maze10", gpu_device)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run("maze10", gpu_device)
    for key in KEYS:
        out[key].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_equal_cases(out, want, "replay")


def test_generated_cases_run_through_the_pipeline(gpu_device):
    """40 x (10 x 10, 8 agents): the device solver and the restatement solver agree on the generated input, every solved
    schedule is a valid one, expert_samples takes it, BatchedEpisode accepts the generated tensors.  (Every valid case is
    solvable in principle - starts and goals share one component - but the solver is incomplete: `all solved` is not asserted.)"""
    from magat_pathplanning_amd import BatchedEpisode, expert_samples, pack_cases, solve_cases, solved_pack
    cases = run("maze10", gpu_device)
    want = expected("maze10")
    assert bool(cases["valid"].all())
    T = 48
    res = solve_cases(cases["map"], cases["start"], cases["goal"], horizon=T, retries=8)
    ref = mr.solve_batch(want["map"], want["start"], want["goal"], T, retries=8)
    for key in ("paths", "lengths", "makespan", "solved", "failed_agent", "order", "rounds"):
        np.testing.assert_array_equal(res[key].cpu().numpy(), ref[key], err_msg=key)
    solved = np.nonzero(ref["solved"])[0]
    assert len(solved) > 0
    paths, lengths = res["paths"].cpu().numpy(), res["lengths"].cpu().numpy()
    for c in solved:
        assert mr.check_schedule(want["map"][c], want["start"][c], want["goal"][c], paths[c], lengths[c]) is None, c
    pack = solved_pack(res)
    s = expert_samples(cases["map"].index_select(0, pack_cases(res)), comm_radius=7, **pack)
    steps = s["valid"].bool()                                             # (K,T)
    assert tuple(s["target"].shape) == (len(solved), pack["T"], 8, 5)
    assert int(steps.sum()) == int((pack["makespan"] + 1).sum())
    assert bool((s["target"].sum(-1)[steps] == 1).all())                  # one action per agent and step
    ep = BatchedEpisode(cases["map"], cases["start"], cases["goal"], maxstep=T, comm_radius=7.0)
    ep.step(actions=torch.full((40, 8), 4, dtype=torch.int32, device=gpu_device))
    assert torch.equal(ep.pos, cases["start"]) and torch.equal(ep.goal, cases["goal"]) and int((ep.flags & 15).max()) == 0
