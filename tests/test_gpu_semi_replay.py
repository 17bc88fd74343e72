"""GPU: SemiLG states from the schedule alone - replayed_semi_states (magat_sim_replayed_states[_wide]), expert_samples(
replay=True) and ExpertMemory(replay=True).  Every comparison is torch.equal / array_equal of {0,1} tensors: against the guid_* /
guidw_* / expert_* fixtures the real reference made, against the carried-view route that existed before, and - on scenes the
fixtures do not hold - against tests/semi_replay_restatement.py, which tests/test_host_semi_replay.py pins to those fixtures."""
import functools

import numpy as np
import pytest
import torch

import semi_replay_restatement as sr
import test_host_semi_replay as hs
import test_host_wide_loop as hw

pytestmark = pytest.mark.gpu

FOV = 9
NARROW = [p for p in hs.STEP_FIXTURES if "guid_" in p]
WIDE = [p for p in hs.STEP_FIXTURES if "guidw_" in p]
SAMPLE_KEYS = ("inputTensor", "target", "GSO", "pos", "case", "step")


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def i32(a, device):
    return dev(np.asarray(a).astype(np.int32), device)


def form_count(form):
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS[form]))


def every_step(z, device, wide):
    """All (instance, step) pairs of a step fixture as ONE batch with the position table as history."""
    from magat_pathplanning_amd import replayed_semi_states
    B, T, N, _ = z["pos"].shape
    case, step = np.repeat(np.arange(B), T), np.tile(np.arange(T), B)
    hist = dict(case=i32(case, device), step=i32(step, device), table=i32(z["pos"], device))
    return replayed_semi_states(dev(z["map"][case], device), i32(z["pos"][case, step], device), i32(z["goal"][case], device), hist,
                                FOV, hs.guidance_of(str(z["_path"])), wide=wide), case, step


def load(path):
    z = dict(np.load(path, allow_pickle=False))
    z["_path"] = path
    return z


# ---- 1. narrow, position-table history ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", NARROW, ids=[i for i in hs.STEP_IDS if i.startswith("guid_")])
def test_narrow_replay_equals_the_reference_at_every_step(gpu_device, path):
    z = load(path)
    assert len(NARROW) == 6
    before = form_count("sim_replay"), form_count("sim_guided")
    x, case, step = every_step(z, gpu_device, wide=False)
    assert (form_count("sim_replay"), form_count("sim_guided")) == (before[0] + 1, before[1])
    assert torch.equal(x.cpu(), torch.from_numpy(z["x"][case, step].astype(np.float32)))


# ---- 2. the 64 x 64 canvas limit ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def canvas_limit_scene():
    m, table, goal = hs.synthetic(54, 54, 5, 12, seed=54)
    table[0, :, 0] = [(0, c) for c in range(20, 32)]      # agent 0 walks along row 0 ...
    table[0, :, 1] = [(r, 53) for r in range(30, 42)]     # ... agent 1 down column 53
    goal[0], goal[1] = (6, 40), (45, 47)
    m[0, 20:32] = 0
    m[30:42, 53] = 0
    rows = np.array([11, 4, 0])
    want = np.stack([sr.replayed_states(m, table[0, t], goal, sr.table_cells(table[0], t), "SemiLG_SD") for t in rows])
    return m, table, goal, rows, want


def test_replay_at_the_canvas_limit_equals_the_restatement(gpu_device):
    from magat_pathplanning_amd import _native as nat, replayed_semi_states
    m, table, goal, rows, want = canvas_limit_scene()
    hist = dict(case=i32(np.zeros(3), gpu_device), step=i32(rows, gpu_device), table=i32(table, gpu_device))
    x = replayed_semi_states(dev(m, gpu_device), i32(table[0, rows], gpu_device), i32(np.stack([goal] * 3), gpu_device), hist, FOV,
                             "SemiLG_SD")
    assert np.array_equal(x.cpu().numpy(), want.astype(np.float32))
    with pytest.raises(nat.MagatNativeError):             # 55 rows: beyond the narrow canvas without `wide`
        replayed_semi_states(torch.zeros(55, 54, dtype=torch.uint8, device=gpu_device), i32(table[0, rows], gpu_device),
                             i32(np.stack([goal] * 3), gpu_device), hist)


# ---- 3. wide -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", WIDE, ids=[i for i in hs.STEP_IDS if i.startswith("guidw_")])
def test_wide_replay_equals_the_reference_at_every_step(gpu_device, path):
    z = load(path)
    assert len(WIDE) == 3
    before = form_count("sim_replay")
    x, case, step = every_step(z, gpu_device, wide=True)
    assert form_count("sim_replay") == before + 1
    assert torch.equal(x.cpu(), torch.from_numpy(z["x"][case, step].astype(np.float32)))


@functools.lru_cache(maxsize=None)
def open256_scene():
    """The wide-loop tests' largest canvas (256 x 256, five words a row, five agents): every agent has walked three cells along its
    border (or stood still) before the cell it is searched from."""
    m, pos, goal = hw.scene("open256")
    N = len(pos)
    table = np.zeros((1, 4, N, 2), dtype=np.int64)
    step = np.array([(0, 1), (1, 0), (0, 1), (0, 1), (0, 0)])
    for t in range(4):
        table[0, t] = pos - (3 - t) * step * np.where(pos == 0, -1, 1)
    assert (table >= 0).all() and (table < 256).all() and (table[0, 3] == pos).all() and (m[table[0, ..., 0], table[0, ..., 1]] == 0).all()
    want = sr.replayed_states(m, pos, goal, sr.table_cells(table[0], 3), "SemiLG_SD")
    return m, pos, goal, table, want


def test_wide_replay_on_the_largest_canvas_equals_the_restatement(gpu_device):
    from magat_pathplanning_amd import replayed_semi_states
    m, pos, goal, table, want = open256_scene()
    hist = dict(case=i32([0], gpu_device), step=i32([3], gpu_device), table=i32(table, gpu_device))
    x = replayed_semi_states(dev(m, gpu_device), i32(pos[None], gpu_device), i32(goal[None], gpu_device), hist, FOV, "SemiLG_SD",
                             wide=True)
    bad = np.nonzero((x[0].cpu().numpy() != want.astype(np.float32)).any(axis=(1, 2, 3)))[0]
    assert bad.size == 0, "agents %s differ" % bad.tolist()


# ---- 4. expert_samples(replay=True) -------------------------------------------------------------------------------------------------------
def expert_pack(z, device):
    return dict(obstacle_map=dev(z["map"], device), paths=dev(z["paths"], device), lengths=dev(z["lengths"], device),
                goal=dev(z["goal"], device), makespan=dev(z["makespan"], device), T=int(z["makespan"].max()) + 1,
                comm_radius=float(z["commR"].reshape(-1)[0]), dynamic_commR=bool(z["dynamic_commR"].reshape(-1)[0]),
                symmetric_norm=bool(z["symmetric_norm"].reshape(-1)[0]), guidance=str(z["guidance"].reshape(-1)[0]))


@functools.lru_cache(maxsize=None)
def carried_samples():
    """expert_samples of the SemiLG expert fixture on the carried-view route (replay=False): computed once, never written to."""
    from magat_pathplanning_amd import expert_samples, flatten_samples
    z = np.load(hs.EXPERT, allow_pickle=False)
    s = expert_samples(**expert_pack(z, torch.device("cuda:0")))
    return z, s, flatten_samples(s)


@pytest.mark.parametrize("max_agent_steps", [None, 2 * 20 * 12], ids=["one_chunk", "three_chunks"])
def test_expert_samples_replay_equals_the_carried_route_and_the_fixture(gpu_device, max_agent_steps):
    from magat_pathplanning_amd import expert_samples
    z, ref, _ = carried_samples()
    kw = {} if max_agent_steps is None else dict(max_agent_steps=max_agent_steps)
    chunks = 1 if max_agent_steps is None else 3          # 5 cases, two a chunk
    before = form_count("sim_replay"), form_count("sim_guided")
    s = expert_samples(replay=True, **dict(expert_pack(z, gpu_device), **kw))
    assert (form_count("sim_replay"), form_count("sim_guided")) == (before[0] + chunks, before[1])
    assert torch.equal(s["inputTensor"].cpu(), torch.from_numpy(z["x"].astype(np.float32)))
    assert sorted(s) == sorted(ref)
    for key in ref:
        assert s[key].dtype == ref[key].dtype and torch.equal(s[key], ref[key]), key


def test_replay_keyword_has_no_effect_on_other_guidances(gpu_device):
    from magat_pathplanning_amd import expert_samples
    z, _, _ = carried_samples()
    p = dict(expert_pack(z, gpu_device), guidance="GlobalG_SD")
    before = form_count("sim_replay")
    a, b = expert_samples(**p), expert_samples(replay=True, **p)
    assert form_count("sim_replay") == before
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ---- 5. ExpertMemory(replay=True) ---------------------------------------------------------------------------------------------------------
def replay_memory(z, device, **kw):
    from magat_pathplanning_amd import ExpertMemory
    N, (H, W) = z["pos"].shape[2], z["map"].shape[-2:]
    p = expert_pack(z, device)
    mem = ExpertMemory(6, N, H, W, int(z["lengths"].max()) + 3, comm_radius=p["comm_radius"], dynamic_commR=p["dynamic_commR"],
                       symmetric_norm=p["symmetric_norm"], guidance=p["guidance"], replay=True, device=device, **kw)
    return mem, {k: p[k] for k in ("obstacle_map", "paths", "lengths", "goal", "makespan", "T")}


def assert_rows(b, ref, idx, what):
    for key in SAMPLE_KEYS:
        want = ref[key].index_select(0, idx)
        got = b[key].to(torch.int64) if key in ("case", "step") else b[key]
        assert got.dtype == want.dtype and torch.equal(got, want), "%s: %s" % (what, key)


def test_memory_refuses_semilg_without_the_keyword(gpu_device):
    from magat_pathplanning_amd import ExpertMemory
    with pytest.raises(ValueError, match="expert_samples"):
        ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance="SemiLG_S", device=gpu_device)


def test_replay_memory_minibatch_equals_flattened_expert_samples(gpu_device):
    z, _, ref = carried_samples()
    mem, p = replay_memory(z, gpu_device)
    total = int(z["valid"].sum())
    assert mem.append(**p) == total == len(mem)
    every = torch.arange(total, device=gpu_device)
    before = form_count("sim_replay"), form_count("sim_guided"), form_count("sim_expert")
    b = mem.minibatch(indices=every)
    assert (form_count("sim_replay"), form_count("sim_guided"), form_count("sim_expert")) == (before[0] + 1, before[1], before[2] + 1)
    assert_rows(b, ref, every, "in order")
    assert torch.equal(b["inputTensor"].cpu(), torch.from_numpy(z["x"][z["valid"].astype(bool)].astype(np.float32)))
    some = torch.randint(total, (total + 9,), generator=torch.Generator().manual_seed(5)).to(gpu_device)
    assert some.unique().numel() < some.numel()
    assert_rows(mem.minibatch(indices=some), ref, some, "shuffled with repeats")
    # sample 0 of a case: a view of its own window only - the states of a fresh view at the start cells
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    firsts = torch.cat([torch.zeros(1, dtype=torch.int64, device=gpu_device), mem.cum[:4]])
    f = mem.minibatch(indices=firsts)
    assert f["step"].tolist() == [0] * 5
    fresh = batched_fov_states(f["map"], f["pos"], f["goal"], FOV, mem.guidance, new_agent_view(5, 12, 10, 10, FOV, gpu_device))
    assert torch.equal(f["inputTensor"], fresh)
    # a sample behind an agent's path length: that agent stands on its goal (the goal rule), and the row equals the reference's
    last = mem.minibatch(indices=mem.cum[:5] - 1)
    behind = last["step"][:, None] >= mem.lengths[:5]
    assert bool(behind.any()) and torch.equal(last["pos"][behind], last["goal"][behind])
    assert_rows(last, ref, mem.cum[:5] - 1, "last steps")
    mem.check()
    # an out-of-range index is clamped to a real sample, and check() raises
    from magat_pathplanning_amd import _native as nat
    odd = torch.tensor([3, total, -1], device=gpu_device)
    c = mem.minibatch(indices=odd)
    assert_rows(c, ref, torch.tensor([3, total - 1, 0], device=gpu_device), "clamped")
    with pytest.raises(nat.MagatNativeError, match="row 1 "):
        mem.check()


def test_replay_memory_on_a_shared_map(gpu_device):
    """The fixture's cases have a map each; a shared-map memory holds the cases of ONE map: case 2, appended twice."""
    z, _, ref = carried_samples()
    one = dev(z["map"][2], gpu_device)
    mem, p = replay_memory(z, gpu_device, shared_map=one)
    sel = {k: (v[[2, 2]].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
    steps = int(z["makespan"][2]) + 1
    assert mem.append(**dict(sel, obstacle_map=None)) == 2 * steps and mem.maps is None
    b = mem.minibatch(indices=torch.arange(2 * steps, device=gpu_device).flip(0).contiguous())
    first = int(z["valid"][:2].sum())                     # case 2's rows of the flattened reference
    want = ref["inputTensor"][first:first + steps].flip(0)
    assert b["map"].dim() == 2 and torch.equal(b["inputTensor"], torch.cat([want, want]))


def test_replay_memory_out_reuse_and_graph_capture(gpu_device):
    from magat_pathplanning_amd.memory import PICK_KEYS
    z, _, ref = carried_samples()
    mem, p = replay_memory(z, gpu_device)
    mem.append(**p)
    total = len(mem)
    idx = torch.arange(8, device=gpu_device)
    b = mem.minibatch(indices=idx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mem.minibatch(indices=idx, out=b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mem.minibatch(indices=idx, out=b)
    for key in PICK_KEYS:
        assert out[key].data_ptr() == b[key].data_ptr(), key                # nothing new for the pick's outputs
    new = torch.tensor([total - 1, 0, 17, 17, 3, total - 2, 9, 1], device=gpu_device)
    idx.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    assert_rows(out, ref, new, "replayed graph")
    mem.check()


def test_online_expert_appends_to_a_replay_memory(gpu_device):
    """The online-expert test's cases with a SemiLG memory: the re-solved cases start with an empty view at the agents' current
    cells, so their first samples equal the states of a fresh view there, and every sample equals expert_samples of the stored
    schedules."""
    import test_host_memory as hm
    from magat_pathplanning_amd import (BatchedEpisode, ExpertMemory, batched_fov_states, expert_samples, flatten_samples,
                                        generate_cases, new_agent_view, online_expert)
    k = hm.ONLINE
    want = hm.online_cases()
    cases = generate_cases(k["C"], k["H"], k["W"], k["N"], seed=k["seed"], device=gpu_device)
    goal = dev(want["goal"], gpu_device)
    stop = torch.full((k["C"], k["N"]), 4, dtype=torch.int32, device=gpu_device)
    mem = ExpertMemory(16, k["N"], k["H"], k["W"], 44, comm_radius=7.0, guidance="SemiLG_SD", replay=True, device=gpu_device)
    ep = BatchedEpisode(cases["map"], cases["start"], goal, k["maxstep"], comm_radius=7.0)
    for _ in range(k["maxstep"]):
        ep.step(actions=stop)
    got = online_expert(ep, mem)
    F = got["added_cases"]
    assert F == mem.cases > 0 and len(mem) == got["added_samples"]
    b = mem.minibatch(indices=torch.arange(len(mem), device=gpu_device))
    cells = mem.cells[:F].cpu().to(torch.int32).to(gpu_device)
    s = expert_samples(mem.maps[:F], torch.stack([cells >> 8, cells & 255], dim=3), mem.lengths[:F], mem.goal[:F], mem.makespan[:F],
                       7.0, guidance="SemiLG_SD")
    assert_rows(b, flatten_samples(s), torch.arange(len(mem), device=gpu_device), "online expert")
    firsts = torch.cat([torch.zeros(1, dtype=torch.int64, device=gpu_device), mem.cum[:F - 1]])
    f = mem.minibatch(indices=firsts)
    fresh = batched_fov_states(f["map"], f["pos"], f["goal"], FOV, "SemiLG_SD", new_agent_view(F, k["N"], k["H"], k["W"], FOV, gpu_device))
    assert f["step"].tolist() == [0] * F and torch.equal(f["inputTensor"], fresh)
    mem.check()


# ---- 6. rule edges through the public function -------------------------------------------------------------------------------------------
def test_rule_edges_equal_the_restatement(gpu_device):
    from magat_pathplanning_amd import replayed_semi_states
    m0, t0, g0 = hs.synthetic(17, 23, 6, 9, seed=1)
    m1, t1, g1 = hs.synthetic(17, 23, 6, 9, seed=2)
    t0[0, 3, 2] = (-1, 5)                                 # a step off the map (above it) ...
    t0[0, 5, 4] = (8, 23)                                 # ... and one to its right: they contribute nothing
    table = np.concatenate([t0, t1])
    maps, goals = np.stack([m0, m1]), np.stack([g0, g1])
    case, step = np.array([0, 1, 0, 1, 0]), np.array([8, 2, 8, 7, 4])      # (0, 8) twice; both cases, different steps
    pos = table[case, step]
    hist = dict(case=i32(case, gpu_device), step=i32(step, gpu_device), table=i32(table, gpu_device))
    x = replayed_semi_states(dev(maps[case], gpu_device), i32(pos, gpu_device), i32(goals[case], gpu_device), hist, FOV, "SemiLG_S")
    for i, (c, t) in enumerate(zip(case, step)):
        want = sr.replayed_states(maps[c], pos[i], goals[c], sr.table_cells(table[c], t), "SemiLG_S")
        assert np.array_equal(x[i].cpu().numpy(), want.astype(np.float32)), (c, t)
    assert torch.equal(x[0], x[2])
    # the store as the history of the same rows: the same tensors
    Lcap = 12
    paths = np.transpose(table, (0, 2, 1, 3)).copy()
    paths[0, 2, 3], paths[0, 4, 5] = paths[0, 2, 2], paths[0, 4, 4]      # (a stored cell cannot lie off the map)
    lengths = np.full((2, 6), 9)
    packed = np.stack([sr.pack_cells(paths[c], lengths[c], Lcap) for c in range(2)])
    last = paths[:, :, -1]                                # behind its length an agent stands on the store's goal: use the last cell
    store = dict(case=hist["case"], step=hist["step"], cells=dev(packed, gpu_device), lengths=i32(lengths, gpu_device),
                 goal=i32(last, gpu_device))
    rows = [1, 3]                                         # case 1 holds no off-map step: table and store agree
    y = replayed_semi_states(dev(maps[case], gpu_device), i32(pos, gpu_device), i32(goals[case], gpu_device), store, FOV, "SemiLG_S")
    assert torch.equal(y[rows], x[rows])
