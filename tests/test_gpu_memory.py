"""GPU: the device-resident training set and the online-expert harvest (magat_pathplanning_amd/memory.py; magat_sim_expert_pick
in csrc/sim_expert.hip).  A minibatch is compared with what existed before it - the same rows of flatten_samples(expert_samples(
...)) on the expert_* fixtures made by the real reference - with torch.equal: the same kernels run on the same rows, so no
tolerance applies.  Index mapping, decode and clamp are compared with tests/memory_restatement.py.  Shapes are the fixtures' and a
hand-made store of cases one step long; the inputs of the online-expert test come from tests/test_host_memory.py, which checks on
the CPU that ECBS's restatement solves every case the episode fails at."""
import functools

import numpy as np
import pytest
import torch

import memory_restatement as mr
import test_host_memory as hm

pytestmark = pytest.mark.gpu

FIXTURES = hm.FIXTURES
IDS = hm.IDS
SAMPLE_KEYS = ("inputTensor", "target", "GSO", "pos", "case", "step")
STORE_KEYS = ("_cells", "lengths", "goal", "makespan", "radii", "cum", "maps")


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def scalar(z, key):
    return z[key].reshape(-1)[0]


def form_count(form="sim_expert"):
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS[form]))


def settings(z):
    return dict(comm_radius=float(scalar(z, "commR")), dynamic_commR=bool(scalar(z, "dynamic_commR")),
                symmetric_norm=bool(scalar(z, "symmetric_norm")), guidance=str(scalar(z, "guidance")))


def pack(z, sel, device, Lmax=None):
    """The cases `sel` of a fixture as append's arguments, paths cut to Lmax (default: the longest path of these cases)."""
    sel = list(sel)
    Lmax = int(z["lengths"][sel].max()) if Lmax is None else Lmax
    return dict(obstacle_map=dev(z["map"][sel], device), paths=dev(z["paths"][sel][:, :, :Lmax], device),
                lengths=dev(z["lengths"][sel], device), goal=dev(z["goal"][sel], device), makespan=dev(z["makespan"][sel], device),
                T=int(z["makespan"][sel].max()) + 1)


def new_memory(z, device, capacity=6, slack=3, **kw):
    from magat_pathplanning_amd import ExpertMemory
    C, T, N = z["pos"].shape[:3]
    H, W = z["map"].shape[-2:]
    return ExpertMemory(capacity, N, H, W, int(z["lengths"].max()) + slack, device=device, **dict(settings(z), **kw))


@functools.lru_cache(maxsize=None)
def reference(path, gso_dtype=torch.float32):
    """flatten_samples(expert_samples(...)) of a fixture's five cases: computed once, shared, never written to."""
    from magat_pathplanning_amd import expert_samples, flatten_samples
    z = np.load(path, allow_pickle=False)
    device = torch.device("cuda:0")
    s = expert_samples(gso_dtype=gso_dtype, **dict(pack(z, range(5), device), **settings(z)))
    flat = flatten_samples(s)
    flat["radii"] = s["radii"]
    return flat


def assert_rows(b, ref, idx, what):
    for key in SAMPLE_KEYS:
        want = ref[key].index_select(0, idx)
        got = b[key].to(torch.int64) if key in ("case", "step") else b[key]
        assert got.dtype == want.dtype and torch.equal(got, want), "%s: %s" % (what, key)
    assert b["action"].dtype == torch.int64 and torch.equal(b["action"], b["target"].argmax(-1)), what
    assert b["case"].dtype == torch.int32 and b["step"].dtype == torch.int32 and b["pos"].dtype == torch.int32


def store_state(mem):
    out = {key: getattr(mem, key).clone() for key in STORE_KEYS if getattr(mem, key) is not None}
    out["flag"] = mem.flag.clone()
    return out


def assert_same_store(a, b, cases):
    for key in STORE_KEYS:
        if getattr(a, key) is not None:
            assert torch.equal(getattr(a, key)[:cases], getattr(b, key)[:cases]), key


# ---- 1. equality with what exists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_minibatch_equals_flattened_expert_samples(gpu_device, path):
    z = np.load(path, allow_pickle=False)
    for gso_dtype in (torch.float32, torch.float64):
        ref = reference(path, gso_dtype)
        mem = new_memory(z, gpu_device, gso_dtype=gso_dtype)
        total = int(z["valid"].sum())
        assert mem.append(**pack(z, range(5), gpu_device)) == total
        assert len(mem) == total and mem.cases == 5
        assert mem.radii.dtype == torch.float64 and torch.equal(mem.radii[:5].cpu(), torch.from_numpy(z["radii"]))      # bit for bit
        assert mem.cells.dtype == torch.uint16 and mem.cum.dtype == torch.int64
        every = torch.arange(total, device=gpu_device)
        b = mem.minibatch(indices=every)
        assert b["GSO"].dtype == gso_dtype and tuple(b["inputTensor"].shape) == (total,) + z["x"].shape[2:]
        assert_rows(b, ref, every, "in order")
        if gso_dtype == torch.float64:
            continue
        # ... and the fixture itself, which the real reference made
        assert torch.equal(b["inputTensor"].cpu(), torch.from_numpy(z["x"][z["valid"].astype(bool)].astype(np.float32)))
        assert torch.equal(b["target"].cpu(), torch.from_numpy(z["target"][z["valid"].astype(bool)].astype(np.float32)))
        assert_rows(mem.minibatch(indices=every.flip(0).contiguous()), ref, every.flip(0), "reversed")
        g = torch.Generator().manual_seed(5)
        some = torch.randint(total, (total + 9,), generator=g).to(gpu_device)      # more draws than samples: some twice
        assert some.unique().numel() < some.numel()
        assert_rows(mem.minibatch(indices=some), ref, some, "shuffled with repeats")
        mem.check()


# ---- 2. appends ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES[:2], ids=IDS[:2])
def test_appends_one_by_one_equal_one_append(gpu_device, path):
    z = np.load(path, allow_pickle=False)
    assert len(set(int(z["lengths"][c].max()) for c in range(5))) >= 2      # the calls differ in Lmax
    whole = new_memory(z, gpu_device)
    whole.append(**pack(z, range(5), gpu_device))
    parts = new_memory(z, gpu_device)
    for c in range(5):
        p = pack(z, [c], gpu_device)
        p.pop("T")                                                           # (read from the device)
        parts.append(**p)
    assert len(parts) == len(whole) and parts.cases == 5
    assert_same_store(whole, parts, 5)
    every = torch.arange(len(whole), device=gpu_device)
    a, b = whole.minibatch(indices=every), parts.minibatch(indices=every)
    for key in SAMPLE_KEYS + ("action", "goal", "radii", "map"):
        assert torch.equal(a[key], b[key]), key


def test_shared_map_memory_equals_per_case_copies(gpu_device):
    z = np.load([p for p in FIXTURES if "ProjectG" in p][0], allow_pickle=False)
    one = dev(z["map"][0], gpu_device)
    p = pack(z, range(5), gpu_device)
    shared = new_memory(z, gpu_device, shared_map=one)
    assert shared.maps is None
    shared.append(**dict(p, obstacle_map=None))
    copies = new_memory(z, gpu_device)
    copies.append(**dict(p, obstacle_map=one.unsqueeze(0).repeat(5, 1, 1)))
    every = torch.arange(len(shared), device=gpu_device)
    a, b = shared.minibatch(indices=every), copies.minibatch(indices=every)
    for key in SAMPLE_KEYS + ("action", "goal", "radii"):
        assert torch.equal(a[key], b[key]), key
    assert a["map"].dim() == 2 and tuple(b["map"].shape) == (len(shared),) + tuple(one.shape)
    assert bool((b["map"] == one).all())


def test_refused_appends_change_nothing(gpu_device):
    from magat_pathplanning_amd import _native as nat
    z = np.load([p for p in FIXTURES if "LocalG_SD" in p][0], allow_pickle=False)
    N = z["pos"].shape[2]
    longest = int(z["lengths"].max(axis=1).argmax())
    short = [c for c in range(5) if c != longest]
    assert int(z["lengths"][short].max()) < int(z["lengths"][longest].max())
    mem = new_memory(z, gpu_device, capacity=5, slack=int(z["lengths"][short].max()) - int(z["lengths"].max()))      # room for `short` only
    mem.append(**pack(z, short, gpu_device))
    every = torch.arange(len(mem), device=gpu_device)
    before, size = store_state(mem), (len(mem), mem.cases)
    batch = mem.minibatch(indices=every)
    one, two = pack(z, short[:1], gpu_device), pack(z, short[:2], gpu_device)
    n = int(z["lengths"][short[0]].argmax())
    assert int(z["lengths"][short[0], n]) >= 2
    bad_move = dict(one, paths=one["paths"].clone())
    first = bad_move["paths"][0, n, 0]
    bad_move["paths"][0, n, 1] = torch.where(first >= 2, first - 2, first + 2)      # a jump of (2, 2) that stays on the map
    shared = new_memory(z, gpu_device, shared_map=dev(z["map"][0], gpu_device))
    refused = [
        (mem, two, nat.MagatNativeError, "do not fit"),                                                      # 4 + 2 > 5
        (mem, pack(z, [longest], gpu_device), nat.MagatNativeError, "cells"),                               # a path longer than max_length
        (mem, {k: (v[:, :N - 1].contiguous() if k in ("paths", "lengths", "goal") else v) for k, v in one.items()},
         nat.MagatNativeError, "paths must be"),                                                             # another N
        (mem, dict(one, obstacle_map=one["obstacle_map"][:, :-1].contiguous()), nat.MagatNativeError, "maps must be"),      # another H
        (mem, dict(one, obstacle_map=one["obstacle_map"][:, :, :-1].contiguous()), nat.MagatNativeError, "maps must be"),   # another W
        (mem, dict(one, obstacle_map=one["obstacle_map"][0]), nat.MagatNativeError, "shared map is refused"),
        (shared, one, nat.MagatNativeError, "per-case maps are refused"),
        (mem, dict(one, paths=one["paths"].cpu()), nat.MagatNativeError, "device tensor"),
        (mem, dict(one, obstacle_map=one["obstacle_map"].cpu()), nat.MagatNativeError, "device tensor"),
        (mem, bad_move, ValueError, "case 0 step 0 agent %d " % n),
    ]
    for target, args, error, text in refused:
        with pytest.raises(error, match=text):
            target.append(**args)
    assert (len(mem), mem.cases) == size and (len(shared), shared.cases) == (0, 0)
    after = store_state(mem)
    for key, value in before.items():
        assert torch.equal(after[key], value), key
    again = mem.minibatch(indices=every)
    for key in SAMPLE_KEYS + ("action", "goal", "radii", "map"):
        assert torch.equal(again[key], batch[key]), key
    mem.append(**one)                                                        # and there is still room for one case
    assert mem.cases == 5


# ---- 3. indices ---------------------------------------------------------------------------------------------------------------------
def one_step_memory(device, capacity=6, **kw):
    from magat_pathplanning_amd import ExpertMemory
    raw, store = mr.one_step_store()
    mem = ExpertMemory(capacity, 2, 12, 12, store["cells"].shape[2], comm_radius=7.0, device=device, **kw)
    mem.append(dev(raw["maps"], device), dev(raw["paths"], device), dev(raw["lengths"], device), dev(raw["goal"], device),
               dev(raw["makespan"], device))
    return mem, raw, store


def assert_equals_restatement(b, want):
    for key in ("case", "step", "pos", "target", "action", "goal"):
        assert torch.equal(b[key].cpu(), torch.from_numpy(want[key])), key


def test_every_sample_and_case_boundary_equals_the_restatement(gpu_device):
    from magat_pathplanning_amd import _native as nat
    mem, raw, store = one_step_memory(gpu_device)
    assert len(mem) == 17 and mem.cases == 6 and mem.cum[:6].cpu().tolist() == store["cum"].tolist()
    assert torch.equal(mem.cells[:6].cpu().to(torch.int32), torch.from_numpy(store["cells"].astype(np.int32)))
    b = mem.minibatch(indices=torch.arange(17, device=gpu_device))
    want = mr.pick(store, list(range(17)))
    assert_equals_restatement(b, want)
    assert want["case"].tolist() == [0, 1, 1, 1, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5]
    for m in (0, 5, 6):                                                     # the one-step cases: everybody on its goal, stopping
        assert torch.equal(b["pos"][m], b["goal"][m]) and b["action"][m].tolist() == [4, 4]
    mem.check()                                                             # a clean memory
    idx = [3, 17, 2, -1, 16, 1 << 40]
    b = mem.minibatch(indices=torch.tensor(idx, device=gpu_device))
    want = mr.pick(store, idx)
    assert want["flag"] == 1 and want["case"].tolist() == [1, 5, 1, 0, 5, 5]
    assert_equals_restatement(b, want)                                      # clamped rows are real samples
    assert bool(torch.isfinite(b["inputTensor"]).all()) and bool(torch.isfinite(b["GSO"]).all())
    with pytest.raises(nat.MagatNativeError, match="row 1 "):
        mem.check()
    mem.minibatch(indices=torch.tensor([-1], device=gpu_device))
    with pytest.raises(nat.MagatNativeError, match="row 0 "):              # the smallest row so far; the flag is sticky
        mem.check()
    with pytest.raises(ValueError, match="empty"):
        from magat_pathplanning_amd import ExpertMemory
        ExpertMemory(2, 2, 12, 12, 4, comm_radius=7.0, device=gpu_device).minibatch(4)


# ---- 4. draws -----------------------------------------------------------------------------------------------------------------------
def test_seeded_draws_repeat_and_an_epoch_is_a_permutation(gpu_device):
    mem, raw, store = one_step_memory(gpu_device, capacity=8)
    sel = [1, 5]
    mem.append(*[dev(raw[key][sel], gpu_device) for key in ("maps", "paths", "lengths", "goal", "makespan")])
    assert len(mem) == 23 and mem.cases == 8
    g = torch.Generator(device=gpu_device)
    batches = []
    for _ in range(2):
        g.manual_seed(1234)
        batches.append(mem.minibatch(9, generator=g))
    for key in SAMPLE_KEYS + ("indices",):
        assert torch.equal(batches[0][key], batches[1][key]), key
    assert tuple(batches[0]["inputTensor"].shape) == (9, 2, 3, 11, 11)
    idx = batches[0]["indices"]
    assert idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < 23
    assert not torch.equal(mem.minibatch(9, generator=g)["indices"], idx)      # the generator moves on
    g.manual_seed(7)
    seen = [b for b in mem.epoch(7, generator=g)]
    assert [b["indices"].numel() for b in seen] == [7, 7, 7, 2]
    assert sorted(torch.cat([b["indices"] for b in seen]).tolist()) == list(range(23))
    both = mr.concat_stores([store, {k: (v[sel] if v is not None else None) for k, v in store.items()}])
    for b in seen:
        assert_equals_restatement(b, mr.pick(both, b["indices"].tolist()))
    g.manual_seed(7)
    dropped = [b["indices"] for b in mem.epoch(7, generator=g, drop_last=True)]
    assert len(dropped) == 3 and all(torch.equal(a, b["indices"]) for a, b in zip(dropped, seen))
    mem.check()


# ---- 5. launches and capture ------------------------------------------------------------------------------------------------------------
def test_one_counted_launch_and_graph_capture(gpu_device, tag_counts):
    z = np.load([p for p in FIXTURES if "LocalG_SD" in p][0], allow_pickle=False)
    mem = new_memory(z, gpu_device)
    mem.append(**pack(z, range(5), gpu_device))
    total = len(mem)
    idx = torch.arange(8, device=gpu_device)
    keep, before_idx = store_state(mem), idx.clone()
    before = form_count()
    with tag_counts() as tc:
        b = mem.minibatch(indices=idx)
    assert form_count() == before + 1 and tc["sim_expert"] == 1
    after = store_state(mem)
    for key, value in keep.items():                                         # the store and the indices are inputs
        assert torch.equal(after[key], value), key
    assert torch.equal(idx, before_idx)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        mem.minibatch(indices=idx, out=b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mem.minibatch(indices=idx, out=b)
    for key in hm_pick_keys(mem):
        assert out[key].data_ptr() == b[key].data_ptr(), key                # nothing new for the pick's outputs
    assert total > 17
    new = torch.tensor([total - 1, 0, 17, 17, 3, total - 2, 9, 1], device=gpu_device)
    idx.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = mem.minibatch(indices=new)
    for key in SAMPLE_KEYS + ("action", "goal", "radii", "map"):
        assert torch.equal(out[key], eager[key]), key
    assert not torch.equal(eager["case"], torch.zeros_like(eager["case"]))
    with pytest.raises(ValueError, match="same M"):
        mem.minibatch(indices=torch.arange(5, device=gpu_device), out=b)
    mem.check()


def hm_pick_keys(mem):
    from magat_pathplanning_amd.memory import PICK_KEYS
    return [key for key in PICK_KEYS if key != "map" or mem.maps is not None]


# ---- 6. training ----------------------------------------------------------------------------------------------------------------------
def test_two_optimiser_steps_on_minibatches(gpu_device):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import make_config
    from oracle import magat_oracle as orc
    z = np.load([p for p in FIXTURES if "LocalG_SD" in p][0], allow_pickle=False)
    N = z["pos"].shape[2]
    mem = new_memory(z, gpu_device)
    mem.append(**pack(z, range(5), gpu_device))
    cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=1, device=str(gpu_device))
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(orc.init_state_dict(cfg, seed=5))
    net = net.to(gpu_device).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    g = torch.Generator(device=gpu_device).manual_seed(3)
    first = {k: v.detach().clone() for k, v in net.named_parameters()}
    for _ in range(2):
        b = mem.minibatch(8, generator=g)
        net.addGSO(b["GSO"])
        pred = net(b["inputTensor"])
        pred = pred if isinstance(pred, torch.Tensor) else torch.stack(list(pred), dim=1)
        loss = torch.nn.CrossEntropyLoss()(pred.reshape(-1, 5), b["action"].reshape(-1))
        assert pred.reshape(-1, 5).shape[0] == 8 * N and bool(torch.isfinite(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert any(not torch.equal(v.detach(), first[k]) for k, v in net.named_parameters())
    assert all(bool(torch.isfinite(v).all()) for v in net.parameters())
    mem.check()


# ---- 7. the online expert ---------------------------------------------------------------------------------------------------------------
def test_online_expert_harvests_the_failed_cases(gpu_device):
    from magat_pathplanning_amd import BatchedEpisode, ExpertMemory, audit_schedules, generate_cases, online_expert
    k = hm.ONLINE
    want = hm.online_cases()
    cases = generate_cases(k["C"], k["H"], k["W"], k["N"], seed=k["seed"], device=gpu_device)
    assert cases["valid"].cpu().tolist() == [1] * k["C"]
    assert torch.equal(cases["map"].cpu(), torch.from_numpy(want["map"])) and torch.equal(cases["start"].cpu(), torch.from_numpy(want["start"]))
    goal = dev(want["goal"], gpu_device)
    stop = torch.full((k["C"], k["N"]), 4, dtype=torch.int32, device=gpu_device)
    mem = ExpertMemory(16, k["N"], k["H"], k["W"], 44, comm_radius=7.0, device=gpu_device)

    def run(goal_):
        ep = BatchedEpisode(cases["map"], cases["start"], goal_, k["maxstep"], comm_radius=7.0)
        for _ in range(k["maxstep"]):
            ep.step(actions=stop)
        return ep

    ep = BatchedEpisode(cases["map"], cases["start"], goal, k["maxstep"], comm_radius=7.0)
    ep.step(actions=stop)
    with pytest.raises(ValueError, match="maxstep"):                        # one step of three
        online_expert(ep, mem)
    ep = run(goal)
    assert torch.equal(ep.pos, cases["start"])                              # nobody moved
    off_goal = (ep.pos != ep.goal).any(dim=2).any(dim=1)
    got = online_expert(ep, mem)
    assert got["failed"].dtype == torch.bool and torch.equal(got["failed"], off_goal)
    assert got["failed"].cpu().tolist() == [c not in k["on_goal"] for c in range(k["C"])]
    F = int(off_goal.sum())
    assert tuple(got["solved"].shape) == (F,) and bool(got["solved"].all())      # (the condition checked in test_host_memory)
    assert got["added_cases"] == int(got["solved"].sum()) == F == mem.cases
    assert len(mem) == int((mem.makespan[:F] + 1).sum()) == got["added_samples"]
    f = torch.nonzero(off_goal).flatten()
    firsts = torch.cat([torch.zeros(1, dtype=torch.int64, device=gpu_device), mem.cum[:F - 1]])
    b = mem.minibatch(indices=firsts)
    assert b["step"].tolist() == [0] * F and b["case"].tolist() == list(range(F))
    assert torch.equal(b["pos"], ep.pos.index_select(0, f)) and torch.equal(b["goal"], ep.goal.index_select(0, f))
    assert torch.equal(b["map"], ep.map.index_select(0, f))
    # the stored schedules are valid schedules from the agents' positions to their goals
    cells = mem.cells[:F].cpu().to(torch.int32).to(gpu_device)
    sched = dict(paths=torch.stack([cells >> 8, cells & 255], dim=3), lengths=mem.lengths[:F], start=b["pos"], goal=mem.goal[:F])
    audit = audit_schedules(b["map"], sched)
    assert audit["status"].tolist() == [0] * F and torch.equal(audit["makespan"], mem.makespan[:F])
    last = mem.minibatch(indices=mem.cum[:F] - 1)
    assert torch.equal(last["step"], mem.makespan[:F]) and bool((last["target"].sum(-1) == 1).all())
    mem.check()
    # an episode with every agent on its goal: nothing is appended and no solver runs
    ep = run(cases["start"])
    size, counts = (len(mem), mem.cases), [form_count(form) for form in ("sim_mapf", "sim_mapf_ecbs", "sim_expert")]
    got = online_expert(ep, mem)
    assert not bool(got["failed"].any()) and got["solved"].numel() == 0 and got["added_cases"] == 0 and got["added_samples"] == 0
    assert (len(mem), mem.cases) == size and [form_count(form) for form in ("sim_mapf", "sim_mapf_ecbs", "sim_expert")] == counts
