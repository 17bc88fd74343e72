"""GPU: expert schedules -> training samples (csrc/sim_expert.hip through magat_pathplanning_amd/expert.py) against the expert_*
fixtures made by the real reference (tools/make_golden_expert.py).  Integer and float64 outputs are compared with torch.equal
(radii bit for bit); the GSO's non-zero pattern is equal and its values are within the tolerance of the sim_* GSO tests
(tests/test_gpu_sim.py: rtol 1e-9 for float64, 1e-6 for float32 - lambda_max is iterative).

Each fixture holds five cases of one configuration (one agent count, map size, guidance and radius rule: what ONE call takes;
the five fixtures differ in all of these and cannot share a call), with mixed step counts: the packed test runs each fixture's
five cases in one call (C = 5, mixed T) and one call per case."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_paths

pytestmark = pytest.mark.gpu

FIXTURES = golden_paths("expert_")
IDS = [os.path.basename(p)[7:-4] for p in FIXTURES]
STATS = (("expert_first_move", "first_move"), ("expert_end_step", "end_step"), ("makespanTarget", "makespanTarget"),
         ("flowtimeTarget", "flowtimeTarget"))


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def scalar(z, key):
    return z[key].reshape(-1)[0]


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_expert"]))


def run_fixture(z, device, cases=None, **kw):
    """expert_samples + expert_stats on the fixture's inputs (all cases, or the listed ones)."""
    from magat_pathplanning_amd import expert_samples, expert_stats
    sel = slice(None) if cases is None else list(cases)
    mk = z["makespan"][sel]
    Lmax = int(z["lengths"][sel].max())
    args = dict(obstacle_map=dev(z["map"][sel], device), paths=dev(z["paths"][sel][:, :, :Lmax], device),
                lengths=dev(z["lengths"][sel], device), goal=dev(z["goal"][sel], device), makespan=dev(mk, device),
                comm_radius=float(scalar(z, "commR")), dynamic_commR=bool(scalar(z, "dynamic_commR")),
                symmetric_norm=bool(scalar(z, "symmetric_norm")), guidance=str(scalar(z, "guidance")), T=int(mk.max()) + 1)
    args.update(kw)
    s = expert_samples(**args)
    st = expert_stats(s["target"], dev(z["start"][sel], device), args["goal"], s["valid"])
    return s, st


def check_case(z, c, s, st, i, gso_rtol):
    """Case c of the fixture against row i of the results, over the case's own T_c steps; everything behind them is zero."""
    Tc = int(z["makespan"][c]) + 1
    def eq(got, want, what):                   # same dtype, same shape (a per-case scalar as one element), same bits
        want = torch.from_numpy(np.atleast_1d(np.ascontiguousarray(want)))
        got = got.cpu().reshape(1) if got.dim() == 0 else got.cpu()
        assert got.dtype == want.dtype and torch.equal(got, want), "%s differs (case %d)" % (what, c)
    eq(s["pos"][i, :Tc], z["pos"][c, :Tc], "pos")
    eq(s["target"][i, :Tc], z["target"][c, :Tc].astype(np.float32), "target")
    eq(s["inputTensor"][i, :Tc], z["x"][c, :Tc].astype(np.float32), "inputTensor")
    assert s["valid"][i].cpu().tolist() == [1] * Tc + [0] * (s["valid"].shape[1] - Tc)
    for key in ("pos", "target", "inputTensor", "GSO"):
        assert not bool(s[key][i, Tc:].any()), "%s is not zero behind the last step (case %d)" % (key, c)
    eq(s["radii"][i], z["radii"][c], "radii")                                  # float64, bit for bit
    assert s["radii"].dtype == torch.float64 and int(s["grow_steps"][i]) == int(z["grow_steps"][c])
    assert int(s["makespan"][i]) == int(z["makespan"][c]) and int(s["bad"][i]) == -1
    S = s["GSO"][i, :Tc].cpu().numpy()
    np.testing.assert_array_equal(S != 0, z["GSO"][c, :Tc] != 0)
    np.testing.assert_allclose(S, z["GSO"][c, :Tc].astype(S.dtype), rtol=gso_rtol, atol=0)
    for ours, theirs in STATS:
        eq(st[ours][i], z[theirs][c], ours)
    eq(st["expert_pos"][i, :Tc + 1], z["expert_pos"][c, :Tc + 1], "expert_pos")
    assert bool((st["expert_pos"][i, Tc + 1:] == st["expert_pos"][i, Tc]).all())


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_samples_equal_reference_fixture_packed_and_one_by_one(gpu_device, path):
    z = np.load(path, allow_pickle=False)
    C = z["pos"].shape[0]
    assert C == 5 and len(set(z["makespan"].tolist())) >= 3                    # mixed T inside the pack
    for dtype, rtol in ((torch.float32, 1e-6), (torch.float64, 1e-9)):
        s, st = run_fixture(z, gpu_device, gso_dtype=dtype)
        assert s["GSO"].dtype == dtype and s["inputTensor"].dtype == torch.float32 and s["target"].dtype == torch.float32
        assert tuple(s["inputTensor"].shape) == z["x"].shape and s["pos"].dtype == torch.int32
        for c in range(C):
            check_case(z, c, s, st, c, rtol)
    # one call per case gives what the packed call gave (and the reference's, again)
    s64 = s                                                                    # the packed float64 run
    for c in range(C):
        s1, st1 = run_fixture(z, gpu_device, cases=[c], gso_dtype=torch.float64)
        check_case(z, c, s1, st1, 0, 1e-9)
        Tc = int(z["makespan"][c]) + 1
        assert s1["pos"].shape[1] == Tc
        assert torch.equal(s1["GSO"][0], s64["GSO"][c, :Tc]) and torch.equal(s1["inputTensor"][0], s64["inputTensor"][c, :Tc])


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_chunked_over_cases_is_the_same(gpu_device, path):
    """max_agent_steps small enough for chunks of two cases, and of one: bit-identical to the single chunk."""
    z = np.load(path, allow_pickle=False)
    C, T, N = z["pos"].shape[:3]
    whole, _ = run_fixture(z, gpu_device, gso_dtype=torch.float64)
    for limit in (2 * T * N, 1):
        part, _ = run_fixture(z, gpu_device, gso_dtype=torch.float64, max_agent_steps=limit)
        for key in ("inputTensor", "target", "GSO", "pos", "valid", "radii", "grow_steps"):
            assert torch.equal(whole[key], part[key]), key


def test_step_entries_one_by_one_and_without_T(gpu_device):
    """expert_schedule / expert_radius on their own; T read from the device when the caller does not pass it."""
    from magat_pathplanning_amd import expert_radius, expert_schedule
    z = np.load([p for p in FIXTURES if "ProjectG_dyn" in p][0], allow_pickle=False)
    a = [dev(z[k], gpu_device) for k in ("paths", "lengths", "goal", "makespan")]
    sch = expert_schedule(*a)
    assert tuple(sch["pos"].shape) == z["pos"].shape and torch.equal(sch["pos"].cpu(), torch.from_numpy(z["pos"]))
    assert torch.equal(sch["valid"].cpu(), torch.from_numpy(z["valid"])) and sch["bad"].cpu().tolist() == [-1] * 5
    radii, grow, step_grow = expert_radius(sch["pos"], sch["valid"], float(scalar(z, "commR")), return_step_grow=True)
    assert torch.equal(radii.cpu(), torch.from_numpy(z["radii"])) and grow.cpu().tolist() == z["grow_steps"].tolist()
    sg = step_grow.cpu()
    assert torch.equal(sg.max(dim=1).values.int(), grow.cpu()) and not bool(sg[~sch["valid"].bool().cpu()].any())
    # the transformer's rule is not the simulator's step-0 rule: a later step decides in at least one case
    assert bool((sg[:, 0] < grow.cpu()).any())
    # a longer T than needed only adds invalid rows
    longer = expert_schedule(*a, T=z["pos"].shape[1] + 3)
    assert torch.equal(longer["pos"][:, :z["pos"].shape[1]], sch["pos"]) and not bool(longer["valid"][:, -3:].any())
    assert not bool(longer["pos"][:, -3:].any()) and not bool(longer["target"][:, -3:].any())


def test_flattened_samples_train_the_planner(gpu_device):
    from magat_pathplanning_amd import DecentralPlannerGATNet, flatten_samples
    from magat_pathplanning_amd.synthetic import make_config
    from oracle import magat_oracle as orc
    z = np.load([p for p in FIXTURES if "LocalG_SD" in p][0], allow_pickle=False)
    s, _ = run_fixture(z, gpu_device)
    b = flatten_samples(s)
    M, N = int(z["valid"].sum()), z["pos"].shape[2]
    assert tuple(b["inputTensor"].shape) == (M, N, 3, 11, 11) and tuple(b["GSO"].shape) == (M, N, N)
    assert tuple(b["target"].shape) == (M, N, 5) and bool((b["target"].sum(-1) == 1).all())
    assert torch.equal(b["case"].cpu(), torch.from_numpy(np.repeat(np.arange(5), z["makespan"] + 1)))
    assert torch.equal(b["inputTensor"][0], s["inputTensor"][0, 0]) and torch.equal(b["GSO"][-1], s["GSO"][4, int(z["makespan"][4])])
    cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=1, device=str(gpu_device))
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(orc.init_state_dict(cfg, seed=5))
    net = net.to(gpu_device).eval()
    with torch.no_grad():
        net.addGSO(b["GSO"][:16])
        pred = net(b["inputTensor"][:16])
    pred = pred if isinstance(pred, torch.Tensor) else torch.stack(list(pred), dim=1)
    loss = torch.nn.CrossEntropyLoss()(pred.reshape(-1, 5), b["target"][:16].argmax(-1).reshape(-1))
    assert pred.reshape(-1, 5).shape[0] == 16 * N and bool(torch.isfinite(loss))


def test_each_entry_is_one_counted_launch(gpu_device, tag_counts):
    from magat_pathplanning_amd import expert_radius, expert_schedule, expert_stats
    z = np.load([p for p in FIXTURES if "idle" in p][0], allow_pickle=False)
    a = [dev(z[k], gpu_device) for k in ("paths", "lengths", "goal", "makespan")]
    T = z["pos"].shape[1]
    before = form_count()
    with tag_counts() as tc:
        sch = expert_schedule(*a, T=T)
        assert form_count() == before + 1
        expert_radius(sch["pos"], sch["valid"], 4.0)
        assert form_count() == before + 2
        expert_stats(sch["target"], dev(z["start"], gpu_device), a[2], sch["valid"])
        assert form_count() == before + 3
    assert tc["sim_expert"] == 3


def test_two_cell_jump_sets_bad_and_corrupts_nothing_else(gpu_device):
    from magat_pathplanning_amd import expert_samples, expert_schedule
    z = np.load([p for p in FIXTURES if "LocalG_SD" in p][0], allow_pickle=False)
    paths = z["paths"].copy()
    c = 2
    n = int(z["lengths"][c].argmax())                        # the agent with the longest path
    L = int(z["lengths"][c, n])
    assert L >= 6
    t = 3
    paths[c, n, t + 1:L] = paths[c, n, t + 2:L].tolist() + [paths[c, n, L - 1].tolist()]      # drop one cell: a jump at step t
    d = np.abs(paths[c, n, t + 1] - paths[c, n, t]).sum()
    if d <= 1:                                                   # (a wait was dropped, or one followed: no jump yet)
        paths[c, n, t + 1:] += np.array([2, 2], dtype=np.int32)  # the shift begins at cell t + 1: a move of (>= 1, >= 1) at step t
    assert np.abs(paths[c, n, t + 1] - paths[c, n, t]).sum() >= 2 and np.array_equal(paths[c, n, :t + 1], z["paths"][c, n, :t + 1])
    a = [dev(paths, gpu_device)] + [dev(z[k], gpu_device) for k in ("lengths", "goal", "makespan")]
    T, N = z["pos"].shape[1], z["pos"].shape[2]
    sch = expert_schedule(*a, T=T)
    bad = sch["bad"].cpu().tolist()
    # steps before t are the fixture's and no other agent changed: the first illegal (t, n) is exactly this one
    assert bad[c] == t * N + n and [v for i, v in enumerate(bad) if i != c] == [-1] * 4
    tb, nb = t, n
    assert not bool(sch["target"][c, tb, nb].any())                         # that sample's target row is zero
    # every other case is what the reference gave, and so are the other agents of the case itself
    others = [i for i in range(5) if i != c]
    assert torch.equal(sch["pos"][others].cpu(), torch.from_numpy(z["pos"][others]))
    assert torch.equal(sch["target"][others].cpu(), torch.from_numpy(z["target"][others].astype(np.float32)))
    keep = [i for i in range(N) if i != n]
    assert torch.equal(sch["pos"][c][:, keep].cpu(), torch.from_numpy(z["pos"][c][:, keep]))
    assert torch.equal(sch["target"][c][:, keep].cpu(), torch.from_numpy(z["target"][c][:, keep].astype(np.float32)))
    assert torch.equal(sch["valid"].cpu(), torch.from_numpy(z["valid"]))
    with pytest.raises(ValueError, match="case %d step %d agent %d" % (c, tb, nb)):
        expert_schedule(*a, T=T, check=True)
    with pytest.raises(ValueError, match="case %d" % c):
        expert_samples(dev(z["map"], gpu_device), *a, comm_radius=7.0, guidance="LocalG_SD", T=T)


def test_cpu_tensor_raises(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import expert_samples, expert_stats
    z = np.load([p for p in FIXTURES if "idle" in p][0], allow_pickle=False)
    a = [dev(z[k], gpu_device) for k in ("paths", "lengths", "goal", "makespan")]
    with pytest.raises(nat.MagatNativeError):
        expert_samples(dev(z["map"], gpu_device), a[0].cpu(), *a[1:], comm_radius=4.0)
    with pytest.raises(nat.MagatNativeError):
        expert_samples(torch.from_numpy(z["map"]), *a, comm_radius=4.0)
    with pytest.raises(nat.MagatNativeError):
        expert_stats(torch.from_numpy(z["target"].astype(np.float32)), dev(z["start"], gpu_device), a[2], dev(z["valid"], gpu_device))


def test_graph_that_cannot_connect_reports_minus_one_and_samples_raise(gpu_device):
    """Two agents 1000 cells apart, radius 1, four growth steps: 1.1^4 is far from 1000."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import expert_radius, expert_samples, pack_schedules
    pk = pack_schedules([[[(0, 0), (0, 1)], [(5, 5)]], [[(0, 0), (0, 1)], [(0, 1000)]]],
                        [[(0, 1), (5, 5)], [(0, 1), (0, 1000)]], device=gpu_device)
    pos = torch.stack([pk["paths"][:, :, 0], pk["paths"][:, :, 1]], dim=1).contiguous()      # (C,T,N,2): both paths are padded
    valid = torch.ones(2, 2, dtype=torch.uint8, device=gpu_device)
    radii, grow = expert_radius(pos, valid, 1.0, max_steps=4)
    assert grow.cpu().tolist()[1] == -1 and float(radii[1]) == 1.0 * 1.1 * 1.1 * 1.1 * 1.1
    radii, grow = expert_radius(pos, valid, 1.0, max_steps=64)
    k = int(grow[0])
    r = 1.0
    for _ in range(k):
        r = r * 1.1
    assert k >= 1 and float(radii[0]) == r and r > 5 * 2 ** 0.5 - 1
    m = torch.zeros(8, 8, dtype=torch.uint8, device=gpu_device)
    with pytest.raises(nat.MagatNativeError, match="disconnected"):
        expert_samples(m, comm_radius=1.0, dynamic_commR=True, max_steps=4, **pk)
