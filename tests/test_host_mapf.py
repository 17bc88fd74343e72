"""CPU-only: the host side of the path-finding expert (csrc/sim_mapf.hip, magat_pathplanning_amd/mapf.py) - header / loader /
build list / argument checks - and the restatement that the GPU tests compare the kernel with (tests/mapf_restatement.py):
hand cases with known answers, arrival times against an exhaustive search written over paths instead of boards, and
check_schedule on schedules with planted faults."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mapf_restatement as mr
from conftest import ROOT

ENTRIES = ("magat_sim_mapf_workspace_bytes", "magat_sim_mapf_plan")
HAND = mr.hand_cases()
SEED_10x10 = 7      # the 10 x 10 batch of the GPU tests: every case solved within the retries (asserted below)


def test_mapf_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "sim_mapf.hip" in build_native.SOURCES
    assert re.search(r"size_t magat_sim_mapf_workspace_bytes\(", hdr) and re.search(r"int magat_sim_mapf_plan\(", hdr)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    # added at the END of the header, behind the expert entries
    assert hdr.index("int magat_sim_expert_stats(") < hdr.index("size_t magat_sim_mapf_workspace_bytes(") \
        < hdr.index("int magat_sim_mapf_plan(")
    assert [len(nat._SIGNATURES[n][1]) for n in ENTRIES] == [2, 18]
    assert int(re.search(r"#define MAGAT_TAG_SIM_MAPF (\d+)", common).group(1)) == nat.TAG_SIM_MAPF == 28
    assert nat.TAGS[nat.TAG_SIM_MAPF] == "sim_mapf"
    assert int(re.search(r"#define MAGAT_FORM_SIM_MAPF (\d+)", common).group(1)) == nat.FORMS["sim_mapf"] == 18
    assert int(re.search(r"#define MAGAT_PROF_TAGS_ALL (\d+)", common).group(1)) == 29
    assert int(re.search(r"#define MAGAT_FORMS_ALL (\d+)", common).group(1)) == 19
    # the public counts are what the bindings of ABI 9 were built against
    assert re.search(r"#define MAGAT_PROF_TAGS 26\b", hdr) and re.search(r"#define MAGAT_FORMS 16\b", hdr)
    for name in ("plan_prioritized", "solve_cases", "solved_pack"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    assert lib.magat_form_count(nat.FORMS["sim_mapf"]) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(nat.TAG_SIM_MAPF, ctypes.byref(c), ctypes.byref(ms)) == 0
    assert lib.magat_sim_mapf_workspace_bytes(3, 64) == 3 * 64 * 5 * 64 * 8
    assert lib.magat_sim_mapf_workspace_bytes(0, 64) == 0 and lib.magat_sim_mapf_workspace_bytes(3, -1) == 0


def test_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one = ctypes.c_void_p(16)
    big = 1 << 40

    def call(map_=one, H=20, W=20, start=one, order=None, paths=one, ws=one, ws_bytes=big, C=2, N=4, T=64):
        return lib.magat_sim_mapf_plan(map_, 0, H, W, start, one, order, paths, one, one, one, one, ws, ws_bytes, C, N, T, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf"])
    assert call(map_=None) == -5 and call(start=None) == -5 and call(paths=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1
    assert call(H=65) == -2 and call(W=65) == -2 and call(T=257) == -2
    assert call(ws_bytes=lib.magat_sim_mapf_workspace_bytes(2, 64) - 1) == -2
    assert call(map_=None, H=0, T=999) == -5 and call(H=0, T=999) == -1      # null, then sizes, then limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf"]) == before            # a refused call is not counted as a launch


def test_cpu_tensors_raise():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    m = torch.zeros(5, 5, dtype=torch.uint8)
    s = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.plan_prioritized(m, s, s)
    with pytest.raises(nat.MagatNativeError):
        mapf.solve_cases(m, s, s)
    assert mapf.default_horizon(20, 20, 10) == 90 and mapf.default_horizon(64, 64, 100) == 256


def test_promote_keeps_the_others_in_order():
    from magat_pathplanning_amd import mapf
    order = torch.tensor([[0, 1, 2, 3], [2, 0, 3, 1], [3, 2, 1, 0]], dtype=torch.int32)
    got = mapf.promote(order, torch.tensor([2, 1, 3], dtype=torch.int32))
    assert got.tolist() == [[2, 0, 1, 3], [1, 2, 0, 3], [3, 2, 1, 0]] and got.dtype == torch.int32
    for row, a in zip(order.tolist(), (2, 1, 3)):
        assert mr.promote(row, a) == mapf.promote(torch.tensor([row]), torch.tensor([a]))[0].tolist()


# ---- the restatement on hand cases -------------------------------------------------------------------------------------------
def _plan(name, order=None):
    k = HAND[name]
    return k, mr.plan(k["map"], k["start"], k["goal"], order, k["T"])


def _static_distance(m, s, g):
    dist = {tuple(s): 0}
    queue = [tuple(s)]
    for u in queue:
        for dr, dc in mr.MOVES[:4]:
            v = (u[0] + dr, u[1] + dc)
            if 0 <= v[0] < m.shape[0] and 0 <= v[1] < m.shape[1] and m[v] == 0 and v not in dist:
                dist[v] = dist[u] + 1
                queue.append(v)
    return dist[tuple(g)]


def test_second_agent_waits_in_the_pocket():
    k, out = _plan("wait_in_pocket")
    assert out["solved"] == 1 and out["failed_agent"] == -1
    assert mr.check_schedule(k["map"], k["start"], k["goal"], out["paths"], out["lengths"]) is None
    assert out["lengths"][0] - 1 == _static_distance(k["map"], k["start"][0], k["goal"][0]) == 6
    assert out["lengths"][1] - 1 > _static_distance(k["map"], k["start"][1], k["goal"][1]) == 6
    p1 = [tuple(c) for c in out["paths"][1]]
    t_pass = [tuple(c) for c in out["paths"][0]].index((1, 4))            # agent 0 passes the mouth of the pocket ...
    assert p1[t_pass] == (2, 4)                                          # ... while agent 1 stands in it
    assert any(p1[t] == p1[t + 1] for t in range(out["lengths"][1] - 1))   # and it spends a stop action on the way
    assert out["makespan"] == out["lengths"].max() - 1
    assert (out["paths"][1, out["lengths"][1]:] == k["goal"][1]).all()     # padded with the last cell


def test_head_on_pair_in_a_closed_corridor_is_unsolved_in_both_orders():
    for order, failing in (([0, 1], 1), ([1, 0], 0)):
        k, out = _plan("head_on_closed", order)
        assert out["solved"] == 0 and out["failed_agent"] == failing
        assert out["lengths"][failing] == 1 and (out["paths"][failing] == k["start"][failing]).all()
        assert out["lengths"][1 - failing] == 7                           # the agent planned before the failure keeps its path
    k = HAND["head_on_closed"]
    out = mr.solve_with_retries(k["map"], k["start"], k["goal"], k["T"], retries=3)
    assert out["solved"] == 0 and out["rounds"] == 4


def test_start_equal_to_goal_has_length_one():
    k, out = _plan("start_is_goal")
    assert out["solved"] == 1 and out["lengths"].tolist() == [1, 1] and out["makespan"] == 0
    assert (out["paths"] == k["start"][:, None, :]).all()


def test_a_goal_crossed_at_time_5_is_not_held_before():
    k, out = _plan("goal_crossed_at_5")
    assert out["solved"] == 1
    assert tuple(out["paths"][0, 5]) == tuple(k["goal"][1])                # the higher-priority agent stands on it at t = 5
    assert _static_distance(k["map"], k["start"][1], k["goal"][1]) == 1
    assert out["lengths"][1] - 1 > 5
    assert mr.check_schedule(k["map"], k["start"], k["goal"], out["paths"], out["lengths"]) is None


def test_unsolved_in_index_order_solved_after_one_promotion():
    k, out = _plan("needs_promotion")
    assert out["solved"] == 0 and out["failed_agent"] == 1
    out = mr.solve_with_retries(k["map"], k["start"], k["goal"], k["T"])
    assert out["solved"] == 1 and out["rounds"] == 2 and out["order"].tolist() == [1, 0]
    assert mr.check_schedule(k["map"], k["start"], k["goal"], out["paths"], out["lengths"]) is None


def test_screening_of_bad_cases():
    k = HAND["wait_in_pocket"]
    T = k["T"]
    on_wall = mr.plan(k["map"], [(1, 0), (0, 0)], [(1, 6), (1, 3)], None, T)
    assert on_wall["solved"] == 0 and on_wall["failed_agent"] == 1 and on_wall["lengths"].tolist() == [7, 1]
    off_map = mr.plan(k["map"], [(1, 0), (1, 3)], [(1, 7), (1, 2)], None, T)
    assert off_map["failed_agent"] == 0 and off_map["lengths"].tolist() == [1, 1] and off_map["makespan"] == 0
    same_goal = mr.plan(k["map"], [(1, 0), (1, 6)], [(1, 3), (1, 3)], [1, 0], T)
    assert same_goal["solved"] == 0 and same_goal["failed_agent"] == 0      # the LATER agent of the order
    same_start = mr.plan(k["map"], [(1, 0), (1, 0)], [(1, 3), (1, 5)], None, T)
    assert same_start["failed_agent"] == 1
    for order in ([0, 0], [0, 2], [0], [-1, 0]):
        bad = mr.plan(k["map"], k["start"], k["goal"], order, T)
        assert bad["solved"] == 0 and bad["failed_agent"] == -2 and bad["lengths"].tolist() == [1, 1]
        assert (bad["paths"] == k["start"][:, None, :]).all()


# ---- the restatement against an exhaustive search ----------------------------------------------------------------------------
def _brute_arrival(m, planned, s, g, T):
    """The earliest arrival of one agent given the padded paths (T,2) of the agents before it: breadth first over (cell, t),
    conflicts read from the PATHS (no boards).  -1: none below T."""
    H, W = m.shape
    s, g = tuple(int(v) for v in s), tuple(int(v) for v in g)
    held = [{tuple(p[t]) for p in planned} for t in range(T)]
    last = max([t for t in range(T) if g in held[t]], default=-1)
    frontier = {s}
    for t in range(T):
        if t > last and g in frontier:
            return t
        if t == T - 1:
            return -1
        nxt = set()
        for u in frontier:
            for dr, dc in mr.MOVES:
                v = (u[0] + dr, u[1] + dc)
                if not (0 <= v[0] < H and 0 <= v[1] < W) or m[v] != 0 or v in held[t + 1]:
                    continue
                if any(tuple(p[t + 1]) == u and tuple(p[t]) == v for p in planned):      # a swap
                    continue
                nxt.add(v)
        frontier = nxt
    return -1


@pytest.mark.parametrize("seed", range(36))
def test_arrival_times_are_optimal_on_random_6x6_cases(seed):
    rng = np.random.default_rng(1000 + seed)
    m, start, goal = mr.random_case(rng, 6, 6, 3, 0.25)
    order = rng.permutation(3).tolist() if seed % 2 else [0, 1, 2]
    T = 20
    out = mr.plan(m, start, goal, order, T)
    planned = []
    for a in order:
        want = _brute_arrival(m, planned, start[a], goal[a], T)
        if want < 0:
            assert out["solved"] == 0 and out["failed_agent"] == a
            break
        assert out["lengths"][a] - 1 == want, (seed, a)
        planned.append(out["paths"][a])
    else:
        assert out["solved"] == 1 and out["failed_agent"] == -1
        assert mr.check_schedule(m, start, goal, out["paths"], out["lengths"]) is None


def test_the_10x10_batch_is_solved_within_the_retries():
    """The batch that tests/test_gpu_mapf.py asserts `all solved` on: the restatement alone solves it (and not all at once)."""
    m, start, goal = mr.random_batch(SEED_10x10, 40, 10, 10, 8, 0.2)
    first = mr.plan_batch(m, start, goal, None, 48)
    out = mr.solve_batch(m, start, goal, 48, retries=8)
    assert 0 < int(first["solved"].sum()) < 40
    assert int(out["solved"].sum()) == 40 and int(out["rounds"].max()) > 1
    for c in range(40):
        assert mr.check_schedule(m, start[c], goal[c], out["paths"][c], out["lengths"][c]) is None, c


# ---- check_schedule finds planted faults -------------------------------------------------------------------------------------
def test_check_schedule_names_planted_faults():
    m = np.zeros((3, 4), dtype=np.uint8)
    m[2, 3] = 1
    start, goal = np.array([[0, 0], [1, 1]]), np.array([[0, 2], [1, 1]])
    good = np.array([[[0, 0], [0, 1], [0, 2], [0, 2]], [[1, 1], [1, 1], [1, 1], [1, 1]]])
    assert mr.check_schedule(m, start, goal, good, [3, 1]) is None

    def fault(paths, lengths=(3, 1), s=start, g=goal):
        return mr.check_schedule(m, s, g, np.array(paths), list(lengths)) or ""

    assert "begin" in fault([[[0, 1], [0, 1], [0, 2], [0, 2]], good[1]])
    assert "end" in fault(good, lengths=(2, 1))
    assert "five moves" in fault([[[0, 0], [0, 2], [0, 2], [0, 2]], good[1]])
    assert "padding" in fault([[[0, 0], [0, 1], [0, 2], [0, 3]], good[1]])
    assert "free" in fault([[[1, 3], [2, 3], [1, 3], [1, 3]], good[1]], s=np.array([[1, 3], [1, 1]]), g=np.array([[1, 3], [1, 1]]))
    assert "share" in fault([[[0, 0], [0, 1], [1, 1], [1, 1]], good[1]], g=np.array([[1, 1], [1, 1]]))
    swap = [[[0, 0], [0, 1], [0, 1], [0, 1]], [[0, 1], [0, 0], [0, 0], [0, 0]]]
    assert "swap" in fault(swap, lengths=(2, 2), s=np.array([[0, 0], [0, 1]]), g=np.array([[0, 1], [0, 0]]))
