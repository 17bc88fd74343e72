"""CPU-only: conflict-based search (csrc/sim_mapf_cbs.hip, mapf.cbs_cases).  The yardstick is tests/cbs_restatement.py; here it
is checked against an exhaustive joint search (optimality, and the lower bound at every budget), against
mapf_restatement.check_schedule and solve_with_retries, and on hand cases; the inputs of tests/test_gpu_cbs.py are made (once per
session, with the restatement's answer) and what each of them is there for is asserted.  Then the host side of the entries -
header / loader / build lists / workspace formula / argument checks - and the kernel compiled for the host, its wavefront
emulated by threads (tools/host_wave)."""
import ctypes
import functools
import heapq
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cbs_restatement as cr
import mapf_restatement as mr
from conftest import ROOT

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
ENTRIES = ("magat_sim_mapf_cbs_workspace_bytes", "magat_sim_mapf_cbs")
KEYS = ("paths", "lengths", "makespan", "solved", "status", "flowtime", "lower_bound", "nodes", "expanded", "horizon_hit")
# the issue's table: seed, C, H, W, N, density, T, cases that end with status 0 at max_nodes = 512
RANDOM = {"r8": (5, 24, 8, 8, 6, 0.2, 40, 17), "r10": (7, 16, 10, 10, 8, 0.1, 48, 14), "r20": (9, 8, 20, 20, 10, 0.1, 64, 8)}


# ---- the inputs: name -> dict(map, start, goal, T, max_nodes) -------------------------------------------------------------------------
def _case(m, s, g, T, max_nodes):
    return dict(map=np.asarray(m, dtype=np.uint8), start=np.asarray(s, dtype=np.int32), goal=np.asarray(g, dtype=np.int32), T=T,
                max_nodes=max_nodes)


def small_batch():
    """Six cases on 3 x 5 maps of their own: an agent parked on its goal that the other must cross (it steps into the pocket and
    comes back: the `last` rule); a goal in another component; a duplicate start; a duplicate goal; a start off the map; a goal
    on an obstacle."""
    pocket = mr.grid(["##.##", ".....", "#####"])
    split = mr.grid(["..#..", "..#..", "..#.."])
    maps = [pocket, split, pocket, pocket, pocket, pocket]
    start = [[(1, 2), (1, 0)], [(0, 0), (1, 0)], [(1, 1), (1, 1)], [(1, 0), (1, 1)], [(1, 0), (1, 5)], [(1, 0), (1, 1)]]
    goal = [[(1, 2), (1, 4)], [(0, 4), (2, 1)], [(1, 3), (1, 4)], [(1, 3), (1, 3)], [(1, 3), (1, 4)], [(1, 3), (0, 0)]]
    return _case(np.stack(maps), start, goal, 16, 64)


def corner64():
    """The pocket swap against row 63 / column 63 of a 64 x 64 map: once along row 63 (lane 63) with the pocket above it, once
    down column 63 (bit 63) with the pocket to its left."""
    a = np.ones((64, 64), dtype=np.uint8)
    a[63, 59:64] = 0
    a[62, 61] = 0
    b = np.ones((64, 64), dtype=np.uint8)
    b[59:64, 63] = 0
    b[61, 62] = 0
    return _case(np.stack([a, b]), [[(63, 60), (63, 62)], [(60, 63), (62, 63)]], [[(63, 62), (63, 60)], [(62, 63), (60, 63)]], 16, 256)


def serpentine_T256():
    """test_gpu_mapf's serpentine with a two-wide last leg: agent 0 walks 134 steps to (14, 0); agent 1 steps out of row 15 onto
    (14, 5) at once and is parked in its way 129 steps later - agent 0 goes round it through row 15."""
    m = np.zeros((16, 16), dtype=np.uint8)
    for r in range(1, 15, 2):
        m[r, :] = 1
        m[r, 15 if (r // 2) % 2 == 0 else 0] = 0
    return _case(m, [[(0, 0), (15, 5)]], [[(14, 0), (14, 5)]], 256, 64)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "pocket":
        k = cr.pocket_swap()
        k = _case(k["map"], k["start"][None], k["goal"][None], k["T"], 256)
    elif name == "hand":          # mapf_restatement's five, a map per case; the closed corridor ends at the budget
        cases = list(mr.hand_cases().values())
        k = _case(np.stack([c["map"] for c in cases]), np.stack([c["start"] for c in cases]), np.stack([c["goal"] for c in cases]), 24, 64)
    elif name == "small":
        k = small_batch()
    elif name in RANDOM:
        seed, C, H, W, N, density, T, _ = RANDOM[name]
        k = _case(*mr.random_batch(seed, C, H, W, N, density, batched_map=True), T, 512)
    elif name.startswith("r8_m"):
        k = dict(case("r8"), max_nodes=int(name[4:]))
    elif name == "r8_c1":
        r8 = case("r8")
        k = _case(r8["map"][:1], r8["start"][:1], r8["goal"][:1], r8["T"], 512)
    elif name == "corner64":
        k = corner64()
    elif name == "w33":           # the remaining ones: ONE map (H,W) for the batch
        k = _case(*mr.random_batch(33, 4, 9, 33, 5, 0.15), 60, 32)
    elif name == "wide5x64":
        k = _case(*mr.random_batch(31, 3, 5, 64, 4, 0.1), 96, 32)
    elif name == "tall64x5":
        k = _case(*mr.random_batch(32, 3, 64, 5, 4, 0.1), 96, 32)
    elif name == "serpentine_T256":
        k = serpentine_T256()
    else:
        raise KeyError(name)
    if "want" not in k or name.startswith("r8_m"):
        k = dict(k, want=cr.cbs_batch(k["map"], k["start"], k["goal"], k["T"], k["max_nodes"]))
    return k


def tiled(name, C):
    """The first C cases of a batch repeated over and over, with the restatement's answers repeated alike."""
    k = case(name)
    idx = np.arange(C) % len(k["start"])
    return dict(map=k["map"][idx] if k["map"].ndim == 3 else k["map"], start=k["start"][idx], goal=k["goal"][idx], T=k["T"], max_nodes=k["max_nodes"],
                want={key: value[idx] for key, value in k["want"].items()})


def case_map(k, c):
    return k["map"] if k["map"].ndim == 2 else k["map"][c]


def flow(res):
    return (np.asarray(res["lengths"], dtype=np.int64) - 1).sum(-1)


def check_consistent(k):
    """What every answer has to satisfy on its own: the schedule of a status-0 case is valid and its numbers agree."""
    w = k["want"]
    for c in range(len(k["start"])):
        if w["status"][c] == 0:
            assert mr.check_schedule(case_map(k, c), k["start"][c], k["goal"][c], w["paths"][c], w["lengths"][c]) is None, c
            assert w["solved"][c] == 1 and w["flowtime"][c] == w["lower_bound"][c] == flow(w)[c]
            assert w["makespan"][c] == w["lengths"][c].max() - 1 and w["nodes"][c] == 1 + 2 * w["expanded"][c]
        else:
            assert w["solved"][c] == 0 and w["flowtime"][c] == -1 and w["makespan"][c] == 0 and (w["lengths"][c] == 1).all()
            assert (w["paths"][c] == k["start"][c][:, None, :]).all()
            assert (w["lower_bound"][c] >= 0) == (w["status"][c] == 1)


ALL_NAMES = ("pocket", "hand", "small", "r8", "r10", "r20", "r8_m1", "r8_m2", "r8_m3", "r8_m8", "r8_c1", "corner64", "w33", "wide5x64",
             "tall64x5", "serpentine_T256")


def check_what_the_case_is_there_for(name):
    k = case(name)
    w = k["want"]
    check_consistent(k)
    if name == "pocket":          # prioritized planning fails in every order; CBS: 21 nodes, flowtime 7
        r = mr.solve_with_retries(k["map"], k["start"][0], k["goal"][0], k["T"])
        assert r["solved"] == 0 and r["rounds"] == 9
        assert (w["status"][0], w["flowtime"][0], w["nodes"][0], w["expanded"][0], w["horizon_hit"][0]) == (0, 7, 21, 10, 0)
    if name == "hand":
        assert w["status"].tolist() == [0, 1, 0, 0, 0] and w["nodes"][1] == 63 and w["nodes"][2] == 1
    if name == "small":
        assert w["status"].tolist() == [0, 2, 3, 3, 3, 3] and w["horizon_hit"].tolist() == [0, 1, 0, 0, 0, 0]
        assert w["nodes"].tolist()[1:] == [0] * 5
        # the parked agent is in the pocket while the other stands on its goal at t = 2, and back at t = 3: 3 + 4 steps
        assert w["lengths"][0].tolist() == [4, 5] and w["paths"][0, :, 2].tolist() == [[0, 2], [1, 2]] and w["flowtime"][0] == 7
    if name in RANDOM:
        assert int((w["status"] == 0).sum()) == RANDOM[name][7] and 2 * RANDOM[name][7] >= len(w["status"])
        assert int(w["horizon_hit"].sum()) == 0 and int(w["nodes"].max()) > 8
    if name.startswith("r8_m"):
        M = k["max_nodes"]
        assert int(w["nodes"].max()) <= M and int((w["status"] == 1).sum()) > 0
        assert int(w["expanded"].max()) == (M - 1) // 2
    if name == "corner64":
        assert w["status"].tolist() == [0, 0] and w["flowtime"].tolist() == [7, 7]
    if name in ("w33", "wide5x64", "tall64x5"):
        assert k["map"].ndim == 2 and int((w["status"] == 0).sum()) > 0 and int(w["nodes"].max()) > 1
    if name == "serpentine_T256":
        assert w["status"].tolist() == [0] and w["lengths"][0, 0] - 1 > 130 and w["nodes"][0] >= 3
        assert w["flowtime"][0] == 134 + 2 + 1


@pytest.mark.parametrize("name", ALL_NAMES)
def test_inputs_of_the_gpu_tests(name):
    check_what_the_case_is_there_for(name)


def test_status_0_never_costs_more_than_prioritized_planning():
    for name in RANDOM:
        k = case(name)
        w = k["want"]
        pp = mr.solve_batch(k["map"], k["start"], k["goal"], k["T"])
        both = (w["status"] == 0) & (pp["solved"] != 0)
        assert int(both.sum()) > 0 and (w["flowtime"][both] <= flow(pp)[both]).all(), name
        assert (w["flowtime"][both] < flow(pp)[both]).any(), name      # ... and it does find better schedules


# ---- optimality and the bound, against an exhaustive joint search -----------------------------------------------------------------------
def optimum(m, start, goal):
    """The smallest flowtime of a case, or None when it has no solution: Dijkstra over (positions, per-agent "stays for good"
    flags).  A step costs the number of agents not yet staying; an agent standing on its goal may begin to stay."""
    free = np.asarray(m) == 0
    H, W = free.shape
    S, G = [tuple(int(v) for v in s) for s in start], [tuple(int(v) for v in g) for g in goal]
    N = len(S)

    def options(pos, flags, movers):
        home = [a for a in movers if pos[a] == G[a]]
        for r in range(len(home) + 1):
            for sub in itertools.combinations(home, r):
                yield tuple(flags[a] or a in sub for a in range(N))

    heap, best = [], {}
    for flags in options(S, (False,) * N, range(N)):
        heapq.heappush(heap, (0, tuple(S), flags))
        best[tuple(S), flags] = 0
    while heap:
        d, pos, flags = heapq.heappop(heap)
        if d > best[pos, flags]:
            continue
        if all(flags):
            return d
        movers = [a for a in range(N) if not flags[a]]
        for combo in itertools.product(mr.MOVES, repeat=len(movers)):
            new = list(pos)
            for a, (dr, dc) in zip(movers, combo):
                new[a] = (pos[a][0] + dr, pos[a][1] + dc)
            if any(not (0 <= v[0] < H and 0 <= v[1] < W) or not free[v] for v in new) or len(set(new)) < N:
                continue
            if any(new[a] == pos[b] and new[b] == pos[a] for a in movers for b in movers if a < b):
                continue
            for nf in options(new, flags, movers):
                key = (tuple(new), nf)
                if d + len(movers) < best.get(key, 1 << 30):
                    best[key] = d + len(movers)
                    heapq.heappush(heap, (d + len(movers), key[0], nf))
    return None


@functools.lru_cache(maxsize=None)
def tiny_cases():
    """20 cases of 2 agents on 4 x 4 and 16 of 3 agents on 3 x 3, with obstacles, and two without a solution; each with its optimum."""
    rng = np.random.default_rng(2024)
    cases = [mr.random_case(rng, 4, 4, 2, 0.3) for _ in range(20)] + [mr.random_case(rng, 3, 3, 3, 0.2) for _ in range(16)]
    closed = mr.grid(["####", "....", "####"])
    cases.append((closed, np.array([(1, 0), (1, 3)]), np.array([(1, 3), (1, 0)])))      # head-on in a closed corridor
    cases.append((closed, np.array([(1, 0), (1, 1)]), np.array([(1, 1), (1, 3)])))      # the one in front stops too early
    return [(m, s, g, optimum(m, s, g)) for m, s, g in cases]


def test_the_exhaustive_search_on_cases_worked_out_by_hand():
    k = cr.pocket_swap()
    assert optimum(k["map"], k["start"], k["goal"]) == 7
    free = mr.grid(["...", "..."])
    assert optimum(free, [(0, 0)], [(1, 2)]) == 3 and optimum(free, [(0, 0), (0, 1)], [(0, 1), (0, 0)]) == 4
    assert optimum(mr.grid(["..."]), [(0, 0), (0, 2)], [(0, 2), (0, 0)]) is None
    assert optimum(free, [(1, 1)], [(1, 1)]) == 0


def test_status_0_is_the_optimum():
    solved = unsolvable = conflicts = 0
    for m, s, g, best in tiny_cases():
        out = cr.cbs(m, s, g, 24, 256)
        if best is None:
            unsolvable += 1
            assert out["status"] in (1, 2)
            continue
        if out["status"] == 0:
            solved += 1
            conflicts += out["nodes"] > 1
            assert out["flowtime"] == best, (m, s, g)
            assert mr.check_schedule(m, s, g, out["paths"], out["lengths"]) is None
        assert out["horizon_hit"] == 1 or out["lower_bound"] <= best
    assert solved >= 30 and unsolvable >= 2 and conflicts >= 8


@pytest.mark.parametrize("max_nodes", [1, 3, 8])
def test_lower_bound_at_every_budget(max_nodes):
    at_budget = 0
    for m, s, g, best in tiny_cases():
        out = cr.cbs(m, s, g, 24, max_nodes)
        assert out["nodes"] <= max_nodes
        at_budget += out["status"] == 1
        if out["status"] == 0:
            assert out["flowtime"] == best
        if out["horizon_hit"] == 0 and out["status"] in (0, 1) and best is not None:
            assert 0 <= out["lower_bound"] <= best, (m, s, g)
    assert at_budget >= 4


# ---- the host side of the entries -----------------------------------------------------------------------------------------------------
def documented_bytes(C, N, T, M):
    return C * 8 * (T * 5 * 64 + (N * T + 3) // 4 + (M * T + 3) // 4 + 2 * M + (N + 1) // 2 + N)


def test_cbs_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(CSRC, "magat_common.h")).read()
    assert "sim_mapf_cbs.hip" in build_native.SOURCES
    text = open(os.path.join(CSRC, "sim_mapf_cbs.hip")).read()
    assert "MAGAT_FORM_SIM_MAPF_CBS" in text and "MAGAT_TAG_SIM_MAPF_CBS" in text
    for part in ("sim_mapf_parts.h", "sim_mapf_audit_parts.h", "sim_mapf_tree.h", "row_board.h"):
        assert '#include "%s"' % part in text and part in build_native.HEADERS
    tree = open(os.path.join(CSRC, "sim_mapf_tree.h")).read()      # the walk, once for the three tree experts: it holds the conflict scan
    assert "mapf_search<true>" in text and "mapf_search<false>" in text and "mapf_tree_search(" in text and "audit_stage2(" in tree
    assert "audit_stage2(" not in text and "asm" not in tree and "printf" not in tree and "assert(" not in tree
    assert "asm" not in text and "printf" not in text and "assert(" not in text and "hipDeviceSynchronize" not in text
    assert re.search(r"^size_t magat_sim_mapf_cbs_workspace_bytes\(int C, int N, int T, int max_nodes\);", hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_cbs\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    assert len(nat._SIGNATURES["magat_sim_mapf_cbs"][1]) == 23
    tag = int(re.search(r"#define MAGAT_TAG_SIM_MAPF_CBS (\d+)", common).group(1))
    form = int(re.search(r"#define MAGAT_FORM_SIM_MAPF_CBS (\d+)", common).group(1))
    assert tag == nat.TAG_SIM_MAPF_CBS and nat.TAGS[tag] == "sim_mapf_cbs" and form == nat.FORMS["sim_mapf_cbs"]
    assert tag == nat.TAG_SIM_MAPF_AUDIT + 1 and form == nat.FORMS["sim_mapf_audit"] + 1
    assert "cbs_cases" in pkg.__all__ and callable(pkg.cbs_cases)
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.magat_form_count(form) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0


def test_cbs_workspace_formula():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for C, N, T, M in ((1, 1, 1, 1), (512, 10, 64, 256), (128, 100, 128, 256), (300, 6, 40, 512), (2, 4096, 256, 4096), (3, 7, 33, 5)):
        assert lib.magat_sim_mapf_cbs_workspace_bytes(C, N, T, M) == documented_bytes(C, N, T, M), (C, N, T, M)
    assert documented_bytes(1, 10, 64, 1024) - documented_bytes(1, 10, 64, 0) == 1024 * (2 * 64 + 16)      # the node pool
    for bad in ((0, 4, 8, 16), (1, 0, 8, 16), (1, 4, 0, 16), (1, 4, 8, 0), (-1, 4, 8, 16), (1, 4097, 8, 16), (1, 4, 257, 16), (1, 4, 8, 4097)):
        assert lib.magat_sim_mapf_cbs_workspace_bytes(*bad) == 0, bad


def test_cbs_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50

    def call(map_=one, H=20, W=20, start=one, paths=one, solved=one, status=one, hit=one, ws=one, ws_bytes=big, C=2, N=4, T=64, M=32):
        return lib.magat_sim_mapf_cbs(map_, 0, H, W, start, one, paths, one, one, solved, status, one, one, one, one, hit, ws, ws_bytes,
                                      C, N, T, M, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_cbs"])
    assert call(map_=None) == -5 and call(start=None) == -5 and call(paths=None) == -5 and call(solved=None) == -5
    assert call(status=None) == -5 and call(hit=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1 and call(M=0) == -1
    assert call(H=65) == -2 and call(W=65) == -2 and call(T=257) == -2 and call(N=4097) == -2 and call(M=4097) == -2
    assert call(ws_bytes=documented_bytes(2, 4, 64, 32) - 1) == -2
    # the limits themselves pass: the next check is the workspace's size, then its alignment
    full = documented_bytes(2, 4096, 256, 4096)
    assert call(H=64, W=64, T=256, N=4096, M=4096, ws_bytes=full - 1) == -2
    assert call(H=64, W=64, T=256, N=4096, M=4096, ws=odd, ws_bytes=full) == -3
    assert call(ws=odd) == -3 and call(H=1, W=1, T=1, N=1, C=1, M=1, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1 and call(T=9999, ws=odd) == -2      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_cbs"]) == before              # a refused call is not counted as a launch


def test_python_surface_on_cpu_tensors():
    import inspect
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    sig = inspect.signature(mapf.cbs_cases)
    assert list(sig.parameters) == ["obstacle_map", "start", "goal", "horizon", "max_nodes"]
    assert sig.parameters["horizon"].default is None and sig.parameters["max_nodes"].default == 256
    assert inspect.signature(mapf.solve_cases).parameters["optimal"].default is None
    m = torch.zeros(5, 5, dtype=torch.uint8)
    cell = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.cbs_cases(m, cell, cell)
    with pytest.raises(nat.MagatNativeError):
        mapf.solve_cases(m, cell, cell, optimal=16)


# ---- the kernel itself, compiled for the host: one thread per lane (tools/host_wave) ---------------------------------------------------
def _case_text(k):
    C, N, _ = k["start"].shape
    ints = [C, N, k["T"], k["map"].shape[-2], k["map"].shape[-1], k["max_nodes"], int(k["map"].ndim == 3)]
    for a in (k["map"], k["start"], k["goal"]):
        ints += np.asarray(a).astype(np.int64).reshape(-1).tolist()
    return " ".join(str(v) for v in ints)


@pytest.fixture(scope="module")
def cbs_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "cbs_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_cbs_check.cpp"), "-o", exe], check=True)
    return exe


# (every thread rendezvous is a futex here, so the suite runs the small inputs; deeper trees were run by hand - DESIGN 4.11)
@pytest.mark.parametrize("name,cases", [("pocket", 1), ("small", 6), ("r8_m8", 4), ("corner64", 2)])
def test_kernel_compiled_for_the_host_equals_the_restatement(cbs_check, tmp_path, name, cases):
    """The kernel with its wavefront emulated by threads and barriers - ballot, DPP shift, readfirstlane and shuffle as exchanges
    inside the wavefront, __syncthreads as a rendezvous, atomicMin as a compare-and-swap.  It covers the algorithm, the indexing
    and the barriers - not the hardware."""
    k = tiled(name, cases)
    (tmp_path / "case.txt").write_text(_case_text(k))
    run = subprocess.run([cbs_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key, line_ in zip(KEYS, lines[1:]):
        got = np.array(line_.split(), dtype=np.int64).reshape(np.asarray(k["want"][key]).shape)
        np.testing.assert_array_equal(got, k["want"][key], err_msg="%s: %s" % (name, key))
