"""CPU-only: bounded-suboptimal conflict-based search, ECBS (csrc/sim_mapf_ecbs.hip, mapf.ecbs_cases).  The yardstick is
tests/ecbs_restatement.py; here it is checked against test_host_cbs's exhaustive joint search (the bound and the promise
1000 * flowtime <= w_milli * lower_bound at every budget, optimality at w = 1), against cbs_restatement on the random batches,
against mapf_restatement.check_schedule, and on hand cases; the inputs of tests/test_gpu_ecbs.py are made (once per session, with
the restatement's answer).  Then the host side of the entries - header / loader / build lists / workspace formula / argument
checks - and the kernel compiled for the host, its wavefront emulated by threads (tools/host_wave)."""
import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ecbs_restatement as er
import mapf_restatement as mr
import test_host_cbs as hc
from conftest import ROOT

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
ENTRIES = ("magat_sim_mapf_ecbs_workspace_bytes", "magat_sim_mapf_ecbs")
KEYS = hc.KEYS
# the inputs of the GPU tests: test_host_cbs's, at (w_milli, levels, max_nodes)
GPU_INPUTS = (("pocket", 1500, 4, 64), ("hand", 1500, 4, 64), ("small", 1500, 4, 64), ("r8", 1000, 4, 64), ("r8", 1200, 2, 64),
              ("r8", 1500, 4, 64), ("r8", 1500, 1, 64), ("r8", 1500, 3, 8), ("r10", 1500, 4, 64), ("r20", 1200, 4, 64),
              ("corner64", 1500, 4, 64), ("w33", 1000, 4, 32), ("wide5x64", 1000, 4, 32), ("wide5x64", 1500, 4, 64),
              ("tall64x5", 1500, 4, 64),
              ("serpentine_T256", 1050, 4, 64))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """map, start, goal, T of one of test_host_cbs's inputs - without its CBS answer where only the inputs are wanted."""
    if name in hc.RANDOM:
        seed, C, H, W, N, density, T, _ = hc.RANDOM[name]
        return hc._case(*mr.random_batch(seed, C, H, W, N, density, batched_map=True), T, 0)
    if name == "small":
        return hc.small_batch()
    if name == "corner64":
        return hc.corner64()
    if name == "serpentine_T256":
        return hc.serpentine_T256()
    if name == "crossing":
        k = er.crossing()
        return hc._case(k["map"], k["start"][None], k["goal"][None], k["T"], 0)
    return hc.case(name)


@functools.lru_cache(maxsize=None)
def case(name, w_milli, levels, max_nodes):
    k = inputs(name)
    k = dict(map=k["map"], start=k["start"], goal=k["goal"], T=k["T"], max_nodes=max_nodes, w_milli=w_milli, levels=levels)
    k["want"] = er.ecbs_batch(k["map"], k["start"], k["goal"], k["T"], w_milli, max_nodes, levels)
    return k


def tiled(k, C):
    """The first C cases of a batch repeated over and over, with the restatement's answers repeated alike."""
    idx = np.arange(C) % len(k["start"])
    return dict(k, map=k["map"][idx] if k["map"].ndim == 3 else k["map"], start=k["start"][idx], goal=k["goal"][idx],
                want={key: value[idx] for key, value in k["want"].items()})


def check_consistent(k):
    """What every answer has to satisfy on its own."""
    w = k["want"]
    for c in range(len(k["start"])):
        if w["status"][c] == 0:
            assert mr.check_schedule(hc.case_map(k, c), k["start"][c], k["goal"][c], w["paths"][c], w["lengths"][c]) is None, c
            assert w["solved"][c] == 1 and w["flowtime"][c] == hc.flow(w)[c]
            assert 1000 * int(w["flowtime"][c]) <= k["w_milli"] * int(w["lower_bound"][c])
            assert w["makespan"][c] == w["lengths"][c].max() - 1 and w["nodes"][c] == 1 + 2 * w["expanded"][c]
        else:
            assert w["solved"][c] == 0 and w["flowtime"][c] == -1 and w["makespan"][c] == 0 and (w["lengths"][c] == 1).all()
            assert (w["paths"][c] == k["start"][c][:, None, :]).all()
            assert (w["lower_bound"][c] >= 0) == (w["status"][c] == 1)
        assert w["nodes"][c] <= k["max_nodes"]


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", GPU_INPUTS)
def test_inputs_of_the_gpu_tests(name, w_milli, levels, max_nodes):
    k = case(name, w_milli, levels, max_nodes)
    check_consistent(k)
    w = k["want"]
    if name == "pocket":
        assert w["status"].tolist() == [0] and w["flowtime"][0] <= 10 and w["lower_bound"][0] <= 7 and w["nodes"][0] > 1
    if name == "small":
        assert w["status"].tolist() == [0, 2, 3, 3, 3, 3] and w["horizon_hit"].tolist() == [0, 1, 0, 0, 0, 0]
        assert w["nodes"].tolist()[1:] == [0] * 5
    if name == "corner64":
        assert w["status"].tolist() == [0, 0]
    if name in ("w33", "wide5x64", "tall64x5"):
        assert k["map"].ndim == 2 and int((w["status"] == 0).sum()) > 0
        assert int(w["nodes"].max()) > 1 or w_milli > 1000      # at w = 1 the tree is needed; at 1.5 the root's focal search does it
    if name == "serpentine_T256":      # T = 256, and the window b = 1.05 t* reaches past t* = 134
        assert k["T"] == 256 and w["status"].tolist() == [0] and w["lengths"][0, 0] - 1 >= 134 and 1050 * 134 // 1000 > 134
    if (name, levels, max_nodes) == ("r8", 3, 8):
        assert int((w["status"] == 1).sum()) > 0


# ---- the promise, against the exhaustive joint search --------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 4])
@pytest.mark.parametrize("w_milli", [1000, 1250, 2000])
def test_bound_and_promise_at_every_budget(w_milli, levels):
    solved = at_budget = 0
    for m, s, g, best in hc.tiny_cases():
        for budget in (1, 3, 8, 256):
            out = er.ecbs(m, s, g, 24, w_milli, budget, levels)
            assert out["nodes"] <= budget
            at_budget += out["status"] == 1
            if out["status"] == 0:
                solved += 1
                assert best is not None
                assert mr.check_schedule(m, s, g, out["paths"], out["lengths"]) is None
                assert out["flowtime"] == int((out["lengths"] - 1).sum())
                assert 1000 * out["flowtime"] <= w_milli * out["lower_bound"], (m, s, g)
                if w_milli == 1000:
                    assert out["flowtime"] == best, (m, s, g)
            if out["horizon_hit"] == 0 and out["status"] in (0, 1) and best is not None:
                assert 0 <= out["lower_bound"] <= best, (m, s, g)
    assert solved >= 4 * 20 and at_budget >= 4


@pytest.mark.parametrize("name", ["r8", "r10", "r20"])
def test_w_1_gives_the_flowtime_of_cbs(name):
    k = case(name, 1000, 4, 64)
    opt = hc.case(name)["want"]            # CBS at 512 nodes
    both = (k["want"]["status"] == 0) & (opt["status"] == 0)
    assert int(both.sum()) > 0
    np.testing.assert_array_equal(k["want"]["flowtime"][both], opt["flowtime"][both])
    if name == "r8":
        for key in ((1000, 4, 64), (1200, 2, 64), (1500, 4, 64), (1500, 1, 64)):
            w = case("r8", *key)["want"]
            known = (w["status"] <= 1) & (opt["status"] == 0)
            assert int(known.sum()) > 0 and (w["lower_bound"][known] <= opt["flowtime"][known]).all(), key


def test_the_focal_search_solves_what_cbs_leaves_open_at_the_same_budget():
    """A condition: at (w 1.5, 4 levels, 64 nodes) every case of the 8 x 8 and the 10 x 10 batch is solved; conflict-based search
    at 64 nodes leaves at least a third of the 8 x 8 batch open."""
    for name in ("r8", "r10"):
        w = case(name, 1500, 4, 64)["want"]
        assert (w["status"] == 0).all(), (name, w["status"].tolist())
    opt = hc.case("r8_m64")["want"]
    assert 3 * int((opt["status"] != 0).sum()) >= len(opt["status"])


def test_pocket_swap_and_the_small_batch():
    k = case("pocket", 1500, 4, 64)
    w = k["want"]
    assert w["status"].tolist() == [0] and 7 <= w["flowtime"][0] <= 10 and w["horizon_hit"].tolist() == [0]
    assert mr.check_schedule(hc.case_map(k, 0), k["start"][0], k["goal"][0], w["paths"][0], w["lengths"][0]) is None
    one = case("pocket", 1000, 4, 64)["want"]
    assert one["status"].tolist() == [0] and one["flowtime"].tolist() == [7] and one["lower_bound"].tolist() == [7]
    w = case("small", 1500, 4, 64)["want"]
    assert w["status"].tolist() == [0, 2, 3, 3, 3, 3]


def test_the_focal_choice_shows_on_a_crossing():
    """Two agents crossing in an open 3 x 5 room: with a clean plane agent 1 waits a step and the root has no conflict; with the
    planner's plane alone it has one."""
    two = case("crossing", 1500, 2, 64)["want"]
    assert two["status"].tolist() == [0] and two["nodes"].tolist() == [1] and two["flowtime"].tolist() == [7]
    assert two["lower_bound"].tolist() == [6] and two["lengths"].tolist() == [[5, 4]]
    one = case("crossing", 1500, 1, 64)["want"]
    assert one["status"].tolist() == [0] and one["nodes"][0] > 1


def test_count_conflicts_on_hand_schedules():
    a, b = [(0, 0), (0, 1), (0, 2)], [(0, 2), (0, 1), (0, 0)]
    assert er.count_conflicts([a, b], [3, 3], 1, 3) == 1                          # both on (0, 1) at t = 1
    assert er.count_conflicts([[(0, 0), (0, 1)], [(0, 1), (0, 0)]], [2, 2], 1, 2) == 1      # one swap
    assert er.count_conflicts([[(0, 0)], [(0, 1), (0, 0)]], [1, 2], 1, 2) == 1     # a parked agent is run into
    assert er.count_conflicts([a, [(1, 0), (1, 1), (1, 2)]], [3, 3], 2, 3) == 0


# ---- the host side of the entries -----------------------------------------------------------------------------------------------------
def documented_bytes(C, N, T, M, K):
    return C * 8 * (T * 64 * (10 + K) + (N * T + 3) // 4 + (M * T + 3) // 4 + 4 * M + (5 * N + 1) // 2)


def test_ecbs_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(CSRC, "magat_common.h")).read()
    assert "sim_mapf_ecbs.hip" in build_native.SOURCES and "sim_mapf_cbs_parts.h" in build_native.HEADERS
    text = open(os.path.join(CSRC, "sim_mapf_ecbs.hip")).read()
    cbs = open(os.path.join(CSRC, "sim_mapf_cbs.hip")).read()
    parts = open(os.path.join(CSRC, "sim_mapf_cbs_parts.h")).read()
    assert "MAGAT_FORM_SIM_MAPF_ECBS" in text and "MAGAT_TAG_SIM_MAPF_ECBS" in text
    for part in ("sim_mapf_parts.h", "sim_mapf_audit_parts.h", "sim_mapf_cbs_parts.h", "sim_mapf_tree.h", "row_board.h"):
        assert '#include "%s"' % part in text and part in build_native.HEADERS
    assert '#include "sim_mapf_cbs_parts.h"' in cbs
    board = open(os.path.join(CSRC, "row_board.h")).read()
    tree = open(os.path.join(CSRC, "sim_mapf_tree.h")).read()
    # one copy, in the shared header: the chain marks and the placing in the parts, the wave reductions with the row boards
    for shared, home in (("wave_all_min", board), ("wave_all_max", board), ("wave_all_sum", board), ("wave_all_or", board), ("wave_all_min3", board),
                         ("cbs_mark", parts), ("cbs_mark_chain", parts), ("cbs_place", parts)):
        assert re.search(r"\b%s\(" % shared, home), shared
        for body in (text, cbs, tree):
            assert not re.search(r"^__device__ [^\n]*\b%s\(" % shared, body, re.M), shared
    for body in (text, cbs, parts, tree):      # and no butterfly of their own
        assert "__shfl_xor" not in body
    # the walk, once: this file calls it and holds no conflict scan of its own
    assert "mapf_tree_search(" in text and "audit_stage2(" in tree and "audit_stage2(" not in text
    assert "asm" not in text and "printf" not in text and "assert(" not in text
    assert "hipDeviceSynchronize" not in text
    assert re.search(r"^size_t magat_sim_mapf_ecbs_workspace_bytes\(int C, int N, int T, int max_nodes, int levels\);", hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_ecbs\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    assert len(nat._SIGNATURES["magat_sim_mapf_ecbs"][1]) == 25 and len(nat._SIGNATURES["magat_sim_mapf_cbs"][1]) == 23
    tag = int(re.search(r"#define MAGAT_TAG_SIM_MAPF_ECBS (\d+)", common).group(1))
    form = int(re.search(r"#define MAGAT_FORM_SIM_MAPF_ECBS (\d+)", common).group(1))
    assert tag == nat.TAG_SIM_MAPF_ECBS and nat.TAGS[tag] == "sim_mapf_ecbs" and form == nat.FORMS["sim_mapf_ecbs"]
    assert tag == nat.TAG_SIM_MAPF_CBS + 1 and form == nat.FORMS["sim_mapf_cbs"] + 1
    assert "ecbs_cases" in pkg.__all__ and callable(pkg.ecbs_cases)
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.magat_form_count(form) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0


def test_ecbs_workspace_formula():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for C, N, T, M, K in ((1, 1, 1, 1, 1), (512, 10, 64, 256, 4), (128, 100, 128, 256, 2), (300, 6, 40, 64, 3), (2, 4096, 256, 4096, 4),
                          (3, 7, 33, 5, 1)):
        assert lib.magat_sim_mapf_ecbs_workspace_bytes(C, N, T, M, K) == documented_bytes(C, N, T, M, K), (C, N, T, M, K)
    assert documented_bytes(1, 10, 64, 64, 4) - documented_bytes(1, 10, 64, 64, 1) == 3 * 64 * 512      # a plane: T * 512 bytes
    assert documented_bytes(1, 10, 64, 1024, 4) - documented_bytes(1, 10, 64, 0, 4) == 1024 * (2 * 64 + 32)      # the node pool
    for bad in ((0, 4, 8, 16, 4), (1, 0, 8, 16, 4), (1, 4, 0, 16, 4), (1, 4, 8, 0, 4), (1, 4, 8, 16, 0), (-1, 4, 8, 16, 4),
                (1, 4097, 8, 16, 4), (1, 4, 257, 16, 4), (1, 4, 8, 4097, 4), (1, 4, 8, 16, 5)):
        assert lib.magat_sim_mapf_ecbs_workspace_bytes(*bad) == 0, bad


def test_ecbs_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50

    def call(map_=one, H=20, W=20, start=one, paths=one, solved=one, status=one, hit=one, ws=one, ws_bytes=big, C=2, N=4, T=64, M=32,
             w=1500, K=4):
        return lib.magat_sim_mapf_ecbs(map_, 0, H, W, start, one, paths, one, one, solved, status, one, one, one, one, hit, ws, ws_bytes,
                                       C, N, T, M, w, K, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_ecbs"])
    assert call(map_=None) == -5 and call(start=None) == -5 and call(paths=None) == -5 and call(solved=None) == -5
    assert call(status=None) == -5 and call(hit=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1 and call(M=0) == -1
    assert call(K=0) == -1 and call(w=999) == -1 and call(w=0) == -1 and call(w=-1500) == -1
    assert call(H=65) == -2 and call(W=65) == -2 and call(T=257) == -2 and call(N=4097) == -2 and call(M=4097) == -2
    assert call(K=5) == -2 and call(w=(1 << 20) + 1) == -2
    assert call(ws_bytes=documented_bytes(2, 4, 64, 32, 4) - 1) == -2
    # the limits themselves pass: the next check is the workspace's size, then its alignment
    full = documented_bytes(2, 4096, 256, 4096, 4)
    assert call(H=64, W=64, T=256, N=4096, M=4096, w=1 << 20, ws_bytes=full - 1) == -2
    assert call(H=64, W=64, T=256, N=4096, M=4096, w=1 << 20, ws=odd, ws_bytes=full) == -3
    assert call(ws=odd) == -3 and call(H=1, W=1, T=1, N=1, C=1, M=1, K=1, w=1000, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1 and call(T=9999, ws=odd) == -2      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_ecbs"]) == before              # a refused call is not counted as a launch


def test_python_surface_on_cpu_tensors():
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    sig = inspect.signature(mapf.ecbs_cases)
    assert list(sig.parameters) == ["obstacle_map", "start", "goal", "w", "horizon", "max_nodes", "levels"]
    assert sig.parameters["w"].default == 1.5 and sig.parameters["horizon"].default is None
    assert sig.parameters["max_nodes"].default == 256 and sig.parameters["levels"].default == 4
    solve = inspect.signature(mapf.solve_cases).parameters
    assert list(solve)[-4:] == ["optimal", "bounded", "bounded_nodes", "certify"]
    assert solve["bounded"].default is None and solve["bounded_nodes"].default == 256 and solve["optimal"].default is None
    m = torch.zeros(5, 5, dtype=torch.uint8)
    cell = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.ecbs_cases(m, cell, cell)
    with pytest.raises(nat.MagatNativeError):
        mapf.solve_cases(m, cell, cell, bounded=1.5)
    for w in (0.999, 0, -2.0, float("nan"), 1049.0):
        with pytest.raises(ValueError):
            mapf.ecbs_cases(m, cell, cell, w=w)
        with pytest.raises(ValueError):
            mapf.solve_cases(m, cell, cell, bounded=w)
    with pytest.raises(ValueError, match="exclude"):
        mapf.solve_cases(m, cell, cell, optimal=16, bounded=1.5)
    # the limits are refused before anything is planned - with their own message, not the planner's
    for kw in (dict(bounded_nodes=0), dict(bounded_nodes=4097), dict(horizon=257)):
        with pytest.raises(nat.MagatNativeError, match="ecbs_cases takes"):
            mapf.solve_cases(m, cell, cell, bounded=1.5, **kw)


# ---- the kernel itself, compiled for the host: one thread per lane (tools/host_wave) ---------------------------------------------------
def _case_text(k):
    C, N, _ = k["start"].shape
    ints = [C, N, k["T"], k["map"].shape[-2], k["map"].shape[-1], k["max_nodes"], int(k["map"].ndim == 3), k["w_milli"], k["levels"]]
    for a in (k["map"], k["start"], k["goal"]):
        ints += np.asarray(a).astype(np.int64).reshape(-1).tolist()
    return " ".join(str(v) for v in ints)


@pytest.fixture(scope="module")
def ecbs_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "ecbs_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_ecbs_check.cpp"), "-o", exe], check=True)
    return exe


# (every thread rendezvous is a futex here, so the suite runs the small inputs)
@pytest.mark.parametrize("name,max_nodes,cases", [("pocket", 64, 1), ("small", 64, 6), ("r8", 8, 4), ("corner64", 64, 2)])
def test_kernel_compiled_for_the_host_equals_the_restatement(ecbs_check, tmp_path, name, max_nodes, cases):
    """The kernel with its wavefront emulated by threads and barriers, as in test_host_cbs: it covers the algorithm, the indexing
    and the barriers - not the hardware."""
    k = case(name, 1500, 4, max_nodes)
    k = tiled(k, cases)
    (tmp_path / "case.txt").write_text(_case_text(k))
    run = subprocess.run([ecbs_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key, line_ in zip(KEYS, lines[1:]):
        got = np.array(line_.split(), dtype=np.int64).reshape(np.asarray(k["want"][key]).shape)
        np.testing.assert_array_equal(got, k["want"][key], err_msg="%s: %s" % (name, key))
