"""CPU-only: the wide form of the schedule improver (csrc/sim_mapf_lns_wide.hip, improve_schedules(..., wide=True); maps up to
256 x 256, horizons up to 1024).  The yardstick is tests/lns_restatement.py on tests/mapf_restatement.py, both unchanged and
size-agnostic: what it does on the inputs of tests/test_gpu_lns_wide.py is asserted here figure by figure, so that no GPU test
can pass on a batch in which nothing happens; the inputs and the restatement's answers are made once per session and shared.
Then the host side of the entry - header / loader / build lists / workspace formula / argument checks / the `wide` keyword -
and the kernel itself compiled for the host, its workgroup of 1 to 4 wavefronts emulated by threads (tools/host_wave)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lns_restatement as lr
import mapf_restatement as mr
import test_host_wide_maps as wm
from conftest import ROOT

KEYS = ("paths", "lengths", "makespan", "flowtime_before", "flowtime_after", "accepted", "status")
RES_KEYS = ("paths", "lengths", "makespan", "solved")
ENTRIES = ("magat_sim_mapf_improve_wide_workspace_bytes", "magat_sim_mapf_improve_wide")
CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")


# ---- the inputs: name -> (map, start, goal, the schedules going in, iterations, k, the restatement's result) ---------------------
def hand_at(H, W, r0, c0):
    """lns_restatement.hand_case() moved into an otherwise walled H x W map: its 2 x 3 block at rows r0, r0 + 1, columns c0 .. c0 + 2."""
    h = lr.hand_case()
    m = np.ones((H, W), dtype=np.uint8)
    m[r0:r0 + 2, c0:c0 + 3] = h["map"]
    off = np.array([r0, c0], dtype=np.int32)
    move = lambda paths: [[(r + r0, c + c0) for r, c in p] for p in paths]      # noqa: E731
    return dict(map=m, start=h["start"] + off, goal=h["goal"] + off, before=move(h["before"]), after=move(h["after"]))


HANDS = {"hand66": (66, 66, 63, 62, 8), "hand130": (130, 130, 127, 126, 8), "hand2x3_T300": (2, 3, 0, 0, 300),
         "hand66_T300": (66, 66, 63, 62, 300)}


def long256():
    """7 x 256, walled but for row 1 columns 0 .. 254, (2, 0), row 3, (4, 126 .. 128), (4, 255), (5, 255) and row 6.  Agent 0 walks
    row 1 to its left end, down and along row 3 into its goal (4, 127) below it; agent 1 comes along row 6, up the right edge
    and back along row 3 to (3, 126): paths of 385 and 386 cells, four words wide."""
    m = np.ones((7, 256), dtype=np.uint8)
    m[1, 0:255] = 0
    m[2, 0] = 0
    m[3, :] = 0
    m[4, 126:129] = 0
    m[4, 255] = m[5, 255] = 0
    m[6, :] = 0
    return m, np.array([[[1, 254], [6, 3]]], dtype=np.int32), np.array([[[4, 127], [3, 126]]], dtype=np.int32)


CLUSTERS = {"clusters65": (52, 8, 65, 65), "clusters70x130": (61, 8, 70, 130), "clusters129": (62, 8, 129, 129),
            "clusters200": (63, 8, 200, 200), "clusters256": (64, 8, 256, 256)}
CLUSTER_FLOWTIMES = {"clusters65": (677, 650), "clusters70x130": (882, 823), "clusters129": (953, 891), "clusters200": (853, 783),
                     "clusters256": (766, 736), "maps65": (495, 470)}


def _stack_res(outs):
    return {key: np.stack([np.asarray(o[key]) for o in outs]).astype(np.uint8 if key == "solved" else np.int32) for key in RES_KEYS}


def edge_inputs():
    """A (C,66,66) batch of 2-agent cases with T = 8 around the hand case at rows 63 | 64: the hand case itself, unsolved
    (solved = 0), and the refused inputs - a length of 0, a length of T + 1, a cell at row 66, a cell on an obstacle (a map per
    case), a diagonal step."""
    h = hand_at(66, 66, 63, 62)
    first = mr.plan(h["map"], h["start"], h["goal"], None, 8)
    maps, outs = [], []
    for what in ("hand", "unsolved", "length_0", "length_T+1", "row_66", "obstacle", "diagonal"):
        o = {key: np.array(first[key]) for key in RES_KEYS}
        m = h["map"].copy()
        if what == "unsolved":
            o["solved"] = np.array(0)
        elif what == "length_0":
            o["lengths"][0] = 0
        elif what == "length_T+1":
            o["lengths"][1] = 9
        elif what == "row_66":
            o["paths"][1, 5] = (66, 62)
        elif what == "obstacle":
            m[63, 63] = 1
        elif what == "diagonal":
            o["paths"][0, 1] = (64, 62)
            o["paths"][0, 2:] = (63, 63)
        maps.append(m), outs.append(o)
    starts = np.tile(h["start"], (len(maps), 1, 1))
    goals = np.tile(h["goal"], (len(maps), 1, 1))
    return np.stack(maps), starts, goals, _stack_res(outs)


@functools.lru_cache(maxsize=None)
def case(name):
    """Treat what comes back as read-only."""
    if name in HANDS:
        H, W, r0, c0, T = HANDS[name]
        h = hand_at(H, W, r0, c0)
        m, s, g = h["map"], h["start"][None], h["goal"][None]
        res, it, k = mr.plan_batch(m, s, g, None, T), 1, 2
    elif name == "long256":
        m, s, g = long256()
        res, it, k = mr.plan_batch(m, s, g, None, 400), 1, 2
    elif name == "serpentine_T1024":
        m, s, g, _, T = wm.batch(name)
        res, it, k = wm.expected_plan(name), 1, 2
    elif name in CLUSTERS:
        seed, C, H, W = CLUSTERS[name]
        m, s, g = wm.clusters(seed, C, H, W, 12, 0.2)
        res, it, k = mr.solve_batch(m, s, g, 40, retries=8), 12, 4
    elif name == "maps65":
        m, s, g = wm.clusters(65, 6, 65, 65, 12, 0.2, batched_map=True)
        res, it, k = mr.solve_batch(m, s, g, 40, retries=8), 12, 4
    elif name == "agents70":            # 10 x 65, 70 agents on 64 threads; case 0 of the batch of two
        m, s, g = mr.random_batch(71, 2, 10, 65, 70, 0.05)
        s, g = s[:1], g[:1]
        res, it, k = mr.solve_batch(m, s, g, 120, retries=8), 8, 4
    elif name in ("edges", "edges_k8", "edges_no_iterations"):
        m, s, g, res = edge_inputs()
        it, k = {"edges": (2, 2), "edges_k8": (3, 8), "edges_no_iterations": (0, 8)}[name]
    elif name == "one_agent":           # N = 1: the seed alone, nothing to gain
        h = hand_at(66, 66, 63, 62)
        m, s, g = h["map"], h["start"][None, 1:], h["goal"][None, 1:]
        res, it, k = mr.plan_batch(m, s, g, None, 8), 3, 4
    elif name in NEWCOMER_NAMES:        # two newcomers in one step of the seed's free path (lr.newcomer_case), 66 x 20
        c, _, _, _, k = lr.newcomer_named(name, 66)
        m, s, g, res, it = c["map"], c["start"], c["goal"], c["res"], 1
    else:
        raise KeyError(name)
    return m, s, g, res, it, k, lr.improve_batch(m, res, it, k)


HAND_NAMES = tuple(HANDS)
EDGE_NAMES = ("edges", "edges_k8", "edges_no_iterations", "one_agent")
BATCH_NAMES = tuple(CLUSTERS) + ("maps65",)
NEWCOMER_NAMES = tuple(lr.newcomer_names(("one_wave", "two_waves", "two_chunks128")))
ALL_NAMES = HAND_NAMES + ("long256", "serpentine_T1024") + BATCH_NAMES + ("agents70",) + EDGE_NAMES + NEWCOMER_NAMES


def check_what_the_case_is_there_for(name):
    """The figures of the restatement alone; the GPU file calls this too, so that an input cannot quietly change under it."""
    m, s, g, res, it, k, want = case(name)
    if name in HANDS:
        H, W, r0, c0, T = HANDS[name]
        h = hand_at(H, W, r0, c0)
        assert res["solved"].tolist() == [1] and (res["paths"][0] == lr.padded(h["before"], T)).all()
        assert (want["paths"][0] == lr.padded(h["after"], T)).all() and want["lengths"].tolist() == [[3, 3]]
        assert (want["flowtime_before"].tolist(), want["flowtime_after"].tolist()) == ([5], [4])
        assert want["accepted"].tolist() == [1] and want["status"].tolist() == [0] and want["makespan"].tolist() == [2]
    elif name == "long256":
        assert res["solved"].tolist() == [1] and res["lengths"].tolist() == [[385, 386]] and want["lengths"].tolist() == [[385, 385]]
        assert (want["flowtime_before"].tolist(), want["flowtime_after"].tolist(), want["accepted"].tolist()) == ([769], [768], [1])
        assert mr.check_schedule(m, s[0], g[0], want["paths"][0], want["lengths"][0]) is None
    elif name == "serpentine_T1024":
        assert res["paths"].shape[2] == 1024 and res["lengths"].tolist() == [[425, 425]]
        assert want["accepted"].tolist() == [0] and want["status"].tolist() == [0] and (want["paths"] == res["paths"]).all()
        assert (want["lengths"] == res["lengths"]).all() and want["flowtime_after"].tolist() == [848]
    elif name in BATCH_NAMES:
        solved = res["solved"] != 0
        if name == "maps65":
            assert solved.tolist() == [0, 1, 1, 1, 1, 1] and want["status"].tolist() == [1, 0, 0, 0, 0, 0]
            for key in ("paths", "lengths", "makespan"):
                assert (want[key][0] == res[key][0]).all(), key
        else:
            assert bool(solved.all()) and want["status"].tolist() == [0] * 8
        assert (int(want["flowtime_before"].sum()), int(want["flowtime_after"].sum())) == CLUSTER_FLOWTIMES[name]
        assert int(want["accepted"].max()) > 0
        for c in np.nonzero(solved)[0]:
            hist = want["history"][c]
            assert len(hist) == it + 1 and all(hist[i + 1] <= hist[i] for i in range(it)), (c, hist)
            mc = m if m.ndim == 2 else m[c]
            assert mr.check_schedule(mc, s[c], g[c], want["paths"][c], want["lengths"][c]) is None, c
            assert want["flowtime_before"][c] == int((res["lengths"][c] - 1).sum()) == hist[0]
            assert want["flowtime_after"][c] == int((want["lengths"][c] - 1).sum()) == hist[-1]
    elif name == "agents70":
        assert res["paths"].shape[:3] == (1, 70, 120) and res["solved"].tolist() == [1]
        assert (want["flowtime_before"].tolist(), want["flowtime_after"].tolist(), want["accepted"].tolist()) == ([2204], [2193], [1])
        assert mr.check_schedule(m, s[0], g[0], want["paths"][0], want["lengths"][0]) is None
    elif name in ("edges", "edges_k8", "edges_no_iterations"):
        assert want["status"].tolist() == [0, 1, 2, 2, 2, 2, 2]
        assert want["accepted"].tolist() == [0 if name == "edges_no_iterations" else 1] + [0] * 6
        assert want["flowtime_before"].tolist() == [5] + [0] * 6
        assert want["flowtime_after"].tolist() == [5 if name == "edges_no_iterations" else 4] + [0] * 6
        for key in ("paths", "lengths", "makespan"):
            assert (want[key][1:] == res[key][1:]).all(), key      # skipped and refused: bit-equal
    elif name == "one_agent":
        assert want["status"].tolist() == [0] and want["accepted"].tolist() == [0] and (want["paths"] == res["paths"]).all()
        assert want["flowtime_before"].tolist() == want["flowtime_after"].tolist() == [2]
    elif name in NEWCOMER_NAMES:
        import test_host_lns as th
        th.check_newcomers(name, 66, want)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_restatement_on_the_wide_inputs(name):
    check_what_the_case_is_there_for(name)


# ---- the host side of the entry ------------------------------------------------------------------------------------------------
def documented_workspace_bytes(C, H, W, N, T):
    """include/magat_hip.h: C * (T * 6 * rows(H) * words(W) * 8 + 8 * ceil(N / 2))."""
    return C * (T * 6 * (64 * -(-H // 64)) * (1 if W <= 64 else 2 if W <= 128 else 4) * 8 + 8 * -(-N // 2))


def test_wide_improve_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert "sim_mapf_lns_wide.hip" in build_native.SOURCES and "sim_mapf_wide_parts.h" in build_native.HEADERS
    assert re.search(r"^size_t magat_sim_mapf_improve_wide_workspace_bytes\(int C, int H, int W, int N, int T\);", hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_improve_wide\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    assert nat._SIGNATURES["magat_sim_mapf_improve_wide"] == nat._SIGNATURES["magat_sim_mapf_improve"]      # the same arguments
    assert len(nat._SIGNATURES["magat_sim_mapf_improve_wide_workspace_bytes"][1]) == 5
    text = open(os.path.join(CSRC, "sim_mapf_lns_wide.hip")).read()
    assert "MAGAT_FORM_SIM_MAPF_LNS" in text and "MAGAT_TAG_SIM_MAPF_LNS" in text      # the 64 form's counter and tag
    assert "asm" not in text and "struct wboard" not in text
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_wide_search_helpers_have_one_home():
    for name in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, name)).read()
        for helper in ("wmapf_search", "wmapf_backtrace"):
            defined = len(re.findall(r"\b%s\s*\([^;{]*\)\s*\{" % helper, text))
            assert defined == (1 if name == "sim_mapf_wide_parts.h" else 0), (name, helper)
        assert len(re.findall(r"\bstruct wide_layers\b", text)) == (1 if name == "sim_mapf_wide_parts.h" else 0), name
    for user in ("sim_mapf_wide.hip", "sim_mapf_lns_wide.hip"):
        assert '#include "sim_mapf_wide_parts.h"' in open(os.path.join(CSRC, user)).read()


def test_wide_improve_workspace_formula():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for C, H, W, N, T in ((1, 65, 65, 12, 40), (3, 10, 65, 70, 120), (2, 70, 130, 9, 24), (1, 129, 129, 1, 16), (8, 200, 200, 1000, 1024),
                          (1, 256, 256, 4096, 1024), (4, 2, 3, 2, 300), (1, 64, 192, 7, 7), (1, 193, 64, 8, 7)):
        assert lib.magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T) == documented_workspace_bytes(C, H, W, N, T), (C, H, W, N, T)
    assert documented_workspace_bytes(3, 65, 65, 9, 40) == documented_workspace_bytes(3, 65, 65, 10, 40) == 3 * (40 * 6 * 128 * 2 * 8 + 40)
    assert lib.magat_sim_mapf_improve_wide_workspace_bytes(3, 65, 65, 9, 40) == 3 * (40 * 6 * 128 * 2 * 8 + 40)      # d0 padded to 8 bytes
    # behind the layers of the wide planner sits d0 alone
    assert (lib.magat_sim_mapf_improve_wide_workspace_bytes(2, 70, 130, 5, 24) - lib.magat_sim_mapf_wide_workspace_bytes(2, 70, 130, 24)
            == 2 * 8 * 3)
    for bad in ((0, 65, 65, 4, 8), (1, 0, 65, 4, 8), (1, 65, -1, 4, 8), (1, 65, 65, 0, 8), (1, 65, 65, 4, 0), (1, 257, 65, 4, 8),
                (1, 65, 257, 4, 8)):
        assert lib.magat_sim_mapf_improve_wide_workspace_bytes(*bad) == 0, bad


def test_wide_improve_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50

    def call(map_=one, H=200, W=200, solved=one, paths=one, status=one, ws=one, ws_bytes=big, C=2, N=4, T=512, it=8, k=3):
        return lib.magat_sim_mapf_improve_wide(map_, 0, H, W, solved, paths, one, one, one, one, one, status, ws, ws_bytes, C, N, T,
                                               it, k, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_lns"])
    assert call(map_=None) == -5 and call(solved=None) == -5 and call(paths=None) == -5 and call(status=None) == -5
    assert call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1
    assert call(H=257) == -2 and call(W=257) == -2 and call(T=1025) == -2
    assert call(k=0) == -2 and call(k=9) == -2 and call(it=-1) == -2 and call(it=4097) == -2
    assert call(ws_bytes=documented_workspace_bytes(2, 200, 200, 4, 512) - 1) == -2
    # 256 x 256, T = 1024, k = 8 and 4096 iterations pass the limits: the next check is the workspace's size, then its alignment
    full = documented_workspace_bytes(2, 256, 256, 4, 1024)
    assert call(H=256, W=256, T=1024, k=8, it=4096, ws_bytes=full - 1) == -2
    assert call(H=256, W=256, T=1024, k=8, it=4096, ws=odd, ws_bytes=full) == -3
    assert call(H=65, W=65, T=257, ws=odd) == -3 and call(H=1, W=1, T=1, it=0, k=1, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1 and call(T=9999, k=0, ws=odd) == -2      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_lns"]) == before              # a refused call is not counted as a launch
    # the 64 form keeps its own limits
    assert lib.magat_sim_mapf_improve(one, 0, 65, 20, one, one, one, one, one, one, one, one, one, big, 2, 4, 64, 8, 3, None) == -2
    assert lib.magat_sim_mapf_improve(one, 0, 20, 20, one, one, one, one, one, one, one, one, one, big, 2, 4, 257, 8, 3, None) == -2


def test_wide_keyword_on_cpu_tensors_raises():
    import inspect
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    sig = inspect.signature(mapf.improve_schedules)
    assert list(sig.parameters) == ["obstacle_map", "res", "iterations", "neighbourhood", "wide"]
    assert sig.parameters["wide"].default is False and sig.parameters["iterations"].default == 32
    m = torch.zeros(70, 70, dtype=torch.uint8)
    res = dict(paths=torch.zeros(1, 2, 300, 2, dtype=torch.int32), lengths=torch.ones(1, 2, dtype=torch.int32),
               makespan=torch.zeros(1, dtype=torch.int32), solved=torch.ones(1, dtype=torch.uint8))
    with pytest.raises(nat.MagatNativeError):
        mapf.improve_schedules(m, res, wide=True)
    with pytest.raises(nat.MagatNativeError):
        mapf.improve_schedules(m, res, iterations=4, neighbourhood=2, wide=True)
    s = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.solve_cases(m, s, s, wide=True, improve=4)


# ---- the kernel itself, compiled for the host: one thread per lane, 1 to 4 wavefronts (tools/host_wave) ---------------------------
def _case_text(m, res, iterations, k):
    C, N, T, _ = res["paths"].shape
    ints = [C, N, T, m.shape[-2], m.shape[-1], iterations, k, int(m.ndim == 3)]
    for a in (m, res["solved"], res["paths"], res["lengths"], res["makespan"]):
        ints += np.asarray(a).astype(np.int64).reshape(-1).tolist()
    return " ".join(str(v) for v in ints)


@pytest.fixture(scope="module")
def wide_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "lns_wide_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_lns_wide_check.cpp"), "-o", exe], check=True)
    return exe


def _run_and_compare(wide_check, tmp_path, name, m, res, it, k, want):
    (tmp_path / "case.txt").write_text(_case_text(m, res, it, k))
    run = subprocess.run([wide_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key, line in zip(KEYS, lines[1:]):
        got = np.array(line.split(), dtype=np.int64).reshape(np.asarray(want[key]).shape)
        np.testing.assert_array_equal(got, want[key], err_msg="%s: %s" % (name, key))


def narrow_names():
    import test_gpu_lns as tg
    return ["edges", "hand_k1", "hand_k8_no_iterations", "hand_k8", "start_is_goal", "corner64"] + tg.NEWCOMER_NAMES


@pytest.mark.parametrize("name", narrow_names())
def test_wide_kernel_compiled_for_the_host_on_the_narrow_inputs(wide_check, tmp_path, name):
    """improve_schedules(..., wide=True) sends a shape inside 64 x 64 to the 64 form, so the wide kernel never meets the narrow
    one's inputs through it; here it does, through its entry: one wavefront, one word, and the results of the restatement - which
    are what tests/test_host_lns.py asks of the narrow kernel on the same case texts."""
    import test_gpu_lns as tg
    m, res, it, k, want = tg.case(name)
    _run_and_compare(wide_check, tmp_path, name, m, res, it, k, want)


@pytest.mark.parametrize("name", HAND_NAMES + ("long256",) + EDGE_NAMES + ("clusters65",) + NEWCOMER_NAMES)
def test_wide_kernel_compiled_for_the_host_equals_the_restatement(wide_check, tmp_path, name):
    """csrc/sim_mapf_lns_wide.hip with its workgroup emulated by threads and barriers - ballot, DPP shift, readfirstlane and
    shuffle as exchanges inside a wavefront, __syncthreads across the workgroup: 1, 2 and 3 wavefronts, 1, 2 and 4 words.  It
    covers the algorithm, the indexing and the barriers - not the hardware."""
    m, _, _, res, it, k, want = case(name)
    _run_and_compare(wide_check, tmp_path, name, m, res, it, k, want)
