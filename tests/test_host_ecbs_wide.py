"""CPU-only: the wide form of ECBS (csrc/sim_mapf_ecbs_wide.hip, mapf.ecbs_cases_wide) and mapf.adopt_bounded.  The yardstick is
tests/ecbs_restatement.py, unchanged - it knows no map widths.  It is slow (per-cell loops), so the inputs are strips and small agent
counts: the smallest shapes at which each piece of the wide layout can go wrong - a second and a third wavefront, two and four
words per row, a row or a column next to a wavefront's or a word's edge, a horizon above 256.  The inputs of
tests/test_gpu_ecbs_wide.py are made here (once per session, with the restatement's answer), each with an assertion of what it
is there for.  Then the host side of the entries - header / loader / build lists / workspace formula / argument checks -, the
Python surface on CPU tensors, and the kernel compiled for the host, its workgroup emulated by threads (tools/host_wave)."""
import ctypes
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cbs_restatement as cr
import ecbs_restatement as er
import mapf_restatement as mr
import test_host_cbs as hc
import test_host_ecbs as he
from conftest import ROOT

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
ENTRIES = ("magat_sim_mapf_ecbs_wide_workspace_bytes", "magat_sim_mapf_ecbs_wide")
KEYS = hc.KEYS
CROWD = ((1000, 4, 64), (1200, 2, 64), (1500, 1, 64), (1500, 3, 8))      # crowd66x5 at (w_milli, levels, max_nodes)
# the inputs of the GPU tests, at (w_milli, levels, max_nodes)
GPU_INPUTS = (("tall65x8", 1500, 4, 64), ("wide8x65", 1500, 4, 64), ("wide8x129", 1500, 4, 64), ("tall129x6", 1500, 4, 64),
              ("corner65", 1500, 2, 64), ("serpentine_T400", 1050, 4, 64), ("small65", 1500, 4, 64)) + tuple(("crowd66x5",) + key
                                                                                                            for key in CROWD)


def _strip(seed, C, H, W, N, density, T, far):
    """C cases on ONE random H x W map: starts and goals drawn from its largest free component, but agent 0 of every case goes
    from the component's first cell to its last one in row-major (far: "rows") or column-major (far: "columns") order - along
    the whole strip."""
    rng = np.random.default_rng(seed)
    m, _, _ = mr.random_case(rng, H, W, N, density)
    cells = mr.largest_component(m == 0)
    order = cells if far == "rows" else cells[np.lexsort((cells[:, 0], cells[:, 1]))]
    ends = {tuple(order[0]), tuple(order[-1])}
    rest = np.array([cell for cell in cells if tuple(cell) not in ends])
    start = np.stack([np.concatenate([order[:1], rest[rng.permutation(len(rest))[:N - 1]]]) for _ in range(C)])
    goal = np.stack([np.concatenate([order[-1:], rest[rng.permutation(len(rest))[:N - 1]]]) for _ in range(C)])
    return hc._case(m, start, goal, T, 0)


def corner65():
    """An open 65 x 65 map, two agents that exchange the corners (0, 0) and (64, 64): row 64 is the second wavefront's only row,
    column 64 the second word's only bit."""
    return hc._case(np.zeros((65, 65), dtype=np.uint8), [[(0, 0), (64, 64)]], [[(64, 64), (0, 0)]], 200, 0)


def serpentine_T400():
    """A 9 x 65 serpentine (and a tenth row below it): agent 0 walks its whole length, 5 * 64 + 8 = 328 steps, to (8, 64); agent 1
    is parked on (8, 30), in its way on the last leg, which is two wide there (row 9 is open from column 28 to 32, and only there):
    one of them goes round the other."""
    m = np.zeros((10, 65), dtype=np.uint8)
    for r in range(1, 9, 2):
        m[r, :] = 1
        m[r, 64 if (r // 2) % 2 == 0 else 0] = 0
    m[9, :] = 1
    m[9, 28:33] = 0
    return hc._case(m, [[(0, 0), (8, 30)]], [[(8, 64), (8, 30)]], 400, 0)


def small65():
    """test_host_cbs's small batch on 65-row maps - the 3 x 5 rooms in the LAST three rows, 62 rows of obstacles above them: the
    pocket swap with the parked agent; a goal in another component (status 2 with horizon_hit); then status 3 for a shared start, a
    shared goal, a start off the map and a goal on an obstacle."""
    k = hc.small_batch()
    maps = np.ones((len(k["map"]), 65, 5), dtype=np.uint8)
    maps[:, 62:] = k["map"]
    shift = np.array([62, 0], dtype=np.int32)
    return hc._case(maps, k["start"] + shift, k["goal"] + shift, 16, 0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    if name == "tall65x8":
        return _strip(65, 2, 65, 8, 6, 0.1, 160, "rows")
    if name == "wide8x65":
        return _strip(66, 2, 8, 65, 6, 0.1, 160, "columns")
    if name == "wide8x129":
        return _strip(129, 1, 8, 129, 6, 0.1, 300, "columns")
    if name == "tall129x6":
        return _strip(130, 1, 129, 6, 6, 0.1, 300, "rows")
    if name == "corner65":
        return corner65()
    if name == "serpentine_T400":
        return serpentine_T400()
    if name == "small65":
        return small65()
    if name == "crowd66x5":
        return hc._case(*mr.random_batch(665, 4, 66, 5, 10, 0.15), 120, 0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, w_milli, levels, max_nodes):
    k = inputs(name)
    k = dict(map=k["map"], start=k["start"], goal=k["goal"], T=k["T"], max_nodes=max_nodes, w_milli=w_milli, levels=levels)
    k["want"] = er.ecbs_batch(k["map"], k["start"], k["goal"], k["T"], w_milli, max_nodes, levels)
    return k


def _crosses(path, length, axis, a, b):
    """the path steps between coordinate a and b = a + 1 of the axis (0: rows, 1: columns)"""
    line = np.asarray(path)[:length, axis]
    return bool(((line[:-1] == a) & (line[1:] == b)).any() or ((line[:-1] == b) & (line[1:] == a)).any())


@pytest.mark.parametrize("name,w_milli,levels,max_nodes", GPU_INPUTS)
def test_inputs_of_the_gpu_tests(name, w_milli, levels, max_nodes):
    k = case(name, w_milli, levels, max_nodes)
    he.check_consistent(k)
    w = k["want"]
    H, W = k["map"].shape[-2:]
    assert max(H, W) >= 65
    if name in ("tall65x8", "wide8x65", "wide8x129", "tall129x6"):
        assert k["map"].ndim == 2 and (w["status"] == 0).all(), w["status"].tolist()
        axis = 0 if name.startswith("tall") else 1
        for c in range(len(k["start"])):      # agent 0 goes along the whole strip: over every wavefront's / word's edge
            for edge in range(63, max(H, W) - 1, 64):
                assert _crosses(w["paths"][c, 0], w["lengths"][c, 0], axis, edge, edge + 1), (name, c, edge)
    if name == "tall65x8":
        assert (H, W) == (65, 8)          # a second wavefront, one word
    if name == "wide8x65":
        assert (H, W) == (8, 65)                           # one wavefront, two words
    if name == "wide8x129":
        assert (H, W) == (8, 129)                          # four words: columns 63 / 64 and 127 / 128 are crossed (above)
    if name == "tall129x6":
        assert (H, W) == (129, 6)                          # three wavefronts: rows 63 / 64 and 127 / 128 are crossed (above)
    if name == "corner65":
        assert w["status"].tolist() == [0] and w["lengths"].tolist() == [[129, 129]] and k["map"].shape == (65, 65)
        assert w["paths"][0, 0, 128].tolist() == [64, 64] and w["paths"][0, 1, 128].tolist() == [0, 0]
    if name == "serpentine_T400":      # T > 256, a length that needs 10 bits, the window b = 1.05 t* reaches past t*, one expansion
        assert k["T"] == 400 and w["status"].tolist() == [0] and w["lengths"][0, 0] - 1 >= 328 and 1050 * 328 // 1000 > 328
        assert w["lengths"][0, 0] > 256 and w["nodes"][0] >= 3
    if name == "small65":
        assert w["status"].tolist() == [0, 2, 3, 3, 3, 3] and w["horizon_hit"].tolist() == [0, 1, 0, 0, 0, 0]
        assert w["nodes"].tolist()[1:] == [0] * 5
    if (name, levels, max_nodes) == ("crowd66x5", 3, 8):
        assert int((w["status"] == 1).sum()) > 0


def test_the_crowd_is_where_the_trees_are():
    """Over crowd66x5's four settings: a tree of at least 7 nodes; at w = 1 the flowtime of conflict-based search."""
    k = inputs("crowd66x5")
    assert k["map"].shape == (66, 5) and 8 <= k["start"].shape[1] <= 10 and k["map"].any()
    assert max(int(case("crowd66x5", *key)["want"]["nodes"].max()) for key in CROWD) >= 7
    one = case("crowd66x5", 1000, 4, 64)["want"]
    opt = cr.cbs_batch(k["map"], k["start"], k["goal"], k["T"], 64)
    both = (one["status"] == 0) & (opt["status"] == 0)
    assert int(both.sum()) > 0
    np.testing.assert_array_equal(one["flowtime"][both], opt["flowtime"][both])


# ---- the host side of the entries -----------------------------------------------------------------------------------------------------
def documented_bytes(C, H, W, N, T, M, K):
    rows, words = 64 * ((H + 63) // 64), 1 if W <= 64 else 2 if W <= 128 else 4
    return C * 8 * (T * rows * words * (10 + K) + (N * T + 3) // 4 + (M * T + 3) // 4 + 4 * M + (5 * N + 1) // 2 + H * W)


def test_wide_ecbs_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert "sim_mapf_ecbs_wide.hip" in build_native.SOURCES and "sim_mapf_ecbs_parts.h" in build_native.HEADERS
    text = open(os.path.join(CSRC, "sim_mapf_ecbs_wide.hip")).read()
    narrow = open(os.path.join(CSRC, "sim_mapf_ecbs.hip")).read()
    parts = open(os.path.join(CSRC, "sim_mapf_ecbs_parts.h")).read()
    assert "MAGAT_FORM_SIM_MAPF_ECBS" in text and "MAGAT_TAG_SIM_MAPF_ECBS" in text
    for part in ("sim_mapf_wide_parts.h", "sim_mapf_audit_parts.h", "sim_mapf_cbs_parts.h", "sim_mapf_ecbs_parts.h", "sim_mapf_tree.h",
                 "row_board.h"):
        assert '#include "%s"' % part in text and part in build_native.HEADERS
    assert '#include "sim_mapf_ecbs_parts.h"' in narrow
    tree = open(os.path.join(CSRC, "sim_mapf_tree.h")).read()
    board = open(os.path.join(CSRC, "row_board.h")).read()
    assert re.search(r"\bwave_all_sum\(", board) and "ecbs_wave_sum" not in parts + text + narrow + tree      # the sum: with the row boards
    assert "mapf_tree_search(" in text and "mapf_tree_search(" in narrow and "audit_stage2(" in tree      # the walk, once for both forms
    for shared in ("ecbs_node", "ecbs_count", "ECBS_MAX_NODES"):      # one copy, in the shared header
        assert re.search(r"\b%s\b" % shared, parts), shared
        for body in (text, narrow):
            assert not re.search(r"^(struct|__device__ [^\n]*|template[^\n]*\n__device__ [^\n]*|constexpr int) ?\b%s\b[ ({=]" % shared, body,
                                 re.M), shared
    assert "audit_stage2(" not in text and "asm" not in text and "printf" not in text and "assert(" not in text
    assert "hipDeviceSynchronize" not in text
    assert re.search(r"^size_t magat_sim_mapf_ecbs_wide_workspace_bytes\(int C, int H, int W, int N, int T, int max_nodes, int levels\);",
                     hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_ecbs_wide\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    assert nat._SIGNATURES["magat_sim_mapf_ecbs_wide"] == nat._SIGNATURES["magat_sim_mapf_ecbs"]      # exactly its argument list
    assert len(nat._SIGNATURES["magat_sim_mapf_ecbs_wide_workspace_bytes"][1]) == 7
    for name in ("ecbs_cases_wide", "adopt_bounded"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_wide_ecbs_workspace_formula():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for shape in ((1, 1, 1, 1, 1, 1, 1), (32, 65, 65, 100, 360, 256, 4), (4, 160, 160, 1000, 1024, 256, 4), (300, 66, 5, 9, 120, 64, 3),
                  (2, 256, 256, 4096, 1024, 4096, 4), (3, 8, 129, 6, 300, 5, 2), (5, 64, 64, 7, 257, 9, 1)):
        assert lib.magat_sim_mapf_ecbs_wide_workspace_bytes(*shape) == documented_bytes(*shape), shape
    # a plane: T * rows * words * 8 bytes; the grids: 8 * H * W
    assert documented_bytes(1, 65, 129, 10, 64, 64, 4) - documented_bytes(1, 65, 129, 10, 64, 64, 1) == 3 * 64 * 128 * 4 * 8
    assert documented_bytes(1, 65, 64, 10, 64, 64, 4) - documented_bytes(1, 65, 63, 10, 64, 64, 4) == 8 * 65
    for bad in ((0, 9, 9, 4, 8, 16, 4), (1, 0, 9, 4, 8, 16, 4), (1, 9, 0, 4, 8, 16, 4), (1, 9, 9, 0, 8, 16, 4), (1, 9, 9, 4, 0, 16, 4),
                (1, 9, 9, 4, 8, 0, 4), (1, 9, 9, 4, 8, 16, 0), (-1, 9, 9, 4, 8, 16, 4), (1, 257, 9, 4, 8, 16, 4), (1, 9, 257, 4, 8, 16, 4),
                (1, 9, 9, 4097, 8, 16, 4), (1, 9, 9, 4, 1025, 16, 4), (1, 9, 9, 4, 8, 4097, 4), (1, 9, 9, 4, 8, 16, 5)):
        assert lib.magat_sim_mapf_ecbs_wide_workspace_bytes(*bad) == 0, bad


def test_wide_ecbs_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50

    def call(map_=one, H=70, W=70, start=one, paths=one, solved=one, status=one, hit=one, ws=one, ws_bytes=big, C=2, N=4, T=300, M=32,
             w=1500, K=4):
        return lib.magat_sim_mapf_ecbs_wide(map_, 0, H, W, start, one, paths, one, one, solved, status, one, one, one, one, hit, ws,
                                            ws_bytes, C, N, T, M, w, K, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_ecbs"])
    assert call(map_=None) == -5 and call(start=None) == -5 and call(paths=None) == -5 and call(solved=None) == -5
    assert call(status=None) == -5 and call(hit=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1 and call(M=0) == -1
    assert call(K=0) == -1 and call(w=999) == -1 and call(w=0) == -1 and call(w=-1500) == -1
    assert call(H=257) == -2 and call(W=257) == -2 and call(T=1025) == -2 and call(N=4097) == -2 and call(M=4097) == -2
    assert call(K=5) == -2 and call(w=(1 << 20) + 1) == -2
    assert call(ws_bytes=documented_bytes(2, 70, 70, 4, 300, 32, 4) - 1) == -2
    # the limits themselves pass: the next check is the workspace's size, then its alignment
    full = documented_bytes(2, 256, 256, 4096, 1024, 4096, 4)
    assert call(H=256, W=256, T=1024, N=4096, M=4096, w=1 << 20, ws_bytes=full - 1) == -2
    assert call(H=256, W=256, T=1024, N=4096, M=4096, w=1 << 20, ws=odd, ws_bytes=full) == -3
    assert call(ws=odd) == -3 and call(H=1, W=1, T=1, N=1, C=1, M=1, K=1, w=1000, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1 and call(T=9999, ws=odd) == -2      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_ecbs"]) == before              # a refused call is not counted as a launch


def test_python_surface_on_cpu_tensors():
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    sig = inspect.signature(mapf.ecbs_cases_wide)
    assert list(sig.parameters) == list(inspect.signature(mapf.ecbs_cases).parameters)
    assert list(sig.parameters) == ["obstacle_map", "start", "goal", "w", "horizon", "max_nodes", "levels"]
    assert sig.parameters["w"].default == 1.5 and sig.parameters["horizon"].default is None
    assert sig.parameters["max_nodes"].default == 256 and sig.parameters["levels"].default == 4
    assert list(inspect.signature(mapf.adopt_bounded).parameters) == ["res", "sub"]
    solve = inspect.signature(mapf.solve_cases).parameters      # today's parameter lists stay
    assert list(solve) == ["obstacle_map", "start", "goal", "horizon", "retries", "wide", "improve", "optimal", "bounded", "bounded_nodes",
                           "certify"]
    m = torch.zeros(65, 5, dtype=torch.uint8)
    cell = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.ecbs_cases_wide(m, cell, cell)
    for w in (0.999, 0, -2.0, float("nan"), 1049.0):
        with pytest.raises(ValueError):
            mapf.ecbs_cases_wide(m, cell, cell, w=w)
    assert "ecbs_cases_wide" in mapf.__doc__ and "adopt_bounded" in mapf.__doc__
    assert "bytes per case" in mapf.ecbs_cases_wide.__doc__ and "no wide form" not in mapf.ecbs_cases_wide.__doc__
    with pytest.raises(nat.MagatNativeError, match="64 x 64"):      # the narrow name refuses as before
        mapf.solve_cases(m, cell, cell, wide=True, bounded=1.5)


def _res(paths, lengths, solved, **more):
    import torch
    paths = torch.tensor(paths, dtype=torch.int32)
    lengths = torch.tensor(lengths, dtype=torch.int32)
    out = dict(paths=paths, lengths=lengths, makespan=lengths.max(1).values - 1, solved=torch.tensor(solved, dtype=torch.uint8),
               start=paths[:, :, 0].clone(), goal=paths[:, :, -1].clone())
    out.update({key: torch.tensor(value, dtype=torch.int32) for key, value in more.items()})
    return out


def test_adopt_bounded_on_hand_made_dicts():
    """Four cases of one agent, T = 4: an unsolved plan and a solved search - taken; a plan with a larger flowtime - taken; a plan
    with the same flowtime - kept; a search that ran out of its budget - kept.  Tensor ops only: CPU tensors will do."""
    import torch
    from magat_pathplanning_amd import mapf
    walk = [[(0, 0), (0, 1), (0, 2), (0, 3)]]
    short = [[(0, 0), (0, 1), (0, 3), (0, 3)]]      # (only told apart here)
    park = [[(0, 0), (0, 0), (0, 0), (0, 0)]]
    res = _res([park, walk, walk, walk], [[1], [4], [4], [4]], [0, 1, 1, 1], failed_agent=[0, -1, -1, -1])
    sub = _res([walk, short, short, park], [[4], [3], [4], [1]], [1, 1, 1, 0], status=[0, 0, 0, 1], flowtime=[3, 2, 3, -1],
               lower_bound=[3, 2, 3, 2], nodes=[1, 3, 5, 8], horizon_hit=[0, 1, 0, 0])
    before = {key: value.clone() for key, value in res.items()}
    out = mapf.adopt_bounded(res, sub)
    assert out["solved"].tolist() == [1, 1, 1, 1] and out["failed_agent"].tolist() == [-1, -1, -1, -1]
    assert out["lengths"].tolist() == [[4], [3], [4], [4]] and out["makespan"].tolist() == [3, 2, 3, 3]
    assert out["paths"].tolist() == _res([walk, short, walk, walk], [[4], [3], [4], [4]], [1] * 4)["paths"].tolist()
    assert out["ecbs_status"].tolist() == [0, 0, 0, 1] and out["ecbs_bound"].tolist() == [3, -1, 3, 2]
    assert out["ecbs_nodes"].tolist() == [1, 3, 5, 8] and out["bounded"].tolist() == [True, True, True, False]
    assert out["bounded"].dtype == torch.bool and out["paths"].dtype == torch.int32 and out["solved"].dtype == torch.uint8
    for key, value in before.items():      # the inputs are not modified
        assert torch.equal(res[key], value), key
    with pytest.raises(ValueError, match="horizon"):
        mapf.adopt_bounded(res, dict(sub, paths=sub["paths"][:, :, :3]))


# ---- the kernel itself, compiled for the host: one thread per lane (tools/host_wave) ---------------------------------------------------
@pytest.fixture(scope="module")
def ecbs_wide_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "ecbs_wide_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_ecbs_wide_check.cpp"), "-o", exe], check=True)
    return exe


# (every thread rendezvous is a futex here, so the suite runs the small inputs)
@pytest.mark.parametrize("name,key,cases", [("tall65x8", (1500, 4, 64), 1), ("wide8x65", (1500, 4, 64), 1), ("small65", (1500, 4, 64), 6),
                                            ("crowd66x5", (1500, 3, 8), 4)])
def test_kernel_compiled_for_the_host_equals_the_restatement(ecbs_wide_check, tmp_path, name, key, cases):
    """The kernel with its workgroup emulated by threads and barriers, as in test_host_ecbs: it covers the algorithm, the indexing
    and the barriers - not the hardware."""
    k = he.tiled(case(name, *key), cases)
    (tmp_path / "case.txt").write_text(he._case_text(k))
    run = subprocess.run([ecbs_wide_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key_, line_ in zip(KEYS, lines[1:]):
        got = np.array(line_.split(), dtype=np.int64).reshape(np.asarray(k["want"][key_]).shape)
        np.testing.assert_array_equal(got, k["want"][key_], err_msg="%s: %s" % (name, key_))


@pytest.mark.parametrize("name,key", [("pocket", (1500, 4, 64)), ("r8", (1500, 3, 8))])
def test_the_forms_agree_where_both_apply(ecbs_wide_check, tmp_path, name, key):
    """One walk, two forms: the wide kernel on a narrow shape (its entry refuses only above 256) gives the restatement's answer,
    which is what the narrow kernel is held to (test_host_ecbs)."""
    k = he.case(name, *key)
    (tmp_path / "case.txt").write_text(he._case_text(k))
    run = subprocess.run([ecbs_wide_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key_, line_ in zip(KEYS, lines[1:]):
        got = np.array(line_.split(), dtype=np.int64).reshape(np.asarray(k["want"][key_]).shape)
        np.testing.assert_array_equal(got, k["want"][key_], err_msg="%s: %s" % (name, key_))
