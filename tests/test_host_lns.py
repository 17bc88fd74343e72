"""CPU-only: the restatement of the schedule improver (tests/lns_restatement.py; the yardstick of tests/test_gpu_lns.py) -
its two properties on random batches, a hand case with the expected schedule written out, and the edge cases - and the host
side of the new entry: header / loader / build list / argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import lns_restatement as lr
import mapf_restatement as mr
from conftest import ROOT


@pytest.mark.parametrize("name", list(lr.BATCHES))
def test_flowtime_never_rises_schedules_stay_valid_and_the_batch_total_drops(name):
    b = lr.BATCHES[name]
    m, start, goal, res, out = lr.solved_and_improved(name)
    assert int(res["solved"].sum()) == len(start)
    for c in range(len(start)):
        h = out["history"][c]
        assert len(h) == b["iterations"] + 1 and all(h[i + 1] <= h[i] for i in range(len(h) - 1)), (c, h)
        assert mr.check_schedule(m, start[c], goal[c], out["paths"][c], out["lengths"][c]) is None, c
        assert out["status"][c] == 0 and out["flowtime_before"][c] == int((res["lengths"][c] - 1).sum()) == h[0]
        assert out["flowtime_after"][c] == int((out["lengths"][c] - 1).sum()) == h[-1]
        assert out["makespan"][c] == out["lengths"][c].max() - 1
        assert (out["accepted"][c] > 0) == (h[-1] < h[0])
    print(name, "sum of lengths", int(res["lengths"].sum()), "->", int(out["lengths"].sum()))
    assert int(out["flowtime_after"].sum()) < int(out["flowtime_before"].sum())


def _hand(iterations=1, k=2):
    h = lr.hand_case()
    first = mr.plan(h["map"], h["start"], h["goal"], None, h["T"])
    out = lr.improve(h["map"], first["paths"], first["lengths"], first["makespan"], first["solved"], iterations, k)
    return h, first, out


def test_hand_case_one_iteration_swaps_the_detour_for_a_way_round():
    h, first, out = _hand()
    assert first["solved"] == 1 and (first["paths"] == lr.padded(h["before"], h["T"])).all()
    assert first["lengths"].tolist() == [3, 4]
    assert (out["paths"] == lr.padded(h["after"], h["T"])).all() and out["lengths"].tolist() == [3, 3]
    assert (out["flowtime_before"], out["flowtime_after"], out["accepted"], out["status"]) == (5, 4, 1, 0)
    assert out["makespan"] == 2 and out["history"] == [5, 4]
    assert mr.check_schedule(h["map"], h["start"], h["goal"], out["paths"], out["lengths"]) is None


def test_neighbourhood_rule():
    cells = [[(0, 0), (0, 1), (1, 1)], [(0, 2), (0, 2), (0, 1), (0, 0)], [(1, 2)]]
    free1 = [(0, 2), (0, 1), (0, 0)]
    assert lr.neighbourhood(1, free1, cells, 2) == [1, 0]               # agent 0 stands on (0, 1) at t = 1
    assert lr.neighbourhood(1, free1, cells, 3) == [1, 0, 2]            # ... and the fill goes on at seed + 1
    assert lr.neighbourhood(1, free1, cells, 1) == [1] and lr.neighbourhood(1, free1, cells, 9) == [1, 0, 2]
    assert lr.neighbourhood(2, [(1, 2)], cells, 2) == [2, 0]            # nobody in the way: seed + 1 (mod N)
    # a swap: agent 0 walks (0,0) -> (0,1) while the free path walks (0,1) -> (0,0) in the same step
    assert lr.neighbourhood(1, [(0, 1), (0, 0)], [[(0, 0), (0, 1)], [(0, 1), (0, 1), (0, 0)], [(1, 2)]], 2) == [1, 0]


def test_edge_cases():
    h, first, out0 = _hand(iterations=0)
    assert out0["accepted"] == 0 and out0["status"] == 0 and out0["history"] == [5] and out0["flowtime_after"] == 5
    assert (out0["paths"] == first["paths"]).all() and out0["makespan"] == first["makespan"] == 3
    _, _, out1 = _hand(iterations=4, k=1)                                   # an agent re-planned alone cannot gain
    assert out1["accepted"] == 0 and (out1["paths"] == first["paths"]).all() and out1["history"] == [5] * 5
    _, _, out9 = _hand(iterations=3, k=9)                                   # k > N: the neighbourhood is everybody
    assert out9["lengths"].tolist() == [3, 3] and out9["accepted"] == 1 and out9["history"] == [5, 4, 4, 4]
    k = mr.hand_cases()["start_is_goal"]
    home = mr.plan(k["map"], k["start"], k["goal"], None, k["T"])
    out = lr.improve(k["map"], home["paths"], home["lengths"], home["makespan"], home["solved"], 3, 2)
    assert out["status"] == 0 and out["accepted"] == 0 and out["flowtime_before"] == out["flowtime_after"] == 0
    assert (out["paths"] == home["paths"]).all() and out["makespan"] == 0


def test_unsolved_and_refused_inputs_come_back_as_they_came():
    k = mr.hand_cases()["head_on_closed"]
    bad = mr.plan(k["map"], k["start"], k["goal"], None, k["T"])
    out = lr.improve(k["map"], bad["paths"], bad["lengths"], bad["makespan"], bad["solved"], 4, 2)
    assert bad["solved"] == 0 and out["status"] == 1 and (out["paths"] == bad["paths"]).all()
    assert (out["lengths"] == bad["lengths"]).all() and out["makespan"] == bad["makespan"]
    assert (out["flowtime_before"], out["flowtime_after"], out["accepted"]) == (0, 0, 0)
    h, first, _ = _hand()
    for what in ("off_map", "length_0", "length_T+1", "diagonal", "obstacle"):
        paths, lengths, m = first["paths"].copy(), first["lengths"].copy(), h["map"].copy()
        if what == "off_map":
            paths[1, 5] = (0, 3)
        elif what == "length_0":
            lengths[0] = 0
        elif what == "length_T+1":
            lengths[1] = h["T"] + 1
        elif what == "diagonal":
            paths[0, 1] = (1, 0)
            paths[0, 2:] = (0, 1)
        else:
            m[0, 1] = 1
        out = lr.improve(m, paths, lengths, 77, 1, 4, 2)
        assert out["status"] == 2 and (out["paths"] == paths).all() and (out["lengths"] == lengths).all(), what
        assert out["makespan"] == 77 and out["accepted"] == 0, what


# ---- the host side of the entry ----------------------------------------------------------------------------------------------
ENTRIES = ("magat_sim_mapf_improve_workspace_bytes", "magat_sim_mapf_improve")


def test_improve_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "sim_mapf_lns.hip" in build_native.SOURCES and "sim_mapf_parts.h" in build_native.HEADERS
    assert re.search(r"size_t magat_sim_mapf_improve_workspace_bytes\(", hdr) and re.search(r"int magat_sim_mapf_improve\(", hdr)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    tag = int(re.search(r"#define MAGAT_TAG_SIM_MAPF_LNS (\d+)", common).group(1))
    form = int(re.search(r"#define MAGAT_FORM_SIM_MAPF_LNS (\d+)", common).group(1))
    assert tag == nat.TAG_SIM_MAPF_LNS and nat.TAGS[tag] == "sim_mapf_lns" and form == nat.FORMS["sim_mapf_lns"]
    assert tag != nat.TAG_SIM_MAPF and form != nat.FORMS["sim_mapf"]
    assert "improve_schedules" in pkg.__all__ and callable(pkg.improve_schedules)
    lib = nat.lib()
    assert lib.magat_form_count(form) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0
    assert lib.magat_sim_mapf_improve_workspace_bytes(3, 10, 64) == 3 * (64 * 5 * 64 * 8 + 40)
    assert lib.magat_sim_mapf_improve_workspace_bytes(3, 9, 64) == 3 * (64 * 5 * 64 * 8 + 40)      # d0 rows padded to 8 bytes
    assert lib.magat_sim_mapf_improve_workspace_bytes(0, 9, 64) == 0 and lib.magat_sim_mapf_improve_workspace_bytes(3, 0, 64) == 0


def test_one_copy_of_the_search_helpers():
    csrc = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name)).read()
        for helper in ("mapf_search", "mapf_backtrace", "board_row"):
            defined = len(re.findall(r"\b%s\s*\([^;{]*\)\s*\{" % helper, text))
            assert defined == (1 if name == "sim_mapf_parts.h" else 0), (name, helper)
    for user in ("sim_mapf.hip", "sim_mapf_lns.hip"):
        assert '#include "sim_mapf_parts.h"' in open(os.path.join(csrc, user)).read()


def test_improve_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one = ctypes.c_void_p(16)
    big = 1 << 40

    def call(map_=one, H=20, W=20, solved=one, paths=one, status=one, ws=one, ws_bytes=big, C=2, N=4, T=64, it=8, k=3):
        return lib.magat_sim_mapf_improve(map_, 0, H, W, solved, paths, one, one, one, one, one, status, ws, ws_bytes, C, N, T,
                                          it, k, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_lns"])
    assert call(map_=None) == -5 and call(solved=None) == -5 and call(paths=None) == -5 and call(status=None) == -5
    assert call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1
    assert call(H=65) == -2 and call(W=65) == -2 and call(T=257) == -2
    assert call(k=0) == -2 and call(k=9) == -2 and call(it=-1) == -2 and call(it=4097) == -2
    assert call(ws_bytes=lib.magat_sim_mapf_improve_workspace_bytes(2, 4, 64) - 1) == -2
    assert call(map_=None, H=0, T=999) == -5 and call(H=0, T=999) == -1      # null, then sizes, then limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_lns"]) == before


def test_cpu_tensors_raise():
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    m = torch.zeros(5, 5, dtype=torch.uint8)
    res = dict(paths=torch.zeros(1, 2, 8, 2, dtype=torch.int32), lengths=torch.ones(1, 2, dtype=torch.int32),
               makespan=torch.zeros(1, dtype=torch.int32), solved=torch.ones(1, dtype=torch.uint8))
    with pytest.raises(nat.MagatNativeError):
        mapf.improve_schedules(m, res)


# ---- the kernel itself, compiled for the host: one thread per lane (tools/host_wave) -------------------------------------------
def _case_text(m, res, iterations, k):
    C, N, T, _ = res["paths"].shape
    ints = [C, N, T, m.shape[-2], m.shape[-1], iterations, k, int(m.ndim == 3)]
    for a in (m, res["solved"], res["paths"], res["lengths"], res["makespan"]):
        ints += np.asarray(a).astype(np.int64).reshape(-1).tolist()
    return " ".join(str(v) for v in ints)


def test_kernel_compiled_for_the_host_equals_the_restatement(tmp_path):
    """csrc/sim_mapf_lns.hip with its wavefront emulated by 64 threads and barriers (ballot, DPP shift, readfirstlane and
    shuffle as exchanges): the hand case, the skipped and the refused inputs, k > N, the 64 x 64 corner.  It covers the
    algorithm, the indexing and the barriers - not the hardware."""
    import shutil
    import subprocess
    import test_gpu_lns as tg
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lns_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_lns_check.cpp"), "-o", exe], check=True)
    for name in ("edges", "hand_k8", "corner64"):
        m, res, it, k, want = tg.case(name)
        (tmp_path / "case.txt").write_text(_case_text(m, res, it, k))
        run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
        lines = run.stdout.strip().split("\n")
        assert lines[0] == "0", name
        for key, line in zip(tg.KEYS, lines[1:]):
            got = np.array(line.split(), dtype=np.int64).reshape(np.asarray(want[key]).shape)
            np.testing.assert_array_equal(got, want[key], err_msg="%s: %s" % (name, key))
