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


def check_newcomers(name, H, want):
    """From the restatement alone: p and q join at the same step of the seed's free path, the smaller index first, and what that
    order does to the schedule (want: the restatement's result on the case, one iteration).  The GPU files call this too."""
    c, s, p, q, k = lr.newcomer_named(name, H)
    cells, first, second = c["cells"], min(p, q), max(p, q)
    assert mr.check_schedule(c["map"], c["start"][0], c["goal"][0], c["res"]["paths"][0], c["res"]["lengths"][0]) is None
    empty = lr._Boards(H, 20, c["T"])
    d0 = [len(empty.plan(c["map"] == 0, w[0], w[-1])) for w in cells]
    delay = [len(w) - d for w, d in zip(cells, d0)]
    assert delay[s] == 2 == max(delay) and delay.count(2) == 1                      # the seed of iteration 0
    assert empty.plan(c["map"] == 0, cells[s][0], cells[s][-1]) == lr.NEWCOMER_FREE_PATH
    others = [[b for b in lr.joiners(lr.NEWCOMER_FREE_PATH, cells, t) if b != s] for t in range(5)]
    assert others == [[], [], [first, second], [], []]                              # both at t = 2, nobody at any other step
    assert cells[p][2] == lr.NEWCOMER_FREE_PATH[2] and (cells[q][1], cells[q][2]) == (lr.NEWCOMER_FREE_PATH[2], lr.NEWCOMER_FREE_PATH[1])
    assert lr.neighbourhood(s, lr.NEWCOMER_FREE_PATH, cells, k) == [s, first, second][:k]
    L = want["lengths"][0]
    if q < p:         # s, then q, then p: everybody finds a way
        assert want["accepted"].tolist() == [1] and (want["flowtime_before"].tolist(), want["flowtime_after"].tolist()) == ([12], [11])
        assert [int(L[s]), int(L[p]), int(L[q])] == ([6, 4, 4] if k == 2 else [5, 5, 4])
    else:             # s, then p: nothing gained (k = 2), or q shut in behind them (k = 3)
        assert want["accepted"].tolist() == [0] and (want["paths"] == c["res"]["paths"]).all()
    assert want["status"].tolist() == [0]


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


def test_the_walk_and_the_group_have_one_home():
    """One body of the improver for both widths (sim_mapf_lns_walk.h), one workgroup per width (sim_group.h): the two kernel files
    bring a form and nothing of the rule, and nobody spells a reduction, a free-map load or a path reservation out again."""
    from magat_pathplanning_amd import build_native
    csrc = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
    assert all(h in build_native.HEADERS for h in ("sim_mapf_lns_walk.h", "sim_group.h", "sim_entry.h"))
    homes = {"mapf_lns_walk": "sim_mapf_lns_walk.h", "lns_mark": "sim_mapf_lns_walk.h", "lns_count_ge": "sim_mapf_lns_walk.h",
             "lns_entry_check": "sim_mapf_lns_walk.h", "load_free": "sim_group.h", "group_min": "sim_group.h", "group_max": "sim_group.h",
             "group_sum": "sim_group.h", "group_or": "sim_group.h", "group_sum_waves": "sim_group.h", "group_min3": "sim_group.h", "group_count": "sim_group.h",
             "publish_free": "sim_group.h", "group_sum_max": "sim_group.h", "sim_entry_check": "sim_entry.h"}
    per_width = {"load_free": 4, "group_min": 2, "group_max": 2, "group_sum": 2, "group_or": 2, "group_min3": 2, "group_count": 2,
                 "group_sum_waves": 2, "group_sum_max": 2, "publish_free": 2}      # load_free: the ballot load of each width and the member that calls it
    once = {"bad |= la < 1 || la > T": "screening", "while (hi - lo > 1)": "the bisection", "const int fc = lds.fcells[t]": "the scan",
            "if (done == m && new_sum < old_sum)": "accept / roll back"}
    free_loads = []
    seen = {key: [] for key in once}
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name)).read()
        code = re.sub(r"//[^\n]*", "", text)
        for helper, home in homes.items():
            defined = len(re.findall(r"\b(?:int|void|bool|u64|wboard<NW>) %s\(" % helper, code))
            assert defined == (per_width.get(helper, 1) if name == home else 0), (name, helper, defined)
        assert text.count("void wide_launch(") == (1 if name == "sim_entry.h" else 0), name
        free_loads += [name] * len(re.findall(r"ballot_w64\(\w+ < W && mp\[[^\]]*\] == 0\)", text))
        for key in once:
            seen[key] += [name] * text.count(key)
        if name in ("sim_mapf_lns.hip", "sim_mapf_lns_wide.hip"):
            assert "__builtin_amdgcn_ballot_w64" not in text and "wave_all_" not in text and "wide_post" not in text, name
    assert free_loads == ["sim_group.h", "sim_group.h"]                # the free-map ballot load: once per width
    assert all(where == ["sim_mapf_lns_walk.h"] for where in seen.values()), seen
    for src, form in (("sim_mapf_lns.hip", "wave_group"), ("sim_mapf_lns_wide.hip", "wide_group<NW>")):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "sim_mapf_lns_walk.h"' in text and text.count("mapf_lns_walk(") == 1 and ": " + form in text, src
        assert "for (int it" not in text and "lns_mark" not in text and not re.search(r"\bgroup_(min|max|sum|or|count)", text), src
    for user in ("sim_mapf_cbs_parts.h", "sim_mapf_ecbs_wide.hip", "sim_mapf.hip", "sim_mapf_wide.hip", "sim_mapf_audit.hip",
                 "sim_mapf_audit_wide.hip"):
        assert '#include "sim_group.h"' in open(os.path.join(csrc, user)).read(), user
    for src in ("sim_mapf_wide.hip", "sim_mapf_lns_wide.hip", "sim_mapf_audit_wide.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert text.count("wide_launch(") == 1 and "switch (wide_words" not in text, src


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
    for name in ("edges", "hand_k8", "corner64") + tuple(tg.NEWCOMER_NAMES):
        m, res, it, k, want = tg.case(name)
        if name in tg.NEWCOMER_NAMES:
            check_newcomers(name, 8, want)
        (tmp_path / "case.txt").write_text(_case_text(m, res, it, k))
        run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
        lines = run.stdout.strip().split("\n")
        assert lines[0] == "0", name
        for key, line in zip(tg.KEYS, lines[1:]):
            got = np.array(line.split(), dtype=np.int64).reshape(np.asarray(want[key]).shape)
            np.testing.assert_array_equal(got, want[key], err_msg="%s: %s" % (name, key))
