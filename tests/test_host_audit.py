"""CPU-only: the schedule audit (csrc/sim_mapf_audit.hip, csrc/sim_mapf_audit_wide.hip, mapf.audit_schedules).  The yardstick
is tests/audit_restatement.py; here it is checked against tests/mapf_restatement.check_schedule and against values worked out
by hand, the inputs of tests/test_gpu_audit.py are made (once per session, with the restatement's answer) and what each of them
is there for is asserted, so that no GPU test can pass on a batch in which nothing happens.  Then the host side of the entries
- header / loader / build lists / workspace formulas / argument checks - and both kernels compiled for the host, their
wavefronts emulated by threads (tools/host_wave)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import audit_restatement as ar
import mapf_restatement as mr
from conftest import ROOT

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
ENTRIES = ("magat_sim_mapf_audit_workspace_bytes", "magat_sim_mapf_audit", "magat_sim_mapf_audit_wide_workspace_bytes",
           "magat_sim_mapf_audit_wide")
NEIGHBOURS = ((-1, 0), (0, -1), (1, 0), (0, 1))


# ---- the inputs: name -> dict(map, start, goal, paths, lengths, solved or None, wide, want) ----------------------------------------
def _inputs(m, s, g, res, solved=True, wide=False):
    return dict(map=np.asarray(m, dtype=np.uint8), start=np.asarray(s, dtype=np.int32), goal=np.asarray(g, dtype=np.int32),
                paths=np.asarray(res["paths"], dtype=np.int32), lengths=np.asarray(res["lengths"], dtype=np.int32),
                solved=np.asarray(res["solved"], dtype=np.uint8) if solved else None, wide=wide)


@functools.lru_cache(maxsize=None)
def seed7():
    m, s, g = mr.random_batch(7, 16, 20, 20, 10, 0.1)
    return m, s, g, mr.solve_batch(m, s, g, 90, retries=8)


def standing(case, a, cell):
    """agent a of a case (dict of arrays of one case) stands on `cell` for ever: start = goal = cell, length 1."""
    case["start"][a] = case["goal"][a] = cell
    case["paths"][a, :] = cell
    case["lengths"][a] = 1


CORRUPTIONS = ("untouched", "kind1", "kind2", "kind3", "kind4", "kind5", "kind6", "kind7", "kind8", "length_0", "length_T+1",
               "cell_-1_3", "cell_H_0", "cell_2^30", "start_on_obstacle", "three_in_a_cell", "swap_beats_vertex",
               "stage1_beats_conflict", "earlier_t_wins", "follow_is_no_swap")
# (kind, t, a, b) that each corruption is built to give; None: whatever the restatement finds is asserted by kind only below
CORRUPTED_FAULTS = {"untouched": (0, -1, -1, -1), "kind1": (1, -1, 3, -1), "kind2": (2, 0, 2, -1), "length_0": (1, -1, 0, -1),
                    "length_T+1": (1, -1, 9, -1), "cell_-1_3": (4, 4, 3, -1), "cell_H_0": (4, 4, 3, -1), "cell_2^30": (4, 4, 3, -1),
                    "start_on_obstacle": (4, 0, 0, -1), "three_in_a_cell": (7, 0, 7, 8), "swap_beats_vertex": (8, 1, 0, 7),
                    "stage1_beats_conflict": (4, 3, 4, -1), "follow_is_no_swap": (0, -1, -1, -1)}
CORRUPTED_KINDS = {"kind3": 3, "kind4": 4, "kind5": 5, "kind6": 6, "kind7": 7, "kind8": 8, "earlier_t_wins": 7}


def corrupted_inputs():
    """One solved 20 x 20 / 10-agent schedule (case 0 of the seed-7 batch, T = 90), one case per corruption, a map per case."""
    m, s, g, res = seed7()
    assert res["solved"][0] == 1
    base = dict(map=m.copy(), start=s[0].copy(), goal=g[0].copy(), paths=res["paths"][0].copy(), lengths=res["lengths"][0].copy())
    T = base["paths"].shape[1]
    P, L = base["paths"], base["lengths"]
    assert all(tuple(P[a, 1]) != tuple(P[a, 0]) for a in (0, 2)) and L[4] >= 3 and L[6] >= 5      # what the constructions lean on
    cases = []
    for what in CORRUPTIONS:
        k = {key: value.copy() for key, value in base.items()}
        if what == "kind1":
            k["lengths"][3] = -2
        elif what == "kind2":
            k["start"][2] = k["goal"][2]
        elif what == "kind3":
            k["goal"][5] = k["start"][5]
        elif what == "kind4":
            k["map"][tuple(P[1, 2])] = 1
        elif what == "kind5":
            k["paths"][4, L[4]] = P[4, L[4] - 2]
        elif what == "kind6":
            jump = next(t for t in range(2, L[6]) if abs(P[6, t] - P[6, 0]).sum() > 1)
            k["paths"][6, 1] = P[6, jump]
        elif what == "kind7":
            standing(k, 8, P[2, 5].copy())
        elif what == "kind8":
            k["start"][9], k["goal"][9] = P[0, 1], P[0, 0]
            k["paths"][9, 0], k["paths"][9, 1:], k["lengths"][9] = P[0, 1], P[0, 0], 2
        elif what == "length_0":
            k["lengths"][0] = 0
        elif what == "length_T+1":
            k["lengths"][9] = T + 1
        elif what == "cell_-1_3":
            k["paths"][3, 4] = (-1, 3)
        elif what == "cell_H_0":
            k["paths"][3, 4] = (20, 0)
        elif what == "cell_2^30":
            k["paths"][3, 4] = (2 ** 30, 2 ** 30)
        elif what == "start_on_obstacle":
            k["map"][tuple(k["start"][0])] = 1
        elif what == "three_in_a_cell":
            cell = next((r, c) for r in range(20) for c in range(20)
                        if m[r, c] == 0 and not (P.reshape(-1, 2) == (r, c)).all(1).any())      # a cell nobody visits
            for a in (7, 8, 9):
                standing(k, a, cell)
        elif what in ("swap_beats_vertex", "stage1_beats_conflict"):
            standing(k, 5, P[2, 1].copy())                        # vertex (2, 5) at t = 1
            if what == "swap_beats_vertex":                       # and a swap (0, 7) at t = 1
                k["start"][7], k["goal"][7] = P[0, 1], P[0, 0]
                k["paths"][7, 0], k["paths"][7, 1:], k["lengths"][7] = P[0, 1], P[0, 0], 2
            else:
                k["paths"][4, 3] = (-1, 0)
        elif what == "earlier_t_wins":
            standing(k, 8, P[2, 5].copy())
            standing(k, 9, P[3, 2].copy())
        elif what == "follow_is_no_swap":      # agent 9 stands where agent a steps to and leaves it for a third cell in the same step
            k = None
            for a in range(9):
                for dr, dc in NEIGHBOURS:
                    A, B = P[a, 0], P[a, 1]
                    C = (int(B[0]) + dr, int(B[1]) + dc)
                    if tuple(A) == tuple(B) or not (0 <= C[0] < 20 and 0 <= C[1] < 20) or m[C] != 0 or C == tuple(A):
                        continue
                    trial = {key: value.copy() for key, value in base.items()}
                    trial["start"][9], trial["goal"][9] = B, C
                    trial["paths"][9, 0], trial["paths"][9, 1:], trial["lengths"][9] = B, C, 2
                    if k is None and ar.audit(trial["map"], trial["start"], trial["goal"], trial["paths"], trial["lengths"])["status"] == 0:
                        k = trial
            assert k is not None
        cases.append(k)
    out = {key: np.stack([k[key] for k in cases]) for key in base}
    return out["map"], out["start"], out["goal"], dict(paths=out["paths"], lengths=out["lengths"], solved=None)


def other_component():
    """5 x 7 with a wall down column 3: agent 0's goal lies behind it (dist -1), agent 1 walks two cells; agent 0 stays at home,
    so its schedule does not end at its goal."""
    m = mr.grid(["...#...", "...#...", "...#...", "...#...", "...#..."])
    s, g = np.array([[[0, 0], [4, 0]]], dtype=np.int32), np.array([[[0, 6], [4, 2]]], dtype=np.int32)
    paths = np.zeros((1, 2, 6, 2), dtype=np.int32)
    paths[0, 0, :] = (0, 0)
    paths[0, 1, :] = (4, 2)
    paths[0, 1, 0], paths[0, 1, 1] = (4, 0), (4, 1)
    return m, s, g, dict(paths=paths, lengths=np.array([[1, 3]], dtype=np.int32), solved=None)


def line(cells, T):
    """A walk as a padded path (T,2) and its length."""
    p = np.array(list(cells) + [cells[-1]] * (T - len(cells)), dtype=np.int32)
    return p, len(cells)


OPEN_MAPS = {"open65": (65, 65), "open10x65": (10, 65), "open65x10": (65, 10), "open70x130": (70, 130), "open129": (129, 129),
             "open256": (256, 256)}


def open_inputs(H, W, T=8):
    """An open H x W map, three cases: straight walks across every seam of the word / wavefront layout (columns and rows 63|64,
    127|128, 191|192), valid; the same with a vertex conflict ON the highest seam; the same with a swap ACROSS it.  The last four
    agents are X, Y (vertex) and P, Q (swap); the seam is a column seam when the map has one, else a row seam (transposed)."""
    walks = []
    for i, seam in enumerate((64, 128, 192)):
        if seam < W:
            walks.append([(2 * i, c) for c in range(seam - 3, min(W, seam + 3))])
        if seam < H:
            walks.append([(r, 2 * i) for r in range(seam - 3, min(H, seam + 3))])
    cols = W > 64
    seam = max(s for s in (64, 128, 192) if s < (W if cols else H))
    flip = (lambda cell: cell) if cols else (lambda cell: (cell[1], cell[0]))
    cases = []
    for what in ("valid", "vertex", "swap"):
        X = [(7, seam - 2), (7, seam - 1), (7, seam)]
        Y = [(5, seam), (6, seam), (7, seam)] if what == "vertex" else [(5, seam)]
        P = [(9, seam - 1), (9, seam)]
        Q = [(9, seam), (9, seam - 1)] if what == "swap" else [(8, seam)]
        rows = walks + [[flip(c) for c in w] for w in (X, Y, P, Q)]
        made = [line(w, T) for w in rows]
        cases.append(dict(paths=np.stack([p for p, _ in made]), lengths=np.array([n for _, n in made], dtype=np.int32),
                          start=np.array([w[0] for w in rows], dtype=np.int32), goal=np.array([w[-1] for w in rows], dtype=np.int32)))
    out = {key: np.stack([k[key] for k in cases]) for key in cases[0]}
    N = out["paths"].shape[1]
    faults = [(0, -1, -1, -1), (7, 2, N - 4, N - 3), (8, 1, N - 2, N - 1)]
    return np.zeros((H, W), dtype=np.uint8), out["start"], out["goal"], dict(paths=out["paths"], lengths=out["lengths"], solved=None), faults


def serpentine65():
    """65 x 65: rows 0, 2, 4, 6, 8 free, the odd rows between them walls with one gap at alternating ends, everything below
    walled: ONE way of 4 * 64 + 8 = 264 steps from (0, 0) to (8, 0), every row of it across the word seam 63|64.  Agent 0 walks
    nowhere (its schedule does not end at its goal), agent 1 wants the other way round."""
    m = np.ones((65, 65), dtype=np.uint8)
    for r in range(0, 9, 2):
        m[r, :] = 0
    for r in range(1, 8, 2):
        m[r, 64 if (r // 2) % 2 == 0 else 0] = 0
    s, g = np.array([[[0, 0], [8, 0]]], dtype=np.int32), np.array([[[8, 0], [0, 0]]], dtype=np.int32)
    paths = np.repeat(s[:, :, None, :], 4, axis=2).astype(np.int32)
    return m, s, g, dict(paths=paths, lengths=np.ones((1, 2), dtype=np.int32), solved=None)


def wall_seam():
    """70 x 130, a wall down column 66 from row 0 to row 66 - across the wavefront seam 63|64 - with the way round it below:
    (10, 60) -> (10, 70) is 57 down, 10 across, 57 up.  Agent 1 stands still next to the wall."""
    m = np.zeros((70, 130), dtype=np.uint8)
    m[0:67, 66] = 1
    s, g = np.array([[[10, 60], [64, 65]]], dtype=np.int32), np.array([[[10, 70], [64, 65]]], dtype=np.int32)
    paths = np.repeat(s[:, :, None, :], 4, axis=2).astype(np.int32)
    return m, s, g, dict(paths=paths, lengths=np.ones((1, 2), dtype=np.int32), solved=None)


def agents1000():
    """160 x 160 open, 1000 agents, each walking 5 cells to the right on a lane of 6 cells of its own (26 lanes per row): case 0
    valid; case 1 the same, but agent 999 stands on agent 998's cell at t = 3."""
    T = 6
    rows = [[(a // 26, 6 * (a % 26) + t) for t in range(6)] for a in range(1000)]
    made = [line(w, T) for w in rows]
    paths = np.stack([p for p, _ in made])
    case0 = dict(paths=paths, lengths=np.full(1000, 6, dtype=np.int32), start=paths[:, 0].copy(), goal=paths[:, 5].copy())
    case1 = {key: value.copy() for key, value in case0.items()}
    standing(case1, 999, paths[998, 3].copy())
    out = {key: np.stack([case0[key], case1[key]]) for key in case0}
    return np.zeros((160, 160), dtype=np.uint8), out["start"], out["goal"], dict(paths=out["paths"], lengths=out["lengths"], solved=None)


NAMES_64 = ("hand", "seed7", "corrupted", "corner64", "wide5x64", "tall64x5", "w33", "crowd70", "serpentine_T256", "other_component",
            "c300")
NAMES_WIDE = tuple(OPEN_MAPS) + ("serpentine65", "wall_seam", "agents1000", "hand_T300")
ALL_NAMES = NAMES_64 + NAMES_WIDE


@functools.lru_cache(maxsize=None)
def case(name):
    """Treat what comes back as read-only."""
    import test_gpu_lns as tl
    import test_gpu_mapf as tm
    if name in ("hand", "wide5x64", "tall64x5", "w33", "serpentine_T256", "c300"):      # the planner's own batches, planned once
        m, s, g, _, _ = tm.batch(name)
        k = _inputs(m, s, g, tm.expected_plan(name))
    elif name == "hand_T300":           # inside 64 x 64, but a horizon for the wide form
        m, s, g, _, _ = tm.batch("hand")
        k = _inputs(m, s, g, mr.plan_batch(m, s, g, None, 300), wide=True)
    elif name == "seed7":
        k = _inputs(*seed7())
    elif name == "corrupted":
        k = _inputs(*corrupted_inputs(), solved=False)
    elif name == "corner64":
        m, s, g = tl.corner64()
        k = _inputs(m, s, g, tl.case("corner64")[1])
    elif name == "crowd70":
        m, s, g = tl.crowd70()
        k = _inputs(m, s, g, tl.case("crowd70")[1])
    elif name == "other_component":
        k = _inputs(*other_component(), solved=False)
    elif name in OPEN_MAPS:
        k = _inputs(*open_inputs(*OPEN_MAPS[name])[:4], solved=False, wide=True)
    elif name == "serpentine65":
        k = _inputs(*serpentine65(), solved=False, wide=True)
    elif name == "wall_seam":
        k = _inputs(*wall_seam(), solved=False, wide=True)
    elif name == "agents1000":
        k = _inputs(*agents1000(), solved=False, wide=True)
    else:
        raise KeyError(name)
    k["want"] = ar.audit_batch(k["map"], k["start"], k["goal"], k["paths"], k["lengths"], k["solved"])
    return k


def check_what_the_case_is_there_for(name):
    """The figures of the restatement alone; the GPU file calls this too, so that an input cannot quietly change under it."""
    k = case(name)
    want = k["want"]
    if name in ("hand", "hand_T300"):
        names = list(mr.hand_cases())
        i = {n: names.index(n) for n in names}
        assert want["status"].tolist() == [0 if k["solved"][c] else 1 for c in range(5)] and 0 < int(k["solved"].sum()) < 5
        assert (k["lengths"][i["wait_in_pocket"]] - 1).tolist() == [6, 9] and want["dist"][i["wait_in_pocket"]].tolist() == [6, 6]
        assert (k["lengths"][i["goal_crossed_at_5"]] - 1).tolist() == [6, 6] and want["dist"][i["goal_crossed_at_5"]].tolist() == [6, 1]
        assert k["solved"][i["head_on_closed"]] == 0 and want["dist"][i["head_on_closed"]].tolist() == [6, 6]
        assert want["flowtime_bound"][i["head_on_closed"]] == 12 and want["flowtime"][i["head_on_closed"]] == -1
        assert want["dist"][i["start_is_goal"]].tolist() == [0, 0] and want["flowtime"][i["start_is_goal"]] == 0
        assert want["flowtime"][i["wait_in_pocket"]] == 15 and want["makespan"][i["wait_in_pocket"]] == 9
        assert bool(ar.certified(want, 1)[i["start_is_goal"]]) and not bool(ar.certified(want, 1)[i["wait_in_pocket"]])
        assert k["paths"].shape[2] == (300 if name == "hand_T300" else 24)
    elif name == "seed7":
        assert want["status"].tolist() == [0] * 16 and bool((k["lengths"] - 1 >= want["dist"]).all())
        ok = ar.certified(want, 1.05)
        assert 0 < int(ok.sum()) < 16 and 0 < int(ar.certified(want, 1).sum()) and bool(ar.certified(want, 2).all())
    elif name == "corrupted":
        for c, what in enumerate(CORRUPTIONS):
            fault = tuple(want["fault"][c].tolist())
            if what in CORRUPTED_FAULTS:
                assert fault == CORRUPTED_FAULTS[what], (what, fault)
            else:
                assert fault[0] == CORRUPTED_KINDS[what], (what, fault)
            assert want["status"][c] == (0 if fault[0] == 0 else 2), what
        t = {what: int(want["fault"][c, 1]) for c, what in enumerate(CORRUPTIONS)}
        assert t["earlier_t_wins"] <= 2 < t["kind7"] <= 5
        c = CORRUPTIONS.index("start_on_obstacle")
        assert want["dist"][c, 0] == -1 and want["flowtime_bound"][c] == -1 and want["makespan_bound"][c] == -1
        assert int((want["flowtime_bound"] >= 0).sum()) >= len(CORRUPTIONS) - 2
    elif name == "corner64":
        assert k["map"].shape == (64, 64) and want["status"].tolist() == [0] and want["dist"].tolist() == [[5, 2]]
        assert k["start"][0, 1].tolist() == [63, 63] and want["flowtime"].tolist() == [10]
    elif name in ("wide5x64", "tall64x5", "w33", "c300"):
        assert want["status"].tolist() == [0 if v else 1 for v in k["solved"]] and int((want["status"] == 0).sum()) >= 2
        assert int(want["flowtime_bound"].min()) > 0
        if name == "c300":
            assert len(want["status"]) == 300 and 0 < int((want["status"] == 1).sum()) < 300
    elif name == "crowd70":
        assert k["paths"].shape[1] == 70 and want["status"].tolist() == [0, 0] and int(want["dist"].min()) >= 1
    elif name == "serpentine_T256":
        assert k["paths"].shape[2] == 256 and want["status"].tolist() == [0] and int(want["dist"].min()) > 128
    elif name == "other_component":
        assert want["dist"].tolist() == [[-1, 2]] and want["flowtime_bound"].tolist() == [-1] and want["makespan_bound"].tolist() == [-1]
        assert want["fault"].tolist() == [[3, 0, 0, -1]] and not bool(ar.certified(want, 2).any())
    elif name in OPEN_MAPS:
        H, W = OPEN_MAPS[name]
        faults = open_inputs(H, W)[4]
        assert [tuple(f) for f in want["fault"].tolist()] == faults and want["status"].tolist() == [0, 2, 2]
        assert (want["dist"] == k["lengths"] - 1).all() and int(want["flowtime"][0]) == int(want["flowtime_bound"][0]) > 0
        seams = sum(1 for s in (64, 128, 192) if s < W) + sum(1 for s in (64, 128, 192) if s < H)
        assert k["paths"].shape[1] == seams + 4
    elif name == "serpentine65":
        assert want["dist"].tolist() == [[264, 264]] and want["makespan_bound"].tolist() == [264] and want["fault"].tolist() == [[3, 0, 0, -1]]
    elif name == "wall_seam":
        assert want["dist"].tolist() == [[124, 0]] and want["fault"].tolist() == [[3, 0, 0, -1]]
    elif name == "agents1000":
        assert want["status"].tolist() == [0, 2] and want["fault"].tolist() == [[0, -1, -1, -1], [7, 3, 998, 999]]
        assert want["flowtime"].tolist() == [5000, -1] and want["flowtime_bound"].tolist() == [5000, 4995]


@pytest.mark.parametrize("name", ALL_NAMES)
def test_restatement_on_the_inputs(name):
    check_what_the_case_is_there_for(name)


# ---- the restatement against mapf_restatement.check_schedule ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand", "seed7", "corrupted"])
def test_restatement_agrees_with_check_schedule(name):
    k = case(name)
    kinds = set()
    for c in range(len(k["start"])):
        if k["solved"] is not None and k["solved"][c] == 0:
            continue
        m = k["map"] if k["map"].ndim == 2 else k["map"][c]
        got = ar.audit(m, k["start"][c], k["goal"][c], k["paths"][c], k["lengths"][c])
        said = mr.check_schedule(m, k["start"][c], k["goal"][c], k["paths"][c], k["lengths"][c])
        assert (got["status"] == 0) == (said is None), (name, c, said)
        if said is not None:
            kind, t, a, b = got["fault"]
            kinds.add(kind)
            assert ar.KIND_WORDS[kind] in said, (name, c, got["fault"], said)
            assert said.startswith("agent %d" % a if b < 0 else "agents %d and %d" % (a, b)), (name, c, got["fault"], said)
            if kind >= 4:
                assert re.search(r"(t = |step )%d\b" % t, said), (name, c, got["fault"], said)
    if name == "corrupted":
        assert kinds == set(range(1, 9))


def test_certified_on_the_restatement():
    want = case("seed7")["want"]
    with pytest.raises(ValueError):
        ar.certified(want, 0.9)
    zero = dict(status=np.array([0, 0, 2, 1]), flowtime_bound=np.array([0, 0, 0, 4]), flowtime=np.array([0, 1, -1, -1]))
    assert ar.certified(zero, 1).tolist() == [True, False, False, False] and ar.certified(zero, 100).tolist() == [True, False, False, False]


# ---- the host side of the entries ---------------------------------------------------------------------------------------------
def documented_bytes(C, N, T):
    """include/magat_hip.h: C * 2 * N * 4."""
    return C * 2 * N * 4


def documented_wide_bytes(C, H, W, N, T):
    """include/magat_hip.h: C * (2 * H * W + 2 * N) * 4."""
    return C * (2 * H * W + 2 * N) * 4


def test_audit_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(CSRC, "magat_common.h")).read()
    for src in ("sim_mapf_audit.hip", "sim_mapf_audit_wide.hip"):
        assert src in build_native.SOURCES, src
        text = open(os.path.join(CSRC, src)).read()
        assert "MAGAT_FORM_SIM_MAPF_AUDIT" in text and "MAGAT_TAG_SIM_MAPF_AUDIT" in text and '#include "sim_mapf_audit_parts.h"' in text
        assert "asm" not in text and "printf" not in text and "assert(" not in text and "hipDeviceSynchronize" not in text
    assert "sim_mapf_audit_parts.h" in build_native.HEADERS
    assert re.search(r"^size_t magat_sim_mapf_audit_workspace_bytes\(int C, int N, int T\);", hdr, re.M)
    assert re.search(r"^size_t magat_sim_mapf_audit_wide_workspace_bytes\(int C, int H, int W, int N, int T\);", hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_audit\(", hdr, re.M) and re.search(r"^int magat_sim_mapf_audit_wide\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    assert nat._SIGNATURES["magat_sim_mapf_audit_wide"] == nat._SIGNATURES["magat_sim_mapf_audit"]      # the same arguments
    assert len(nat._SIGNATURES["magat_sim_mapf_audit"][1]) == 22
    tag = int(re.search(r"#define MAGAT_TAG_SIM_MAPF_AUDIT (\d+)", common).group(1))
    form = int(re.search(r"#define MAGAT_FORM_SIM_MAPF_AUDIT (\d+)", common).group(1))
    assert tag == nat.TAG_SIM_MAPF_AUDIT and nat.TAGS[tag] == "sim_mapf_audit" and form == nat.FORMS["sim_mapf_audit"]
    assert tag == nat.TAG_SIM_MAPF_LNS + 1 and form == nat.FORMS["sim_mapf_lns"] + 1
    for name in ("audit_schedules", "certified", "certified_pack"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.magat_form_count(form) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(ms)) == 0


def test_the_audit_body_has_one_home():
    """audit_walk in sim_mapf_audit_parts.h is the body of both kernels: the stages are called from there alone, and the two kernel
    files bring a form (the flood, the owner grids) on sim_group.h's workgroup and nothing of the rule."""
    for name in sorted(os.listdir(CSRC)):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        for helper in ("audit_stage1", "audit_walk", "audit_entry_check", "audit_write", "audit_fault1"):
            defined = len(re.findall(r"\b(?:int|void) %s\(" % helper, text))
            assert defined == (1 if name == "sim_mapf_audit_parts.h" else 0), (name, helper)
        calls = len(re.findall(r"\baudit_stage1\(", text))
        assert calls == (2 if name == "sim_mapf_audit_parts.h" else 0), (name, calls)      # its definition and ONE call
    for src, group, flood in (("sim_mapf_audit.hip", "wave_group", "audit_flood"), ("sim_mapf_audit_wide.hip", "wide_group<NW>", "waudit_flood")):
        text = open(os.path.join(CSRC, src)).read()
        assert text.count("audit_walk(") == 1 and ": " + group in text and len(re.findall(r"\bint %s\(" % flood, text)) == 1, src
        assert "__syncthreads" not in text and "audit_stage" not in text and "wave_all_" not in text, src


def test_audit_workspace_formulas():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for C, N, T in ((1, 1, 1), (16, 10, 90), (300, 3, 20), (2, 70, 40), (1, 4096, 256), (5, 7, 256)):
        assert lib.magat_sim_mapf_audit_workspace_bytes(C, N, T) == documented_bytes(C, N, T), (C, N, T)
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8), (1, 4097, 8), (1, 4, 257)):
        assert lib.magat_sim_mapf_audit_workspace_bytes(*bad) == 0, bad
    for C, H, W, N, T in ((1, 65, 65, 7, 8), (3, 10, 65, 5, 8), (2, 70, 130, 9, 24), (2, 160, 160, 1000, 6), (1, 256, 256, 4096, 1024),
                          (5, 5, 7, 2, 300), (1, 1, 1, 1, 1)):
        assert lib.magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T) == documented_wide_bytes(C, H, W, N, T), (C, H, W, N, T)
    for bad in ((0, 65, 65, 4, 8), (1, 0, 65, 4, 8), (1, 65, -1, 4, 8), (1, 65, 65, 0, 8), (1, 65, 65, 4, 0), (1, 257, 65, 4, 8),
                (1, 65, 257, 4, 8), (1, 65, 65, 4097, 8), (1, 65, 65, 4, 1025)):
        assert lib.magat_sim_mapf_audit_wide_workspace_bytes(*bad) == 0, bad


@pytest.mark.parametrize("wide", [False, True])
def test_audit_argument_checks_answer_before_anything_touches_a_device(wide):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50
    side, horizon = (256, 1024) if wide else (64, 256)
    entry = lib.magat_sim_mapf_audit_wide if wide else lib.magat_sim_mapf_audit

    def call(map_=one, H=20, W=20, solved=one, paths=one, start=one, status=one, dist=one, makespan=one, ws=one, ws_bytes=big, C=2,
             N=4, T=64):
        return entry(map_, 0, H, W, solved, paths, one, start, one, status, one, dist, one, one, one, makespan, ws, ws_bytes, C, N, T,
                     None)

    def needed(C, H, W, N, T):
        return documented_wide_bytes(C, H, W, N, T) if wide else documented_bytes(C, N, T)

    before = lib.magat_form_count(nat.FORMS["sim_mapf_audit"])
    assert call(map_=None) == -5 and call(paths=None) == -5 and call(start=None) == -5 and call(status=None) == -5
    assert call(dist=None) == -5 and call(makespan=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1
    assert call(H=side + 1) == -2 and call(W=side + 1) == -2 and call(T=horizon + 1) == -2 and call(N=4097) == -2
    assert call(ws_bytes=needed(2, 20, 20, 4, 64) - 1) == -2
    # the limits themselves pass: the next check is the workspace's size, then its alignment; `solved` may be NULL
    full = needed(2, side, side, 4096, horizon)
    assert call(H=side, W=side, T=horizon, N=4096, ws_bytes=full - 1) == -2
    assert call(H=side, W=side, T=horizon, N=4096, ws=odd, ws_bytes=full) == -3
    assert call(solved=None, ws=odd) == -3 and call(H=1, W=1, T=1, N=1, C=1, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1 and call(T=9999, ws=odd) == -2      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf_audit"]) == before            # a refused call is not counted as a launch


def test_python_surface_on_cpu_tensors():
    import inspect
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import mapf
    assert list(inspect.signature(mapf.audit_schedules).parameters) == ["obstacle_map", "res", "wide"]
    assert inspect.signature(mapf.audit_schedules).parameters["wide"].default is False
    sig = inspect.signature(mapf.solve_cases)
    assert list(sig.parameters)[-1] == "certify" and sig.parameters["certify"].default is None
    m = torch.zeros(5, 5, dtype=torch.uint8)
    cell = torch.zeros(1, 2, 2, dtype=torch.int32)
    res = dict(paths=torch.zeros(1, 2, 8, 2, dtype=torch.int32), lengths=torch.ones(1, 2, dtype=torch.int32), start=cell, goal=cell)
    with pytest.raises(nat.MagatNativeError):
        mapf.audit_schedules(m, res)
    with pytest.raises(nat.MagatNativeError):
        mapf.audit_schedules(m, res, wide=True)
    with pytest.raises(ValueError):
        mapf.solve_cases(m, cell, cell, certify=0.9)
    audit = dict(status=torch.tensor([0, 0, 2, 1, 0]), flowtime_bound=torch.tensor([0, 0, 0, 4, 20]),
                 flowtime=torch.tensor([0, 1, -1, -1, 21]))
    assert mapf.certified(audit, 1).tolist() == [True, False, False, False, False]
    assert mapf.certified(audit, 1.05).tolist() == [True, False, False, False, True]
    with pytest.raises(ValueError):
        mapf.certified(audit, 0.9)
    with pytest.raises(ValueError):
        mapf.certified_pack(res, dict(audit, status=torch.full((5,), 2)), 2)


# ---- the kernels themselves, compiled for the host: one thread per lane, 1 to 4 wavefronts (tools/host_wave) -----------------------
def _case_text(k):
    C, N, T, _ = k["paths"].shape
    ints = [C, N, T, k["map"].shape[-2], k["map"].shape[-1], int(k["map"].ndim == 3), int(k["solved"] is not None)]
    for a in (k["map"], k["solved"], k["paths"], k["lengths"], k["start"], k["goal"]):
        if a is not None:
            ints += np.asarray(a).astype(np.int64).reshape(-1).tolist()
    return " ".join(str(v) for v in ints)


@pytest.fixture(scope="module")
def audit_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "audit_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "mapf_audit_check.cpp"), "-o", exe], check=True)
    return exe


# (every thread rendezvous is a futex here, so the suite runs the small inputs; the others were run by hand - DESIGN 4.11)
HOST_RUNS = [("hand", "64"), ("corrupted", "64"), ("corner64", "64"), ("other_component", "64"), ("open65", "wide"),
             ("open10x65", "wide"), ("open65x10", "wide"), ("open70x130", "wide")]


# the 64 form's host inputs through the WIDE kernel's entry: audit_schedules(..., wide=True) sends a shape inside 64 x 64 to the
# 64 form, so only here do the two kernels meet on one input - one body (audit_walk), two forms, one answer
HOST_RUNS += [(name, "wide") for name, form in HOST_RUNS if form == "64"]


@pytest.mark.parametrize("name,form", HOST_RUNS)
def test_kernels_compiled_for_the_host_equal_the_restatement(audit_check, tmp_path, name, form):
    """Both kernels with their wavefronts emulated by threads and barriers - ballot, DPP shift, readfirstlane and shuffle as
    exchanges inside a wavefront, __syncthreads across the workgroup, atomicMin as a compare-and-swap: 1, 2 and 3 wavefronts,
    1, 2 and 4 words.  It covers the algorithm, the indexing and the barriers - not the hardware."""
    k = case(name)
    (tmp_path / "case.txt").write_text(_case_text(k))
    run = subprocess.run([audit_check, form, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    assert lines[0] == "0", name
    for key, line_ in zip(ar.KEYS, lines[1:]):
        got = np.array(line_.split(), dtype=np.int64).reshape(np.asarray(k["want"][key]).shape)
        np.testing.assert_array_equal(got, k["want"][key], err_msg="%s: %s" % (name, key))
