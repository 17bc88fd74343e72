"""CPU-only: the host side of the wide forms of the solver and the case generator (csrc/sim_mapf_wide.hip,
csrc/sim_cases_wide.hip; maps up to 256 x 256, horizons up to 1024) - header / loader / build list / argument checks / the
workspace formula / the `wide` keyword - and the inputs of tests/test_gpu_wide_maps.py with the restatements' answers to them
(tests/mapf_restatement.py and tests/cases_restatement.py, unchanged: they are size-agnostic), made once and shared."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import cases_restatement as cr
import mapf_restatement as mr
from conftest import ROOT

ENTRIES = ("magat_sim_mapf_wide_workspace_bytes", "magat_sim_mapf_plan_wide", "magat_sim_cases_generate_wide")
BOUNDARIES = (63, 127, 191)      # the last column of a word, the last row of a wavefront


def documented_workspace_bytes(C, H, W, T):
    """include/magat_hip.h: C * T * 6 * rows(H) * words(W) * 8, rows = 64 * ceil(H / 64), words = 1, 2 or 4."""
    return C * T * 6 * (64 * -(-H // 64)) * (1 if W <= 64 else 2 if W <= 128 else 4) * 8


# ---- the inputs of the GPU tests: name -> (map, start, goal, order or None, T) ---------------------------------------------------
def hops(H, W):
    """An open H x W map, one case.  Across every word boundary (columns b | b + 1) and wave boundary (rows b | b + 1) on the
    map: a single agent in each direction, a head-on pair in one line (one of them has to step aside and wait), and a
    diagonal hop over the crossing of the first row and column boundary.  Hops of 3 to 5 cells, arrivals below 10."""
    start, goal = [], []

    def add(s, g):
        start.append(s)
        goal.append(g)

    for b in BOUNDARIES:
        if b + 2 < W:
            r = min(b // 8, H - 4)      # three free rows of their own per boundary
            add((r, b - 1), (r, b + 2))
            add((r + 1, b + 2), (r + 1, b - 1))
            add((r + 3, b - 1), (r + 3, b + 2))      # the pair, in one row
            add((r + 3, b + 2), (r + 3, b - 1))
        elif b + 1 < W:                              # W = b + 2: the last column alone is in the next word
            add((0, b - 2), (0, b + 1))
            add((1, b + 1), (1, b - 2))
        if b + 2 < H:
            c = min(20 + b // 8, W - 4)
            add((b - 1, c), (b + 2, c))
            add((b + 2, c + 1), (b - 1, c + 1))
            add((b - 1, c + 3), (b + 2, c + 3))
            add((b + 2, c + 3), (b - 1, c + 3))
        elif b + 1 < H:
            add((b - 2, W - 1), (b + 1, W - 1))
            add((b + 1, W - 2), (b - 2, W - 2))
    if H > 65 and W > 65:
        add((62, 62), (65, 65))
        add((65, 61), (62, 66))
    m = np.zeros((H, W), dtype=np.uint8)
    assert len(set(start)) == len(start) and len(set(goal)) == len(goal)
    return m, np.array([start], dtype=np.int32), np.array([goal], dtype=np.int32)


def corridors():
    """70 x 130, a map per case, walls everywhere but: a one-cell corridor over column 63 | 64 (row 5, columns 60 .. 67) with a
    head-on pair - with a pocket at (6, 65), where the second agent waits, and closed (unsolved in any order: the swap rule
    across the word boundary); the same over row 63 | 64 (column 5, rows 60 .. 67, pocket (65, 6)); a goal at (5, 64) that
    the first agent crosses at t = 5; and a dead end at (5, 62 .. 64) that needs one promotion."""
    def blank():
        return np.ones((70, 130), dtype=np.uint8)

    maps, start, goal = [], [], []
    for pocket in (True, False):
        m = blank()
        m[5, 60:68] = 0
        if pocket:
            m[6, 65] = 0
        maps.append(m)
        start.append([(5, 60), (5, 67)])
        goal.append([(5, 67), (5, 60)])
        m = blank()
        m[60:68, 5] = 0
        if pocket:
            m[65, 6] = 0
        maps.append(m)
        start.append([(60, 5), (67, 5)])
        goal.append([(67, 5), (60, 5)])
    m = blank()
    m[5, 59:67] = 0
    m[4, 64] = 0
    maps.append(m)
    start.append([(5, 59), (4, 64)])
    goal.append([(5, 66), (5, 64)])
    m = blank()
    m[5, 62:65] = 0
    m[6, 63] = 0
    maps.append(m)
    start.append([(5, 63), (5, 64)])
    goal.append([(5, 63), (5, 62)])
    return np.stack(maps), np.array(start, dtype=np.int32), np.array(goal, dtype=np.int32)


def ring(H, W):
    """Only the outermost ring free: four agents walk it clockwise into the four corners - the last bit of the last word, the
    last lane of the last wave.  A shift that wrapped would arrive in 2 steps."""
    m = np.ones((H, W), dtype=np.uint8)
    m[0, :] = m[H - 1, :] = m[:, 0] = m[:, W - 1] = 0
    start = np.array([[[0, 1], [1, W - 1], [H - 1, W - 2], [H - 2, 0]]], dtype=np.int32)
    goal = np.array([[[0, W - 1], [H - 1, W - 1], [H - 1, 0], [0, 0]]], dtype=np.int32)
    return m, start, goal


def long_serpentine():
    """12 x 70: row 0 a wall with one pocket at (0, 10); below it a serpentine through rows 1, 3, .. 11 (424 steps from (1, 0) to
    its end (11, 0)).  Agent 0 walks all of it; agent 1 stands in the pocket, ahead of agent 0 and behind it in the order, so
    it has to wait until agent 0 has passed, then follows it to the cell before the end."""
    m = np.ones((12, 70), dtype=np.uint8)
    m[0, 10] = 0
    for i, r in enumerate(range(1, 12, 2)):
        m[r, :] = 0
        if r + 1 < 12:
            m[r + 1, 69 if i % 2 == 0 else 0] = 0
    return m, np.array([[[1, 0], [0, 10]]], dtype=np.int32), np.array([[[11, 0], [11, 1]]], dtype=np.int32)


def clusters(seed, C, H, W, N, density, batched_map=False):
    """C cases of N agents whose starts and goals lie within a 9 x 9 window of the largest free component - the windows sit on
    the word / wave boundary, in the corners and inside, so the hops are short and the restatement stays cheap."""
    rng = np.random.default_rng(seed)
    centres = [(63, 63), (63, 10), (10, 63), (H - 5, W - 5), (30, 30), (4, 4), (63, 40), (40, 63)]

    def one(m, k):
        comp = mr.largest_component(m == 0)
        r0, c0 = centres[k % len(centres)]
        near = comp[(abs(comp[:, 0] - r0) <= 4) & (abs(comp[:, 1] - c0) <= 4)]
        assert len(near) >= 2 * N
        return near[rng.permutation(len(near))[:N]], near[rng.permutation(len(near))[:N]]

    if batched_map:
        maps = [(rng.random((H, W)) < density).astype(np.uint8) for _ in range(C)]
        pairs = [one(m, k) for k, m in enumerate(maps)]
        return np.stack(maps), np.stack([p[0] for p in pairs]).astype(np.int32), np.stack([p[1] for p in pairs]).astype(np.int32)
    m = (rng.random((H, W)) < density).astype(np.uint8)
    pairs = [one(m, k) for k in range(C)]
    return m, np.stack([p[0] for p in pairs]).astype(np.int32), np.stack([p[1] for p in pairs]).astype(np.int32)


HOP_SHAPES = ((65, 65), (10, 65), (65, 10), (70, 130), (129, 129), (256, 256))


@functools.lru_cache(maxsize=None)
def batch(name):
    if name.startswith("hops"):
        H, W = (int(v) for v in name[4:].split("x"))
        return hops(H, W) + (None, 16)
    if name == "corridors":
        return corridors() + (None, 24)
    if name == "ring256":
        return ring(256, 256) + (None, 300)
    if name == "ring65x130":
        return ring(65, 130) + (None, 160)
    if name == "serpentine_T1024":
        return long_serpentine() + (None, 1024)
    if name == "serpentine_one_short":      # the horizon ends one layer before agent 0's arrival
        return long_serpentine() + (None, 424)
    if name == "clusters65":
        return clusters(41, 40, 65, 65, 6, 0.25) + (None, 32)
    if name == "maps_and_order":
        m, s, g = clusters(42, 6, 65, 65, 6, 0.1, batched_map=True)
        rng = np.random.default_rng(43)
        return m, s, g, np.stack([rng.permutation(6) for _ in range(6)]).astype(np.int32), 32
    if name == "bad_cases":                 # case 1: an order that is no permutation; case 2: two agents with one start
        m, s, g, _, T = batch("clusters65")
        s, g = s[:4].copy(), g[:4].copy()
        order = np.tile(np.arange(6, dtype=np.int32), (4, 1))
        order[1] = [0, 0, 1, 2, 3, 4]
        s[2, 4] = s[2, 1]
        return m, s, g, order, T
    raise KeyError(name)


HOP_NAMES = tuple("hops%dx%d" % hw for hw in HOP_SHAPES)
PLAN_NAMES = HOP_NAMES + ("corridors", "ring256", "ring65x130", "serpentine_T1024", "serpentine_one_short", "clusters65",
                          "maps_and_order", "bad_cases")
SOLVE_NAMES = ("corridors", "clusters65")


@functools.lru_cache(maxsize=None)
def expected_plan(name):
    m, s, g, order, T = batch(name)
    return mr.plan_batch(m, s, g, order, T)


@functools.lru_cache(maxsize=None)
def expected_solve(name):
    m, s, g, _, T = batch(name)
    return mr.solve_batch(m, s, g, T, retries=8)


def big_room_map():
    """256 x 256: the largest free component (a room with a pillar) lies wholly in words 2 - 3 and rows 128 and above; three
    smaller rooms elsewhere, one of them found first."""
    m = np.ones((256, 256), dtype=np.uint8)
    m[3:40, 3:60] = 0
    m[10:60, 140:250] = 0
    m[140:250, 10:100] = 0
    m[130:252, 129:256] = 0
    m[180:200, 180:200] = 1
    return m


def few_cells_map(H, W):
    m = np.ones((H, W), dtype=np.uint8)
    m[H - 1, W - 4:] = 0      # four free cells in the last row and word
    return m


# name -> (kind, C, H, W, N, density, complexity, seed, maps or None)
@functools.lru_cache(maxsize=None)
def gen_case(name):
    if name == "uni65":
        return ("uniform", 6, 65, 65, 10, 0.2, 0.0, 51, None)
    if name == "uni70x130":
        return ("uniform", 2, 70, 130, 10, 0.3, 0.0, 52, None)
    if name == "uni256":
        return ("uniform", 1, 256, 256, 300, 0.1, 0.0, 53, None)
    if name == "maze65":
        return ("maze", 3, 65, 65, 10, 0.3, 0.05, 54, None)
    if name == "maze130x70":
        return ("maze", 2, 130, 70, 10, 0.3, 0.05, 55, None)
    if name == "given70x130":      # a full-width serpentine, a checkerboard, four free cells for four agents
        return ("given", 3, 70, 130, 4, 0.0, 0.0, 56, np.stack([cr.serpentine(70, 130), cr.checkerboard(70, 130), few_cells_map(70, 130)]))
    if name == "given256":
        return ("given", 2, 256, 256, 8, 0.0, 0.0, 57, np.stack([np.zeros((256, 256), dtype=np.uint8), big_room_map()]))
    raise KeyError(name)


GEN_NAMES = ("uni65", "uni70x130", "uni256", "maze65", "maze130x70", "given70x130", "given256")


@functools.lru_cache(maxsize=None)
def expected_cases(name):
    kind, C, H, W, N, density, complexity, seed, maps = gen_case(name)
    return cr.generate(kind, C, H, W, N, density, complexity, seed=seed, maps=maps)


# ---- the host side ------------------------------------------------------------------------------------------------------------
def test_wide_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    assert "sim_mapf_wide.hip" in build_native.SOURCES and "sim_cases_wide.hip" in build_native.SOURCES
    assert re.search(r"^size_t magat_sim_mapf_wide_workspace_bytes\(int C, int H, int W, int T\);", hdr, re.M)
    assert re.search(r"^int magat_sim_mapf_plan_wide\(", hdr, re.M) and re.search(r"^int magat_sim_cases_generate_wide\(", hdr, re.M)
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS, name
    # the same arguments as the 64 x 64 forms
    assert nat._SIGNATURES["magat_sim_mapf_plan_wide"] == nat._SIGNATURES["magat_sim_mapf_plan"]
    assert nat._SIGNATURES["magat_sim_cases_generate_wide"] == nat._SIGNATURES["magat_sim_cases_generate"]
    assert len(nat._SIGNATURES["magat_sim_mapf_wide_workspace_bytes"][1]) == 4
    # the multi-word board helpers have one home, next to the single-word ones
    csrc = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
    assert "struct wboard" in open(os.path.join(csrc, "row_board.h")).read()
    for src in ("sim_mapf_wide.hip", "sim_cases_wide.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "row_board.h"' in text and "struct wboard" not in text and "asm" not in text
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_workspace_formula():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for C, H, W, T in ((1, 65, 65, 32), (3, 10, 65, 257), (2, 65, 10, 100), (2, 70, 130, 24), (1, 129, 129, 16), (8, 200, 200, 1024),
                       (1, 256, 256, 1024), (4, 20, 20, 300), (1, 64, 192, 7), (1, 193, 64, 7)):
        assert lib.magat_sim_mapf_wide_workspace_bytes(C, H, W, T) == documented_workspace_bytes(C, H, W, T), (C, H, W, T)
    assert documented_workspace_bytes(1, 256, 256, 1024) == 1024 * 6 * 256 * 4 * 8
    for bad in ((0, 65, 65, 8), (1, 0, 65, 8), (1, 65, -1, 8), (1, 65, 65, 0), (1, 257, 65, 8), (1, 65, 257, 8)):
        assert lib.magat_sim_mapf_wide_workspace_bytes(*bad) == 0, bad


def test_solver_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    big = 1 << 50

    def call(map_=one, H=200, W=200, start=one, paths=one, ws=one, ws_bytes=big, C=2, N=4, T=512):
        return lib.magat_sim_mapf_plan_wide(map_, 0, H, W, start, one, None, paths, one, one, one, one, ws, ws_bytes, C, N, T, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf"])
    assert call(map_=None) == -5 and call(start=None) == -5 and call(paths=None) == -5 and call(ws=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1 and call(T=0) == -1
    assert call(H=257) == -2 and call(W=257) == -2 and call(T=1025) == -2
    # 256 x 256 and T = 1024 pass the limits: the next check is the workspace's size, then its alignment (-3)
    assert call(H=256, W=256, T=1024, ws_bytes=documented_workspace_bytes(2, 256, 256, 1024) - 1) == -2
    assert call(H=256, W=256, T=1024, ws=odd, ws_bytes=documented_workspace_bytes(2, 256, 256, 1024)) == -3
    assert call(H=65, W=65, T=257, ws=odd) == -3 and call(H=1, W=1, T=1, ws=odd) == -3
    assert call(map_=None, H=0, T=9999) == -5 and call(H=0, T=9999) == -1      # null, then sizes, then limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf"]) == before              # a refused call is not counted as a launch


def test_generator_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one = ctypes.c_void_p(16)
    MAZE, UNIFORM, GIVEN = 0, 1, 2

    def call(kind=MAZE, map_in=None, H=200, W=200, aisles=10, walk=2, first=0, map_out=one, start=one, valid=one, C=2, N=4):
        return lib.magat_sim_cases_generate_wide(kind, map_in, 0, H, W, aisles, walk, 1 << 30, 1, first, map_out, start, one, one,
                                                 valid, C, N, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf"])
    assert call(map_out=None) == -5 and call(start=None) == -5 and call(valid=None) == -5
    assert call(kind=GIVEN, map_in=None) == -5
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1
    assert call(kind=3) == -1 and call(kind=-1) == -1 and call(aisles=-1) == -1 and call(walk=-1) == -1
    assert call(H=257) == -2 and call(W=257) == -2 and call(kind=UNIFORM, H=257) == -2
    assert call(N=4097) == -2 and call(H=256, W=256, N=4097) == -2 and call(H=10, W=65, N=651) == -2
    assert call(H=3) == -2 and call(W=2) == -2 and call(aisles=4097) == -2 and call(walk=1025) == -2      # the maze bounds stay
    assert call(first=-1) == -2 and call(first=(1 << 32) - 1) == -2
    assert call(map_out=None, H=0, W=257) == -5 and call(H=0, W=257) == -1 and call(kind=7, W=257) == -1  # null, sizes, limits
    # 256 x 256 with 4096 agents passes every check but the last one
    assert call(H=256, W=256, N=4096, first=-1) == -2 and call(H=256, W=256, N=4096, kind=GIVEN, map_in=None) == -5
    assert lib.magat_form_count(nat.FORMS["sim_mapf"]) == before


def test_wide_keyword_on_cpu_tensors_raises_and_the_default_horizon():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import cases, mapf
    m = torch.zeros(70, 70, dtype=torch.uint8)
    s = torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        mapf.plan_prioritized(m, s, s, wide=True)
    with pytest.raises(nat.MagatNativeError):
        mapf.solve_cases(m, s, s, wide=True)
    with pytest.raises(nat.MagatNativeError):
        cases.generate_cases(2, 70, 70, 3, device="cpu", wide=True)
    with pytest.raises(nat.MagatNativeError):
        cases.generate_cases(2, 70, 70, 3, obstacle_map=m, wide=True)
    assert mapf.default_horizon(65, 65, 100, wide=True) == 360 and mapf.default_horizon(200, 200, 1000, wide=True) == 1024
    assert mapf.default_horizon(20, 20, 10, wide=True) == mapf.default_horizon(20, 20, 10) == 90
    assert mapf.default_horizon(65, 65, 100) == mapf.default_horizon(65, 65, 100, wide=False) == 256


# ---- the yardsticks at this size ------------------------------------------------------------------------------------------------
def test_restatements_on_wide_hand_maps():
    """What the GPU tests are there for, in the restatement alone."""
    m, s, g, _, T = batch("corridors")
    out = expected_plan("corridors")
    assert out["solved"].tolist() == [1, 1, 0, 0, 1, 0] and out["failed_agent"].tolist() == [-1, -1, 1, 1, -1, 1]
    for c, pocket in ((0, (6, 65)), (1, (65, 6))):      # the second agent of the pair passes its time in and around the pocket
        p = [tuple(v) for v in out["paths"][c, 1]]
        t_pass = [tuple(v) for v in out["paths"][c, 0]].index((pocket[0] - 1, pocket[1]) if c == 0 else (pocket[0], pocket[1] - 1))
        assert p[t_pass] == pocket                   # it stands in the pocket while the first agent passes its mouth
        assert out["lengths"][c, 0] == 8 and out["lengths"][c, 1] == 12      # 7 steps apart, 4 steps lost
    assert tuple(out["paths"][4, 0, 5]) == (5, 64) and out["lengths"][4, 1] - 1 > 5      # the goal is crossed at t = 5
    solved = expected_solve("corridors")
    assert solved["solved"].tolist() == [1, 1, 0, 0, 1, 1] and solved["rounds"].tolist() == [1, 1, 9, 9, 1, 2]
    for c in np.nonzero(solved["solved"])[0]:
        assert mr.check_schedule(m[c], s[c], g[c], solved["paths"][c], solved["lengths"][c]) is None, c
    # the serpentine: 424 steps, the follower waits in its pocket until the leader has passed
    out = expected_plan("serpentine_T1024")
    assert out["solved"].tolist() == [1] and out["lengths"].tolist() == [[425, 425]]
    assert tuple(out["paths"][0, 0, 10]) == (1, 10) and tuple(out["paths"][0, 1, 10]) == (0, 10) and tuple(out["paths"][0, 1, 11]) == (1, 10)
    short = expected_plan("serpentine_one_short")
    assert short["solved"].tolist() == [0] and short["failed_agent"].tolist() == [0]
    for name, steps in (("ring256", 254), ("ring65x130", None)):
        out = expected_plan(name)
        assert out["solved"].tolist() == [1]
        if steps:
            assert out["lengths"].tolist() == [[steps + 1] * 4]
    assert expected_plan("ring65x130")["lengths"].tolist() == [[129, 64, 129, 64]]
    for name in HOP_NAMES:
        out = expected_plan(name)
        assert out["solved"].tolist() == [1] and out["makespan"][0] < 12, name
        m, s, g, _, T = batch(name)
        assert mr.check_schedule(m, s[0], g[0], out["paths"][0], out["lengths"][0]) is None, name
    first, after = expected_plan("clusters65"), expected_solve("clusters65")
    assert int(first["solved"].sum()) == 33 and int(after["solved"].sum()) == 39 and int(after["rounds"].max()) == 9      # promotions
    bad = expected_plan("bad_cases")
    assert bad["failed_agent"].tolist()[1:3] == [-2, 4]


def test_case_restatement_on_wide_hand_maps():
    out = expected_cases("given70x130")
    snake = cr.serpentine(70, 130)
    assert out["free_cells"].tolist() == [int((snake == 0).sum()), 1, 4] and out["valid"].tolist() == [1, 0, 0]
    assert (out["map"][0] == snake).all()
    out = expected_cases("given256")
    room = 122 * 127 - 400
    assert out["free_cells"].tolist() == [65536, room] and out["valid"].tolist() == [1, 1]
    kept = np.argwhere(out["map"][1] == 0)
    assert kept[:, 0].min() == 130 and kept[:, 1].min() == 129 and kept[:, 1].max() == 255
    assert expected_cases("uni256")["valid"].tolist() == [1]
    rows = expected_cases("uni256")["start"][0, :, 0]
    assert len({int(r) // 64 for r in rows}) == 4      # starts in all four waves' rows
