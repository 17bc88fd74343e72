"""CPU-only: the host side of the wide forms of the A*-guided state encodings and the move step (csrc/sim_guidance_wide.hip,
sim_move_kernel<WIDE> in csrc/sim_frontend.hip; maps up to 256 x 256) - the yardstick at the new sizes (tests/
guidance_restatement.py equals every guidw_* fixture of the real reference), header / loader / build list, the workspace
formulas, the `wide` keyword - and the inputs of tests/test_gpu_wide_loop.py with the restatement's answers to them, made once
and shared.  The move rules need no pinning here: oracle/sim_oracle.py does not depend on the map's size."""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import guidance_restatement as gr
from conftest import ROOT, golden_paths

FIXTURES = golden_paths("guidw_")
ENTRIES = ("magat_sim_guided_states_wide_workspace_bytes", "magat_sim_guided_states_wide", "magat_sim_move_wide_workspace_bytes",
           "magat_sim_move_wide", "magat_sim_step_wide")
FOV, HALF = 9, 4
GUIDE_CAP = 1024                     # DESIGN 4.9, wide form: workgroups of a launch
WORD_EDGES = (63, 127, 191, 255)     # canvas column / row b | b + 1: the last bit of a 64-bit word of a board's row


def documented_guided_workspace_bytes(B, N, H, W, fov=FOV):
    """include/magat_hip.h: min(B N, 1024) * canvas rows * canvas columns * 8."""
    return min(B * N, GUIDE_CAP) * (H + 2 * (fov // 2) + 2) * (W + 2 * (fov // 2) + 2) * 8


def documented_move_workspace_bytes(B, H, W, N):
    return B * H * W * 4


def fixture_guidance(path):
    return "_".join(os.path.basename(path).split("_")[1:3])


# ---- the inputs of the GPU guidance tests: name -> (map (H,W), pos (N,2), goal (N,2)) ----------------------------------------------
def wall_in(m, cell, keep):
    """Obstacles on the four neighbours of `cell` (where they lie on the map and hold nobody of `keep`)."""
    for dr, dc in gr.MOVES:
        r, c = cell[0] + dr, cell[1] + dc
        if 0 <= r < m.shape[0] and 0 <= c < m.shape[1] and (r, c) not in keep:
            m[r, c] = 1


def random_scene(seed, H, W, N, density=0.1):
    """A seeded random map; agent 0 at the corner (0, 0) with its goal at the opposite corner, agent 1 walled in."""
    rng = np.random.default_rng(seed)
    m = (rng.random((H, W)) < density).astype(np.uint8)
    m[0, :2] = m[1, 0] = m[H - 1, W - 1] = 0
    free = [tuple(c) for c in np.argwhere(m == 0) if tuple(c) not in {(0, 0), (0, 1), (1, 0), (H - 1, W - 1)}]
    idx = rng.permutation(len(free))
    pos = np.array([free[i] for i in idx[:N]], dtype=np.int32)
    goal = np.array([free[i] for i in idx[N:2 * N]], dtype=np.int32)
    pos[0], goal[0] = (0, 0), (H - 1, W - 1)
    wall_in(m, tuple(pos[1]), {tuple(p) for p in pos} | {(0, 0), (0, 1), (1, 0)})
    return m, pos, goal


def open256():
    """256 x 256 without obstacles but those around the walled-in agent 4.  Agents 0 .. 3 start at the four corners; map
    coordinate = canvas - 5, so the canvas edges 63|64, 127|128, 191|192, 255|256 are map 58|59, 122|123, 186|187, 250|251.  On an
    open map the search visits the rectangle between start and goal, each below 5000 cells:
        0: (0, 0) -> (125, 30)         rows 58|59, 122|123                     126 x 31
        1: (0, 255) -> (65, 185)       rows 58|59; columns 250|251, 186|187    66 x 71
        2: (255, 0) -> (185, 65)       rows 250|251, 186|187; columns 58|59    71 x 66
        3: (255, 255) -> (240, 120)    columns 250|251, 186|187, 122|123       16 x 136"""
    m = np.zeros((256, 256), dtype=np.uint8)
    pos = np.array([(0, 0), (0, 255), (255, 0), (255, 255), (130, 130)], dtype=np.int32)
    goal = np.array([(125, 30), (65, 185), (185, 65), (240, 120), (10, 10)], dtype=np.int32)
    wall_in(m, (130, 130), set())
    return m, pos, goal


def serpentine():
    """25 x 200: walls on the odd rows, open at the right end, then the left, in turn: one path of 13 * 200 + 12 = 2612 cells from
    (0, 0) to (24, 199), so that g passes 2^11; agent 1 walks it the other way."""
    m = np.zeros((25, 200), dtype=np.uint8)
    for k in range(12):
        m[2 * k + 1, :] = 1
        m[2 * k + 1, 199 if k % 2 == 0 else 0] = 0
    pos = np.array([(0, 0), (24, 199)], dtype=np.int32)
    goal = np.array([(24, 199), (0, 0)], dtype=np.int32)
    return m, pos, goal


SCENES = {"first_refused_55x54": lambda: random_scene(5554, 55, 54, 8),      # canvas 65 x 64: the first shape with two words
          "two_words_118": lambda: random_scene(118, 118, 118, 8),           # canvas 128: the last with two words
          "three_words_119": lambda: random_scene(119, 119, 119, 8),         # canvas 129: the first with three
          "open256": open256, "serpentine": serpentine}
SCENE_GUIDANCE = {"first_refused_55x54": ("GlobalG_S", "GlobalG_SD", "SemiLG_SD"), "two_words_118": ("GlobalG_SD", "SemiLG_SD"),
                  "three_words_119": ("GlobalG_SD", "SemiLG_S"), "open256": ("GlobalG_SD", "SemiLG_SD"),
                  "serpentine": ("GlobalG_S", "SemiLG_SD")}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, guidance):
    """(x (N,3,11,11) uint8, agent_view after the call or None, stats) of the restatement."""
    m, pos, goal = scene(name)
    view = gr.new_agent_view(len(pos), m.shape[0], m.shape[1], FOV) if guidance.startswith("SemiLG") else None
    stats = []
    x = gr.guided_states(m, pos, goal, guidance, FOV, view, stats)
    x.setflags(write=False)
    return x, view, stats


# ---- the inputs of the GPU move tests -----------------------------------------------------------------------------------------------
def move_scene(H, W, batched_map, seed, B=3, N=40):
    """B instances of N = 40 agents: one at each corner, 36 packed into a 12 x 12 cluster (a quarter of its cells, a tenth of
    the others obstacles), so that most steps have swaps, several claims on a cell, obstacle stops and cascades; goals inside
    the cluster as well.  Returns map (H,W) or (B,H,W), pos, goal (B,N,2)."""
    rng = np.random.default_rng(seed)
    maps = (rng.random((B if batched_map else 1, H, W)) < 0.02).astype(np.uint8)
    pos, goal = np.zeros((B, N, 2), np.int32), np.zeros((B, N, 2), np.int32)
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    origins = [(H - 14, W - 14), (1, W - 14), (H // 2, max(W // 2 - 6, 1))]      # the far corner: the largest cell indices
    for b in range(B):
        r0, c0 = origins[b % 3]
        for mm in (maps if batched_map else maps[:1]):
            mm[r0:r0 + 12, c0:c0 + 12] = rng.random((12, 12)) < 0.1
        m = maps[b if batched_map else 0]
        for r, c in corners:
            m[r, c] = 0
        cells = [(r0 + i, c0 + j) for i in range(12) for j in range(12) if m[r0 + i, c0 + j] == 0]
        idx = rng.permutation(len(cells))
        pos[b, :4], goal[b, :4] = corners, corners[::-1]
        pos[b, 4:] = [cells[i] for i in idx[:N - 4]]
        goal[b, 4:] = [cells[i] for i in idx[N - 4:2 * (N - 4)]]
    if not batched_map:      # one map for all: every instance's corners and agents stand on free cells of it
        for b in range(B):
            assert all(maps[0][tuple(p)] == 0 for p in pos[b])
    return (maps if batched_map else maps[0]), pos, goal


MOVE_SCENES = {"205x205": (205, 205, False, 205), "256x256": (256, 256, False, 256), "256x40_batched": (256, 40, True, 25640)}


@functools.lru_cache(maxsize=None)
def move_inputs(name):
    return move_scene(*MOVE_SCENES[name])


def corner_keys(H, W):
    """The action keys that send the four corner agents out of the arena: up, up, down, down."""
    return [0, 0, 2, 2]


def oracle_flag_bits(fl):
    return (1 if fl["out_boundary"].any() else 0) | (2 if fl["swap"] else 0) | (4 if fl["wall"] else 0) | (8 if fl["collide"] else 0)


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_fixture_set():
    names = [os.path.basename(p) for p in FIXTURES]
    assert len(names) == 6 and sum("n24_map65" in n for n in names) == 4 and sum("n12_map70x130" in n for n in names) == 2
    assert not [n for n in names if n.startswith("guid_")]
    for p in FIXTURES:
        assert os.path.getsize(p) < 4 * 50592 // 2
        z = np.load(p, allow_pickle=False)
        assert sorted(z.files) == ["goal", "map", "pos", "x"]
        assert z["map"].dtype == np.uint8 and z["x"].dtype == np.uint8 and z["pos"].dtype == np.int32 and z["goal"].dtype == np.int32


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_restatement_equals_the_reference_at_the_wide_sizes(path):
    z = np.load(path, allow_pickle=False)
    g = fixture_guidance(path)
    for b in range(len(z["map"])):
        if g.startswith("SemiLG"):
            view = gr.new_agent_view(z["goal"].shape[1], z["map"].shape[1], z["map"].shape[2], FOV)
            for t in range(z["pos"].shape[1]):
                x = gr.guided_states(z["map"][b], z["pos"][b, t], z["goal"][b], g, FOV, view)
                np.testing.assert_array_equal(x, z["x"][b, t], err_msg="%s instance %d step %d" % (g, b, t))
        else:
            x = gr.guided_states(z["map"][b], z["pos"][b], z["goal"][b], g, FOV)
            np.testing.assert_array_equal(x, z["x"][b], err_msg="%s instance %d" % (g, b))


def test_scenes_hold_what_they_are_for():
    _, _, stats = expected("open256", "GlobalG_SD")
    rows, cols = set(), set()
    for s in stats[:4]:
        assert len(s["path"]) > 1
        for (r0, c0), (r1, c1) in zip(s["path"], s["path"][1:]):
            if min(r0, r1) in WORD_EDGES and r0 != r1:
                rows.add(min(r0, r1))
            if min(c0, c1) in WORD_EDGES and c0 != c1:
                cols.add(min(c0, c1))
    assert rows == set(WORD_EDGES) and cols == set(WORD_EDGES)
    assert all(s["pops"] < 5000 for s in stats)
    m, pos, _ = scene("open256")
    assert {tuple(p) for p in pos[:4]} == {(0, 0), (0, 255), (255, 0), (255, 255)}
    for name in SCENES:
        for g in SCENE_GUIDANCE[name]:
            st = expected(name, g)[2]
            if name != "serpentine":
                assert any(len(s["path"]) == 1 and s["pops"] == 1 for s in st), (name, g)      # the walled-in agent
    _, _, st = expected("serpentine", "GlobalG_S")
    assert len(st[0]["path"]) == 2612 and len(st[1]["path"]) == 2612 and st[0]["pops"] > 2048


def test_move_scenes_hold_what_they_are_for():
    from oracle import sim_oracle as so
    for name in MOVE_SCENES:
        m, pos, goal = move_inputs(name)
        H, W = m.shape[-2:]
        assert 4 * H * W + 16 * pos.shape[1] > 160 * 1024 or name == "256x40_batched"
        rng = np.random.default_rng(1)
        seen = 0
        for b in range(len(pos)):
            p = pos[b].astype(np.int64)
            mb = m if m.ndim == 2 else m[b]
            assert all(mb[tuple(q)] == 0 for q in p) and len({tuple(q) for q in p}) == len(p)
            for _ in range(6):
                keys = rng.integers(0, 5, len(p))
                keys[:4] = corner_keys(H, W)
                mv, fl = so.shield_moves(mb, p, so.MOVES[keys])
                seen |= oracle_flag_bits(fl)
                p = p + mv
        assert seen == 15, (name, seen)


def test_header_loader_and_build_list():
    from magat_pathplanning_amd import _native as nat, build_native
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in nat._SIGNATURES and name in nat.EXPORTED_SYMBOLS
    assert "sim_guidance_wide.hip" in build_native.SOURCES and "sim_guidance_parts.h" in build_native.HEADERS
    assert len(nat._SIGNATURES["magat_sim_guided_states_wide"][1]) == len(nat._SIGNATURES["magat_sim_guided_states"][1]) + 2
    assert len(nat._SIGNATURES["magat_sim_move_wide"][1]) == len(nat._SIGNATURES["magat_sim_move"][1]) + 2
    assert len(nat._SIGNATURES["magat_sim_step_wide"][1]) == len(nat._SIGNATURES["magat_sim_step"][1]) + 2


def test_the_keyword_is_there_and_off_by_default():
    from magat_pathplanning_amd import expert, simulator
    for fn in (simulator.batched_fov_states, simulator.batched_move, simulator.BatchedEpisode.__init__, expert.expert_samples):
        assert inspect.signature(fn).parameters["wide"].default is False, fn
    assert simulator.guided_needs_wide(55, 54, 9) and simulator.guided_needs_wide(54, 55, 9)
    assert not simulator.guided_needs_wide(54, 54, 9) and not simulator.guided_needs_wide(20, 20, 9)
    assert simulator.move_needs_wide(205, 205, 40) and not simulator.move_needs_wide(200, 200, 40)
    assert not simulator.move_needs_wide(256, 40, 40)


def test_workspace_bytes_equal_their_formulas():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    assert lib.magat_abi_version() == 9
    for B, N, H, W in ((1, 1, 20, 20), (2, 40, 65, 65), (64, 100, 65, 65), (8, 1000, 200, 200), (1, 5, 256, 256), (3, 7, 70, 130)):
        assert lib.magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV) == documented_guided_workspace_bytes(B, N, H, W)
        assert lib.magat_sim_move_wide_workspace_bytes(B, H, W, N) == documented_move_workspace_bytes(B, H, W, N)
    assert lib.magat_sim_guided_states_wide_workspace_bytes(1, 1, 256, 256, 29) == 286 * 286 * 8
    for bad in ((0, 1, 20, 20, 9), (1, 1, 257, 20, 9), (1, 1, 20, 257, 9), (1, 1, 20, 20, 8), (1, 1, 20, 20, 31)):
        assert lib.magat_sim_guided_states_wide_workspace_bytes(*bad) == 0
    for bad in ((0, 20, 20, 1), (1, 257, 20, 1), (1, 20, 257, 1), (1, 20, 20, 4097)):
        assert lib.magat_sim_move_wide_workspace_bytes(*bad) == 0


def test_argument_checks_answer_before_any_launch():
    """Null pointers and bad shapes are answered on the host: no device is needed to see the codes."""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one = 8
    assert lib.magat_sim_guided_states_wide(None, 0, 20, 20, one, one, one, 9, 1, 1, 2, 0, None, one, 1 << 30, None) == -5
    assert lib.magat_sim_guided_states_wide(one, 0, 0, 20, one, one, one, 9, 1, 1, 2, 0, None, one, 1 << 30, None) == -1
    assert lib.magat_sim_guided_states_wide(one, 0, 20, 20, one, one, one, 9, 1, 1, 1, 0, None, one, 1 << 30, None) == -2      # LocalG
    assert lib.magat_sim_guided_states_wide(one, 0, 20, 20, one, one, one, 9, 1, 1, 3, 0, None, one, 1 << 30, None) == -5      # no view
    assert lib.magat_sim_guided_states_wide(one, 0, 257, 20, one, one, one, 9, 1, 1, 2, 0, None, one, 1 << 30, None) == -2
    assert lib.magat_sim_guided_states_wide(one, 0, 20, 20, one, one, one, 9, 1, 1, 2, 0, None, None, 1 << 30, None) == -5
    need = documented_guided_workspace_bytes(1, 1, 20, 20)
    assert lib.magat_sim_guided_states_wide(one, 0, 20, 20, one, one, one, 9, 1, 1, 2, 0, None, one, need - 1, None) == -2
    assert lib.magat_sim_guided_states_wide(one, 0, 20, 20, one, one, one, 9, 1, 1, 2, 0, None, 12, need, None) == -3
    assert lib.magat_sim_move_wide(None, one, one, 0, 257, 20, one, None, None, None, None, None, 1, 1, one, 1 << 30, None) == -2
    assert lib.magat_sim_move_wide(None, one, one, 0, 20, 20, one, None, None, None, None, None, 1, 4097, one, 1 << 30, None) == -2
    assert lib.magat_sim_move_wide(None, one, one, 0, 20, 20, one, None, None, None, None, None, 1, 1, None, 1 << 30, None) == -5
    assert lib.magat_sim_move_wide(None, one, one, 0, 20, 20, one, None, None, None, None, None, 1, 1, one, 1599, None) == -2
    assert lib.magat_sim_move_wide(None, one, one, 0, 20, 20, one, None, None, None, None, None, 1, 1, 10, 1600, None) == -3
    assert lib.magat_sim_step_wide(None, one, 1 << 30, None) == -5
