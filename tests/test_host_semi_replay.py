"""CPU-only: SemiLG states from the schedule alone (magat_sim_replayed_states[_wide] in csrc/sim_guidance.hip /
csrc/sim_guidance_wide.hip, replayed_semi_states, expert_samples(replay=True), ExpertMemory(replay=True)).  The yardstick is
tests/semi_replay_restatement.py - the closed form "seen so far AND blocked" of an agent's remembered map: pinned here against
the sequentially carried view of tests/guidance_restatement.py and against the stored `x` of every SemiLG fixture the real
reference made, with both decodes of the history.  Then the host side of the two entries - header / loader / exports / argument
refusals -, the kernels compiled for the host (tools/host_wave/semi_replay_check.cpp) against the restatement, and the Python
surface on CPU tensors."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_restatement as gr
import semi_replay_restatement as sr
from conftest import ROOT, golden_paths

STEP_FIXTURES = golden_paths("guid_SemiLG_") + golden_paths("guidw_SemiLG_")
STEP_IDS = [os.path.basename(p)[:-4] for p in STEP_FIXTURES]
EXPERT = golden_paths("expert_n12_map10_dense_SemiLG_S_fixed")[0]
FOV = 9


def guidance_of(path):
    return "SemiLG_SD" if "SemiLG_SD" in path else "SemiLG_S"


# ---- the closed form against the carried view and the reference's own tensors -----------------------------------------------------------
@pytest.mark.parametrize("path", STEP_FIXTURES, ids=STEP_IDS)
def test_replayed_view_and_states_equal_the_carried_ones_and_the_reference(path):
    z = np.load(path, allow_pickle=False)
    g = guidance_of(path)
    B, T, N, _ = z["pos"].shape
    assert len(STEP_FIXTURES) == 9
    for b in range(B):
        m, goal = z["map"][b], z["goal"][b]
        view = gr.new_agent_view(N, m.shape[0], m.shape[1], FOV)
        for t in range(T):
            carried = gr.guided_states(m, z["pos"][b, t], goal, g, FOV, agent_view=view)      # updates `view`: steps 0..t seen
            cells = sr.table_cells(z["pos"][b], t)
            np.testing.assert_array_equal(sr.replayed_view(m, cells, goal, FOV), view, err_msg="view %d %d" % (b, t))
            x = sr.replayed_states(m, z["pos"][b, t], goal, cells, g, FOV)
            np.testing.assert_array_equal(x, carried, err_msg="carried %d %d" % (b, t))
            np.testing.assert_array_equal(x, z["x"][b, t], err_msg="reference %d %d" % (b, t))


def test_expert_fixture_both_decodes_and_the_goal_rule():
    z = np.load(EXPERT, allow_pickle=False)
    C, T, N, _ = z["pos"].shape
    Lcap = z["paths"].shape[2] + 3
    behind = 0
    for c in range(C):
        m, goal = z["map"][c], z["goal"][c]
        packed = sr.pack_cells(z["paths"][c], z["lengths"][c], Lcap)
        steps = int(z["makespan"][c]) + 1
        assert z["valid"][c].sum() == steps
        view = gr.new_agent_view(N, m.shape[0], m.shape[1], FOV)
        for t in range(steps):
            a, s = sr.table_cells(z["pos"][c], t), sr.store_cells(packed, z["lengths"][c], goal, t)
            np.testing.assert_array_equal(a, s, err_msg="decode %d %d" % (c, t))
            behind += int((t >= z["lengths"][c]).sum())
            assert all((s[t, n] == goal[n]).all() for n in range(N) if t >= z["lengths"][c, n])      # the goal rule
            carried = gr.guided_states(m, z["pos"][c, t], goal, "SemiLG_S", FOV, agent_view=view)
            np.testing.assert_array_equal(sr.replayed_view(m, s, goal, FOV), view)
            x = sr.replayed_states(m, z["pos"][c, t], goal, s, "SemiLG_S", FOV)
            np.testing.assert_array_equal(x, carried)
            np.testing.assert_array_equal(x, z["x"][c, t], err_msg="reference %d %d" % (c, t))
    assert behind > 0                                     # the fixture does hold steps behind an agent's path length


def test_rule_edges_of_the_restatement():
    m = np.zeros((6, 7), dtype=np.uint8)
    m[2, 3] = 1
    goal = np.array([[5, 6], [9, 9]])                     # agent 1's goal is off the map: it is never searched and sees nothing
    cells = np.array([[[0, 0], [1, 1]], [[-1, 0], [1, 2]], [[0, 0], [1, 2]]])      # agent 0's step 1 is off the map
    v = sr.replayed_view(m, cells, goal, 3)
    assert v.shape == (2, 8, 9) and not v[1].any()
    want = np.zeros((8, 9), dtype=np.uint8)
    want[0, 0:3] = 1                                      # the window of (0, 0): padded rows 0..2, columns 0..2; ring cells blocked
    want[0:3, 0] = 1
    np.testing.assert_array_equal(v[0], want)


# ---- the entry points: declared, bound, exported; refusals -------------------------------------------------------------------------------
def test_replay_entries_are_declared_bound_and_exported():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "sim_guidance_parts.h" in build_native.HEADERS
    for name, src, nargs in (("magat_sim_replayed_states", "sim_guidance.hip", 12),
                             ("magat_sim_replayed_states_wide", "sim_guidance_wide.hip", 14)):
        text = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", src)).read()
        assert src in build_native.SOURCES and re.search(r'extern "C" int %s\(' % name, text)
        assert "MAGAT_FORM_SIM_REPLAY" in text and "MAGAT_TAG_SIM_GUIDED" in text and "guide_history_walk" in text
        assert len(re.findall(r"while \(nopen > 0\)", text)) == 1      # ONE copy of the search
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl and name in nat.EXPORTED_SYMBOLS
        res, sig = nat._SIGNATURES[name]
        assert res is ctypes.c_int and len(decl.group(1).split(",")) == len(sig) == nargs
    fields = re.search(r"typedef struct magat_sim_history_desc \{(.*?)\} magat_sim_history_desc;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", fields))
    assert [n for g in names for n in g if n] == [f for f, _ in nat.SimHistoryDesc._fields_]
    assert ctypes.sizeof(nat.SimHistoryDesc) == 6 * 8 + 3 * 4 + 4
    form = int(re.search(r"#define MAGAT_FORM_SIM_REPLAY (\d+)", common).group(1))
    assert form == nat.FORMS["sim_replay"] == 24 == nat.FORMS["chain_tile16"] + 1
    assert nat.FORMS["sim_guided"] == 16 and nat.TAG_SIM_GUIDED == 26
    assert "replayed_semi_states" in pkg.__all__ and callable(pkg.replayed_semi_states)
    lib = nat.lib()                                       # loads without a GPU
    assert lib.magat_abi_version() == 9 and lib.magat_form_count(form) >= 0


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_replay_refusals_are_uncounted(wide):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    p = 16
    before = lib.magat_form_count(nat.FORMS["sim_replay"]), lib.magat_form_count(nat.FORMS["sim_guided"])

    def desc(**kw):
        f = dict(row_case=p, row_step=p, pos_table=p, cells=None, lengths=None, goal=None, cases=3, T=8, Lcap=0)
        f.update(kw)
        return nat.SimHistoryDesc(**f)

    store = dict(pos_table=None, cells=p, lengths=p, goal=p, T=0, Lcap=8)

    def call(d, ptrs=(p, p, p, p), shape=(10, 10), FOV=9, B=2, N=3, ws=p, ws_bytes=1 << 30):
        a = [ptrs[0], 1, shape[0], shape[1], ptrs[1], ptrs[2], ptrs[3], FOV, B, N, ctypes.byref(d) if d is not None else None]
        if wide:
            return lib.magat_sim_replayed_states_wide(*a, ws, ws_bytes, None)
        return lib.magat_sim_replayed_states(*a, None)

    for i in range(4):
        ptrs = [p] * 4
        ptrs[i] = None
        assert call(desc(), ptrs=tuple(ptrs)) == -5, i
    assert call(desc(), B=0) == -1 and call(desc(), N=-1) == -1 and call(desc(), shape=(0, 10)) == -1
    assert call(desc(), FOV=8) == -1 and call(desc(), FOV=31) == -2 and call(desc(), FOV=1) == -2
    big = (257, 10) if wide else (55, 10)
    assert call(desc(), shape=big) == -2 and call(desc(), shape=big[::-1]) == -2
    assert call(None) == -5 and call(desc(row_case=None)) == -5 and call(desc(row_step=None)) == -5
    assert call(desc(pos_table=None)) == -5                                            # neither source
    assert call(desc(**dict(store, goal=None))) == -5 and call(desc(**dict(store, cells=None))) == -5      # half a store
    assert call(desc(cells=p, lengths=p, goal=p, Lcap=8)) == -2                        # both sources
    assert call(desc(lengths=p)) == -2
    assert call(desc(cases=0)) == -1 and call(desc(T=0)) == -1 and call(desc(**dict(store, Lcap=0))) == -1
    assert call(desc(T=1025)) == -2
    if wide:
        assert call(desc(), ws=None) == -5 and call(desc(), ws_bytes=8) == -2 and call(desc(), ws=20) == -3
        assert call(None, ws=None) == -5                                               # the history before the workspace
    assert (lib.magat_form_count(nat.FORMS["sim_replay"]), lib.magat_form_count(nat.FORMS["sim_guided"])) == before


# ---- the kernels themselves, compiled for the host (tools/host_wave) ------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "semi_replay_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "semi_replay_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, tmp_path, maps, pos, goal, row_case, row_step, wide, table=None, store=None, fov=FOV):
    (tmp_path / "case.txt").write_text(sr.dump_case(maps, pos, goal, row_case, row_step, fov, wide, table=table, store=store))
    run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    rc, x = sr.parse_result(run.stdout, pos.shape[0], pos.shape[1], fov)
    assert rc == 0
    return x


def dense_rows():
    """Rows of the dense 10 x 10 expert fixture (windows hang over every border): a first step, steps behind path lengths, one
    (case, step) twice, cases and steps mixed."""
    z = np.load(EXPERT, allow_pickle=False)
    rows = [(0, 0), (1, 5), (3, int(z["makespan"][3])), (1, 5), (4, 2)]
    case, step = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return z, case, step


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("source", ["table", "store"])
def test_host_kernel_equals_the_restatement_on_the_expert_fixture(replay_check, tmp_path, source, wide):
    z, case, step = dense_rows()
    maps, pos, goal = z["map"][case], z["pos"][case, step], z["goal"][case]
    Lcap = z["paths"].shape[2] + 3
    packed = np.stack([sr.pack_cells(z["paths"][c], z["lengths"][c], Lcap) for c in range(z["pos"].shape[0])])
    if source == "table":
        x = run_check(replay_check, tmp_path, maps, pos, goal, case, step, wide, table=z["pos"])
    else:
        x = run_check(replay_check, tmp_path, maps, pos, goal, case, step, wide, store=(packed, z["lengths"], z["goal"]))
    np.testing.assert_array_equal(x, z["x"][case, step])
    assert (step[2] >= z["lengths"][3]).any()             # that row uses the goal rule


def synthetic(H, W, N, T, seed, fov=FOV):
    """One instance of straight-ish walks on a sparse map, goals a few cells ahead: short searches, long enough histories."""
    rng = np.random.default_rng(seed)
    m = (rng.random((H, W)) < 0.12).astype(np.uint8)
    table = np.zeros((1, T, N, 2), dtype=np.int64)
    goal = np.zeros((N, 2), dtype=np.int64)
    for n in range(N):
        r, c = int(rng.integers(0, H)), int(rng.integers(0, W))
        for t in range(T):
            table[0, t, n] = (r, c)
            dr, dc = ((-1, 0), (0, -1), (1, 0), (0, 1), (0, 0))[int(rng.integers(0, 5))]
            if 0 <= r + dr < H and 0 <= c + dc < W:
                r, c = r + dr, c + dc
        goal[n] = (min(H - 1, max(0, r + int(rng.integers(-4, 5)))), min(W - 1, max(0, c + int(rng.integers(-4, 5)))))
    m[table[0, :, :, 0], table[0, :, :, 1]] = 0
    return m, table, goal


def test_host_kernel_three_words_a_row_and_an_off_map_step(replay_check, tmp_path):
    m, table, goal = synthetic(11, 125, 3, 6, seed=5)     # canvas 21 x 135: three words a row
    table[0, 2, 1] = (-1, 4)                              # a step off the map contributes nothing
    goal[2] = (11, 3)                                     # a goal off the map: that agent is not searched
    rows = np.array([5, 3])
    pos = table[0, rows]
    x = run_check(replay_check, tmp_path, np.stack([m, m]), pos, np.stack([goal, goal]), np.zeros(2, dtype=np.int64), rows, True,
                  table=table)
    on_map = goal.copy()
    on_map[2] = (10, 3)                                   # (the restatement takes no goal off the map; agents 0 and 1 do not read it)
    for i, t in enumerate(rows):
        want = sr.replayed_states(m, pos[i], on_map, sr.table_cells(table[0], t), "SemiLG_S")
        np.testing.assert_array_equal(x[i, :2], want[:2])
        np.testing.assert_array_equal(x[i, 2, [0, 2]], want[2, [0, 2]])
        assert not x[i, 2, 1].any()


# ---- the Python surface refuses without touching a device ------------------------------------------------------------------------------
def test_python_surface_refuses_on_the_host():
    from magat_pathplanning_amd import ExpertMemory, expert_samples, replayed_semi_states
    from magat_pathplanning_amd import _native as nat
    for g in ("SemiLG_S", "SemiLG_SD"):
        with pytest.raises(ValueError, match="expert_samples"):
            ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance=g)
        with pytest.raises(ValueError, match="replay=True"):
            ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance=g, replay=False)
        with pytest.raises(nat.MagatNativeError):         # past the guidance check: the memory lives on the device
            ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance=g, replay=True, device="cpu")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)   # noqa: E731
    hist = dict(case=i32(2), step=i32(2), table=i32(1, 4, 3, 2))
    with pytest.raises(ValueError, match="SemiLG"):
        replayed_semi_states(torch.zeros(10, 10), i32(2, 3, 2), i32(2, 3, 2), hist, guidance="GlobalG_S")
    with pytest.raises(nat.MagatNativeError, match="device tensor"):
        replayed_semi_states(torch.zeros(10, 10), i32(2, 3, 2), i32(2, 3, 2), hist)
    z = np.load(EXPERT, allow_pickle=False)
    with pytest.raises(nat.MagatNativeError, match="device tensor"):
        expert_samples(torch.from_numpy(z["map"]), torch.from_numpy(z["paths"]), torch.from_numpy(z["lengths"]),
                       torch.from_numpy(z["goal"]), torch.from_numpy(z["makespan"]), 7.0, guidance="SemiLG_S", replay=True)
