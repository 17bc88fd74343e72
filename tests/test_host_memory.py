"""CPU-only: the device-resident training set (magat_pathplanning_amd/memory.py, magat_sim_expert_pick in csrc/sim_expert.hip /
csrc/sim_expert_pick.h).  The yardstick is tests/memory_restatement.py: its index mapping against a brute-force list of (case,
step) pairs, its decode against the expert_* fixtures made by the real reference (every sample of the four fixtures whose
guidance is not SemiLG).  Then the host side of the entry - header / loader / exports / argument checks -, the kernel compiled
for the host (tools/host_wave/expert_pick_check.cpp) against the restatement, the Python surface on CPU tensors, and the inputs of
the online-expert GPU test with the condition they are chosen for."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import cases_restatement as cs
import ecbs_restatement as er
import memory_restatement as mr
from conftest import ROOT, golden_paths

FIXTURES = [p for p in golden_paths("expert_") if "SemiLG" not in p]
IDS = [os.path.basename(p)[7:-4] for p in FIXTURES]
ONE_STEP = [0, 3, 0, 0, 7, 1]
# the online-expert GPU test: 6 maze cases of 10 x 10 / 4 agents from this seed; in the cases listed every agent's goal is moved
# onto its start, so an episode of "stop" actions leaves exactly the other cases failed
ONLINE = dict(C=6, H=10, W=10, N=4, seed=11, on_goal=(1, 4), maxstep=3, w_milli=1100, nodes=256)


def fixture_store(z, slack=3):
    return mr.make_store(z["paths"], z["lengths"], z["goal"], z["makespan"], int(z["lengths"].max()) + slack, radii=z["radii"],
                         maps=z["map"])


def online_cases():
    """The generator's restatement on ONLINE's arguments (generate_cases gives the same cases on the device), with the goals of
    the on_goal cases moved onto the starts."""
    k = ONLINE
    g = cs.generate("maze", k["C"], k["H"], k["W"], k["N"], seed=k["seed"])
    goal = g["goal"].copy()
    for c in k["on_goal"]:
        goal[c] = g["start"][c]
    return dict(map=g["map"], start=g["start"], goal=goal, valid=g["valid"])


def test_fixture_set():
    assert len(FIXTURES) == 4
    early = 0
    for p in FIXTURES:
        z = np.load(p, allow_pickle=False)
        early += int((z["lengths"] < (z["makespan"] + 1)[:, None]).sum())
    assert early > 0      # agents whose path ends before their case does: t = L - 1, t = L and the last step differ from t < L - 1


def test_index_mapping_against_a_brute_force_list():
    cum = np.cumsum(np.asarray(ONE_STEP, dtype=np.int64) + 1)
    pairs = [(c, t) for c, mk in enumerate(ONE_STEP) for t in range(mk + 1)]
    assert len(pairs) == int(cum[-1]) == 17
    for j, (c, t) in enumerate(pairs):
        assert mr.locate(cum, j) == (c, t, False), j
    firsts = [0] + cum[:-1].tolist()
    for c, mk in enumerate(ONE_STEP):      # the first and the last sample of every case
        assert mr.locate(cum, firsts[c]) == (c, 0, False) and mr.locate(cum, int(cum[c]) - 1) == (c, mk, False)
    assert mr.locate(cum, -1) == (0, 0, True) and mr.locate(cum, 17) == (5, 1, True)
    assert mr.locate(cum, -(1 << 40)) == (0, 0, True) and mr.locate(cum, 1 << 40) == (5, 1, True)
    _, store = mr.one_step_store()
    got = mr.pick(store, [3, 17, 2, -1, 16])
    assert got["flag"] == 1 and got["case"].tolist() == [1, 5, 1, 0, 5] and got["step"].tolist() == [2, 1, 1, 0, 1]
    assert mr.pick(store, [0, 16])["flag"] == mr.NO_ROW
    assert mr.pick(store, [5, 4, -3])["flag"] == 2
    one = mr.locate(np.array([4], dtype=np.int64), 3)      # a store of one case
    assert one == (0, 3, False)


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_decode_equals_the_reference_on_every_sample(path):
    z = np.load(path, allow_pickle=False)
    store = fixture_store(z)
    total = int(store["cum"][-1])
    assert total == int(z["valid"].sum())
    got = mr.pick(store, list(range(total)))
    assert got["flag"] == mr.NO_ROW
    pairs = [(c, t) for c in range(len(z["makespan"])) for t in range(int(z["makespan"][c]) + 1)]
    assert list(zip(got["case"].tolist(), got["step"].tolist())) == pairs
    for m, (c, t) in enumerate(pairs):
        np.testing.assert_array_equal(got["pos"][m], z["pos"][c, t], err_msg="pos of case %d step %d" % (c, t))
        np.testing.assert_array_equal(got["target"][m], z["target"][c, t], err_msg="target of case %d step %d" % (c, t))
        np.testing.assert_array_equal(got["action"][m], z["target"][c, t].argmax(-1))
        assert got["radii"][m] == z["radii"][c]
    # the padding behind a path is made from its length: garbage behind `lengths` in the input changes nothing
    dirty = z["paths"].copy()
    for c in range(dirty.shape[0]):
        for n in range(dirty.shape[1]):
            dirty[c, n, int(z["lengths"][c, n]):] = 200
    again = mr.make_store(dirty, z["lengths"], z["goal"], z["makespan"], store["cells"].shape[2], radii=z["radii"], maps=z["map"])
    np.testing.assert_array_equal(again["cells"], store["cells"])


def test_decode_at_the_end_of_a_short_path():
    """An agent with L < T_c, in a fixture: at t = L - 1 its move leads to the goal, from t = L on it stands there and stops."""
    hits = 0
    for path in FIXTURES:
        z = np.load(path, allow_pickle=False)
        store = fixture_store(z)
        for c, n in zip(*np.nonzero(z["lengths"] < (z["makespan"] + 1)[:, None])):
            L, last = int(z["lengths"][c, n]), int(z["makespan"][c])
            for t in sorted({L - 1, L, last}):
                pos, target, _ = mr.decode(store, c, t)
                np.testing.assert_array_equal(pos[n], z["pos"][c, t, n])
                np.testing.assert_array_equal(target[n], z["target"][c, t, n])
                if t >= L:
                    assert tuple(pos[n]) == tuple(z["goal"][c, n]) and target[n].tolist() == [0, 0, 0, 0, 1]
            hits += 1
    assert hits > 0


def test_appends_give_the_store_of_their_concatenation():
    z = np.load(FIXTURES[0], allow_pickle=False)
    whole = fixture_store(z)
    cap = whole["cells"].shape[2]
    parts = []
    for c in range(len(z["makespan"])):
        Lc = int(z["lengths"][c].max())      # each append with its own Lmax
        parts.append(mr.make_store(z["paths"][c:c + 1, :, :Lc], z["lengths"][c:c + 1], z["goal"][c:c + 1], z["makespan"][c:c + 1], cap,
                                   radii=z["radii"][c:c + 1], maps=z["map"][c:c + 1]))
    both = mr.concat_stores(parts)
    for key in ("cells", "lengths", "goal", "makespan", "radii", "cum", "maps"):
        np.testing.assert_array_equal(both[key], whole[key], err_msg=key)


def test_pick_entry_is_declared_bound_and_exported():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    src = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "sim_expert.hip")).read()
    assert "sim_expert_pick.h" in build_native.HEADERS and '#include "sim_expert_pick.h"' in src
    decl = re.search(r"int magat_sim_expert_pick\(([^;]*)\);", hdr)
    assert decl and "magat_sim_expert_pick" in nat.EXPORTED_SYMBOLS
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1)).split(",")]
    res, sig = nat._SIGNATURES["magat_sim_expert_pick"]
    assert res is ctypes.c_int and len(args) == len(sig) == 24
    for a, s in zip(args, sig):      # pointers and ints stand where the header has them
        assert ("*" in a) == (s is ctypes.c_void_p) and (s is ctypes.c_void_p or s is ctypes.c_int), a
    assert re.search(r'extern "C" int magat_sim_expert_pick\(', src)
    assert hdr.index("int magat_sim_expert_stats(") < hdr.index("int magat_sim_expert_pick(")
    for name in ("ExpertMemory", "online_expert"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9 and nat.FORMS["sim_expert"] == 17 and nat.TAG_SIM_EXPERT == 27


def test_pick_refusals_in_order_and_uncounted():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    p = ctypes.c_void_p(16)
    before = lib.magat_form_count(nat.FORMS["sim_expert"])

    def call(ptrs=None, sizes=(4, 2, 8, 10, 10, 3)):
        ptrs = dict(ptrs or {})
        a = [ptrs.get(i, p) for i in range(17)]
        return lib.magat_sim_expert_pick(*a, *sizes, None)

    for i in range(17):      # every pointer but maps (6) and map_out (15) is required
        if i not in (6, 15):
            assert call({i: None}) == -5, i
    assert call({0: None}, sizes=(0, 2, 8, 10, 10, 3)) == -5            # NULL before sizes
    for k in range(6):
        sizes = [4, 2, 8, 10, 10, 3]
        sizes[k] = 0
        assert call(sizes=tuple(sizes)) == -1, k
        sizes[k] = -1
        assert call(sizes=tuple(sizes)) == -1, k
    assert call({6: None}, sizes=(4, 2, 8, 0, 10, 3)) == -1             # sizes before limits
    assert call(sizes=(4, 2, 8, 257, 10, 3)) == -2 and call(sizes=(4, 2, 8, 10, 257, 3)) == -2
    assert call(sizes=(4, 1 << 16, 8, 10, 10, 1 << 15)) == -2           # M * N = 2^31
    assert call(sizes=(4, 1, 8, 256, 256, 1 << 15)) == -2               # M * H * W = 2^31
    assert call({6: None}) == -2 and call({15: None}) == -2             # maps and map_out: both or neither
    assert lib.magat_form_count(nat.FORMS["sim_expert"]) == before      # a refused call is not counted as a launch


# ---- the kernel itself, compiled for the host (tools/host_wave) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pick_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "expert_pick_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "expert_pick_check.cpp"), "-o", exe], check=True)
    return exe


def case_text(store, indices):
    count, N, Lcap = store["cells"].shape
    maps = store["maps"]
    H, W = (maps.shape[1], maps.shape[2]) if maps is not None else (7, 9)
    flat = lambda a: " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))      # noqa: E731
    lines = ["%d %d %d %d %d %d %d" % (count, N, Lcap, H, W, len(indices), int(maps is not None)), flat(store["cells"]),
             flat(store["lengths"]), flat(store["goal"]), flat(store["makespan"]), " ".join(repr(float(r)) for r in store["radii"]),
             flat(store["cum"]), flat(maps) if maps is not None else "", flat(indices)]
    return "\n".join(lines) + "\n"


def run_check(exe, tmp_path, store, indices):
    (tmp_path / "case.txt").write_text(case_text(store, indices))
    run = subprocess.run([exe, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True)
    lines = run.stdout.split("\n")
    want = mr.pick(store, indices)
    assert int(lines[0]) == want["flag"]
    for key, line in zip(("case", "step", "pos", "target", "action", "goal"), lines[1:7]):
        got = np.array(line.split(), dtype=np.int64).reshape(want[key].shape)
        np.testing.assert_array_equal(got, want[key].astype(np.int64), err_msg=key)
    assert [float(v) for v in lines[7].split()] == want["radii"].tolist()      # (17 digits: the same float64)
    if want["map"] is not None:
        np.testing.assert_array_equal(np.array(lines[8].split(), dtype=np.int64).reshape(want["map"].shape), want["map"])
    return want


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_host_kernel_equals_the_restatement_on_the_fixture_samples(pick_check, tmp_path, path):
    z = np.load(path, allow_pickle=False)
    store = fixture_store(z)
    total = int(store["cum"][-1])
    run_check(pick_check, tmp_path, store, list(range(total)))
    rng = np.random.default_rng(3)
    run_check(pick_check, tmp_path, store, rng.integers(0, total, size=37).tolist())      # some samples twice, in any order


def test_host_kernel_on_the_one_step_store(pick_check, tmp_path):
    _, store = mr.one_step_store()
    want = run_check(pick_check, tmp_path, store, list(range(17)))
    assert want["case"].tolist() == [0, 1, 1, 1, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5]
    want = run_check(pick_check, tmp_path, store, [16, 17, 0, -1, 5, 1 << 40])
    assert want["flag"] == 1
    # M * N = 300: a full workgroup and 44 threads of a second one (a sample's agents on both sides of the edge: 256 = 2 * 128)
    run_check(pick_check, tmp_path, store, [j % 17 for j in range(150)])
    run_check(pick_check, tmp_path, dict(store, maps=None), list(range(17)))      # the shared-map form: nothing is copied
    odd = dict(store, maps=np.arange(6 * 5 * 7, dtype=np.uint8).reshape(6, 5, 7) % 2)      # H * W = 35: the byte-wise copy
    run_check(pick_check, tmp_path, odd, list(range(16, -1, -1)))


def test_host_kernel_on_a_store_of_one_agent(pick_check, tmp_path):
    paths = np.array([[[(3, 3), (3, 4), (2, 4), (2, 4)]], [[(0, 0), (0, 0), (0, 0), (0, 0)]], [[(5, 1), (6, 1), (6, 0), (5, 0)]]])
    store = mr.make_store(paths, [[3], [1], [4]], [[(2, 4)], [(0, 0)], [(5, 0)]], [4, 0, 3], 6, radii=[2.0, 3.3, 1.1 * 1.1],
                          maps=np.zeros((3, 8, 8), dtype=np.uint8) + np.arange(3, dtype=np.uint8)[:, None, None])
    want = run_check(pick_check, tmp_path, store, list(range(10)) + [9, 0])
    assert want["action"][:5, 0].tolist() == [3, 0, 4, 4, 4] and want["action"][6:10, 0].tolist() == [2, 1, 0, 4]
    run_check(pick_check, tmp_path, store, list(range(10)) * 30)      # M * N = 300 with N = 1


# ---- the Python surface refuses without touching a device ------------------------------------------------------------------------------
def test_python_surface_refuses_on_the_host():
    from magat_pathplanning_amd import ExpertMemory, online_expert
    from magat_pathplanning_amd import _native as nat
    for g in ("SemiLG_S", "SemiLG_SD"):
        with pytest.raises(ValueError, match="expert_samples"):
            ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance=g)
    with pytest.raises(ValueError):
        ExpertMemory(4, 2, 10, 10, 8, 7.0, guidance="nonsense")
    with pytest.raises(TypeError):
        ExpertMemory(4, 2, 10, 10, 8, 7.0, gso_dtype=torch.float16)
    with pytest.raises(ValueError):
        ExpertMemory(4, 2, 257, 10, 8, 7.0)
    with pytest.raises(ValueError):
        ExpertMemory(0, 2, 10, 10, 8, 7.0)
    with pytest.raises(nat.MagatNativeError):
        ExpertMemory(4, 2, 10, 10, 8, 7.0, device="cpu")
    with pytest.raises(nat.MagatNativeError):
        ExpertMemory(4, 2, 10, 10, 8, 7.0, shared_map=torch.zeros(10, 10, dtype=torch.uint8))
    z = torch.zeros(1, 2, 3, 2, dtype=torch.int32)
    blank = object.__new__(ExpertMemory)      # append looks at its arguments before it looks at the memory
    with pytest.raises(nat.MagatNativeError, match="device tensor"):
        ExpertMemory.append(blank, torch.zeros(1, 10, 10, dtype=torch.uint8), z, torch.ones(1, 2, dtype=torch.int32), z[:, :, 0],
                            torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="maxstep"):
        online_expert(types.SimpleNamespace(currentstep=2, maxstep=3), None)


# ---- the inputs of the online-expert GPU test -------------------------------------------------------------------------------------------
def test_online_expert_inputs_meet_their_condition():
    """With ONLINE's seed every case is valid, and ECBS's restatement at w = 1.1 with 256 nodes solves every case the episode of
    "stop" actions fails at - so the GPU test may assert solved.all()."""
    from magat_pathplanning_amd import mapf
    k = ONLINE
    cases = online_cases()
    assert cases["valid"].tolist() == [1] * k["C"]
    failed = [c for c in range(k["C"]) if (cases["start"][c] != cases["goal"][c]).any()]
    assert failed == [c for c in range(k["C"]) if c not in k["on_goal"]] and len(failed) == 4
    T = mapf.default_horizon(k["H"], k["W"], k["N"])
    assert T == 44
    for c in failed:
        out = er.ecbs(cases["map"][c], cases["start"][c], cases["goal"][c], T, w_milli=k["w_milli"], max_nodes=k["nodes"])
        assert out["status"] == 0 and out["solved"] == 1, c
        assert out["makespan"] + 1 <= T
