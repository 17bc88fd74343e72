"""CPU-only: the host side of the expert-schedule entries (csrc/sim_expert.hip, magat_pathplanning_amd/expert.py) - header /
loader / build list, pack_schedules, flatten_samples, the bad-move message - and the expert_* fixtures made by the real
reference (tools/make_golden_expert.py): they load and are consistent with themselves."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_paths

FIXTURES = golden_paths("expert_")
IDS = [os.path.basename(p)[7:-4] for p in FIXTURES]
MOVES = np.array([[-1, 0], [0, -1], [1, 0], [0, 1], [0, 0]])
ENTRIES = ("magat_sim_expert_schedule", "magat_sim_expert_radius", "magat_sim_expert_stats")


def test_fixture_set_is_complete():
    assert set(IDS) == {"n10_map20_ProjectG_dyn", "n10_map20_LocalG_SD_fixed", "n12_map10_dense_SemiLG_S_fixed",
                        "n30_map40_GlobalG_S_dyn_symnorm", "n8_map10_idle"}
    for p in FIXTURES:
        assert os.path.getsize(p) < 1000 * 1000, p


def test_expert_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "sim_expert.hip" in build_native.SOURCES and "sim_connect.h" in build_native.HEADERS
    for name in ENTRIES:
        assert name in nat.EXPORTED_SYMBOLS and re.search(r"int %s\(" % name, hdr), name
    # added at the END of the header, behind everything ABI 9 already had
    assert hdr.index("magat_form_reset(void)") < min(hdr.index("int %s(" % n) for n in ENTRIES)
    assert [len(nat._SIGNATURES[n][1]) for n in ENTRIES] == [13, 11, 13]
    assert int(re.search(r"#define MAGAT_TAG_SIM_EXPERT (\d+)", common).group(1)) == nat.TAG_SIM_EXPERT
    assert nat.TAGS[nat.TAG_SIM_EXPERT] == "sim_expert"
    assert int(re.search(r"#define MAGAT_FORM_SIM_EXPERT (\d+)", common).group(1)) == nat.FORMS["sim_expert"]
    for name in ("pack_schedules", "expert_schedule", "expert_radius", "expert_stats", "expert_samples", "flatten_samples"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    assert lib.magat_form_count(nat.FORMS["sim_expert"]) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(nat.TAG_SIM_EXPERT, ctypes.byref(c), ctypes.byref(ms)) == 0
    # argument checks answer before anything touches a device
    one = ctypes.c_void_p(16)
    before = lib.magat_form_count(nat.FORMS["sim_expert"])
    assert lib.magat_sim_expert_schedule(None, one, one, one, one, one, one, one, 1, 4, 8, 8, None) == -5
    assert lib.magat_sim_expert_schedule(one, one, one, one, one, one, one, one, 1, 4, 0, 8, None) == -1
    assert lib.magat_sim_expert_schedule(one, one, one, one, one, one, one, one, 1 << 16, 1 << 10, 8, 1 << 6, None) == -2
    assert lib.magat_sim_expert_radius(one, one, 7.0, one, None, one, 1, 8, 4, 64, None) == -5
    assert lib.magat_sim_expert_radius(one, one, 0.0, one, one, one, 1, 8, 4, 64, None) == -1
    assert lib.magat_sim_expert_radius(one, one, 7.0, one, one, one, 1, 8, 6000, 64, None) == -2      # 3 N ints of LDS
    assert lib.magat_sim_expert_stats(one, one, one, one, one, one, one, one, None, 1, 8, 4, None) == -5
    assert lib.magat_sim_expert_stats(one, one, one, one, one, one, one, one, one, 1, 0, 4, None) == -1
    assert lib.magat_form_count(nat.FORMS["sim_expert"]) == before      # a refused call is not counted as a launch


def test_pack_schedules_round_trip():
    from magat_pathplanning_amd import pack_schedules
    paths = [[[(0, 0), (0, 1), (1, 1)], [(3, 3)]],
             [np.array([[2, 2], [2, 3]]), np.array([[5, 5], [4, 5], [4, 5], [3, 5], [3, 4]])]]
    goals = [[(1, 1), (3, 3)], np.array([[2, 3], [3, 4]])]
    pk = pack_schedules(paths, goals, device="cpu")
    assert pk["T"] == 5 and pk["makespan"].tolist() == [2, 4] and pk["makespan"].dtype == torch.int32
    assert tuple(pk["paths"].shape) == (2, 2, 5, 2) and pk["paths"].dtype == torch.int32
    assert pk["lengths"].tolist() == [[3, 1], [2, 5]]
    assert pk["start"].tolist() == [[[0, 0], [3, 3]], [[2, 2], [5, 5]]] and pk["goal"].tolist() == [[[1, 1], [3, 3]], [[2, 3], [3, 4]]]
    for c in range(2):
        for n in range(2):
            L = int(pk["lengths"][c, n])
            got = pk["paths"][c, n].numpy()
            np.testing.assert_array_equal(got[:L], np.asarray(paths[c][n]))
            assert (got[L:] == got[L - 1]).all()              # padded with the last cell
    assert pack_schedules(paths, goals, makespan=[6, 1], device="cpu")["T"] == 7
    with pytest.raises(ValueError):
        pack_schedules(paths, goals[:1], device="cpu")
    with pytest.raises(ValueError):
        pack_schedules([[[(0, 0)]], [[(0, 0)], [(1, 1)]]], [[(0, 0)], [(0, 0), (1, 1)]], device="cpu")
    with pytest.raises(ValueError):
        pack_schedules([[[]]], [[(0, 0)]], device="cpu")


def test_flatten_samples_on_hand_made_tensors():
    from magat_pathplanning_amd import flatten_samples
    C, T, N = 3, 4, 2
    valid = torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0]], dtype=torch.uint8)
    tag = (torch.arange(C)[:, None] * 10 + torch.arange(T)[None]).float()                  # value = 10 c + t
    s = dict(valid=valid, inputTensor=tag.view(C, T, 1, 1, 1, 1).expand(C, T, N, 3, 5, 5).clone(),
             target=tag.view(C, T, 1, 1).expand(C, T, N, 5).clone(), GSO=tag.view(C, T, 1, 1).expand(C, T, N, N).clone(),
             pos=tag.view(C, T, 1, 1).expand(C, T, N, 2).int().clone())
    f = flatten_samples(s)
    want = [0., 1., 10., 11., 12., 13., 20.]
    assert tuple(f["inputTensor"].shape) == (7, N, 3, 5, 5) and tuple(f["target"].shape) == (7, N, 5)
    assert tuple(f["GSO"].shape) == (7, N, N) and tuple(f["pos"].shape) == (7, N, 2)
    for key in ("inputTensor", "target", "GSO", "pos"):
        assert f[key].reshape(7, -1)[:, 0].float().tolist() == want, key
    assert f["case"].tolist() == [0, 0, 1, 1, 1, 1, 2] and f["step"].tolist() == [0, 1, 0, 1, 2, 3, 0]


def test_bad_move_message_and_cpu_tensors_raise():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import expert
    assert expert.bad_move_message(torch.tensor([-1, -1], dtype=torch.int32), 10) is None
    msg = expert.bad_move_message(torch.tensor([-1, 37, 4], dtype=torch.int32), 10)
    assert "case 1" in msg and "step 3" in msg and "agent 7" in msg and "2 case" in msg
    z = torch.zeros(1, 2, 3, 2, dtype=torch.int32)
    with pytest.raises(nat.MagatNativeError):
        expert.expert_schedule(z, torch.ones(1, 2, dtype=torch.int32), z[:, :, 0], torch.ones(1, dtype=torch.int32), T=2)
    with pytest.raises(nat.MagatNativeError):
        expert.expert_radius(z, torch.ones(1, 2, dtype=torch.uint8), 7.0)
    with pytest.raises(nat.MagatNativeError):
        expert.expert_stats(torch.zeros(1, 2, 3, 5), z[:, 0], z[:, 0], torch.ones(1, 2, dtype=torch.uint8))
    with pytest.raises(nat.MagatNativeError):
        expert.expert_samples(torch.zeros(4, 4, dtype=torch.uint8), z, torch.ones(1, 2, dtype=torch.int32), z[:, :, 0],
                              torch.ones(1, dtype=torch.int32), 7.0)
    with pytest.raises(ValueError):
        expert.expert_samples(torch.zeros(4, 4, dtype=torch.uint8), z, None, None, None, 7.0, guidance="nonsense")


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_fixture_is_self_consistent(path):
    z = np.load(path, allow_pickle=False)
    C, T, N = z["pos"].shape[:3]
    assert z["x"].dtype == np.uint8 and set(np.unique(z["x"])) <= {0, 1} and z["x"].shape == (C, T, N, 3, 11, 11)
    assert z["GSO"].dtype == np.float64 and z["GSO"].shape == (C, T, N, N) and z["radii"].dtype == np.float64
    assert T == int(z["makespan"].max()) + 1 and z["expert_pos"].shape == (C, T + 1, N, 2)
    assert str(z["guidance"].reshape(-1)[0]) in ("Project_G", "LocalG_SD", "SemiLG_S", "GlobalG_S")
    for c in range(C):
        Tc = int(z["makespan"][c]) + 1
        assert z["valid"][c].tolist() == [1] * Tc + [0] * (T - Tc)
        assert (z["target"][c, :Tc].sum(-1) == 1).all() and set(np.unique(z["target"])) <= {0, 1}      # one-hot
        for key in ("pos", "target", "x", "GSO"):
            assert not z[key][c, Tc:].any(), key                                                      # padded rows are zero
        # pos[t + 1] - pos[t] is the move that target[t] encodes; behind the last step it leads to the goal
        nxt = np.concatenate([z["pos"][c, 1:Tc], z["goal"][c][None]]) if Tc > 1 else z["goal"][c][None]
        cut = z["lengths"][c].max() - 1 > z["makespan"][c]                    # a schedule cut short does not end at the goals
        steps = Tc - 1 if cut else Tc
        np.testing.assert_array_equal((nxt - z["pos"][c, :Tc])[:steps], MOVES[z["target"][c, :Tc].argmax(-1)][:steps])
        np.testing.assert_array_equal(z["pos"][c, 0], z["start"][c])
        # the expert's walk re-derived from the targets is the schedule itself
        np.testing.assert_array_equal(z["expert_pos"][c, :Tc], z["pos"][c, :Tc])
        # the stored radius is R * 1.1 * ... * 1.1, grow_steps multiplications in sequence
        r = float(z["commR"].reshape(-1)[0])
        for _ in range(int(z["grow_steps"][c])):
            r = r * 1.1
        assert r == float(z["radii"][c])
        assert int(z["dynamic_commR"].reshape(-1)[0]) or int(z["grow_steps"][c]) == 0
        fm, es = z["first_move"][c], z["end_step"][c]
        assert int(z["makespanTarget"][c]) == es.max() - fm.min() + 1 and int(z["flowtimeTarget"][c]) == (es - fm + 1).sum()
    if int(z["dynamic_commR"].reshape(-1)[0]):
        assert (z["grow_steps"] >= 1).any()
