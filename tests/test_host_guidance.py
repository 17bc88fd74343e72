"""CPU-only: the numpy restatement of the A*-guided state encodings (tests/guidance_restatement.py) equals every guid_* fixture
made by the real reference (tools/make_golden_guidance.py) - after that the GPU tests may use it as the expected value on
scenarios the fixtures do not hold.  Plus the host side of the new entry: argument checks, header / loader / build list."""
import os
import re

import numpy as np
import pytest
import torch

import guidance_restatement as gr
from conftest import ROOT, golden_paths

FIXTURES = golden_paths("guid_")
IDS = [os.path.basename(p)[5:-4] for p in FIXTURES]


def fixture_guidance(path):
    return "_".join(os.path.basename(path).split("_")[1:3])


def test_fixture_set_is_complete():
    got = {os.path.basename(p)[5:-4] for p in FIXTURES}
    want = {"%s_%s" % (g, c) for g in gr.GUIDANCE for c in ("n10_map20", "n100_map50", "n12_map10_dense")}
    assert got == want, got ^ want


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_restatement_equals_reference_fixture(path):
    z = np.load(path, allow_pickle=False)
    g = fixture_guidance(path)
    assert z["x"].dtype == np.uint8 and z["pos"].dtype == np.int32 and z["goal"].dtype == np.int32 and z["map"].dtype == np.uint8
    assert set(np.unique(z["x"])) <= {0, 1}
    for b in range(z["map"].shape[0]):
        if g.startswith("SemiLG"):
            T, N = z["pos"].shape[1:3]
            view = gr.new_agent_view(N, z["map"].shape[1], z["map"].shape[2])
            for t in range(T):
                x = gr.guided_states(z["map"][b], z["pos"][b, t], z["goal"][b], g, agent_view=view)
                np.testing.assert_array_equal(x, z["x"][b, t], err_msg="%s instance %d step %d" % (g, b, t))
        else:
            x = gr.guided_states(z["map"][b], z["pos"][b], z["goal"][b], g)
            np.testing.assert_array_equal(x, z["x"][b], err_msg="%s instance %d" % (g, b))


def test_semilg_fixture_needs_the_memory():
    """Fed an EMPTY memory at the last step, the restatement does not give the fixture: the sequence test above does test the
    memory."""
    path = [p for p in FIXTURES if "SemiLG_SD_n100_map50" in p][0]
    z = np.load(path, allow_pickle=False)
    T, N = z["pos"].shape[1:3]
    x = gr.guided_states(z["map"][0], z["pos"][0, T - 1], z["goal"][0], "SemiLG_SD",
                         agent_view=gr.new_agent_view(N, z["map"].shape[1], z["map"].shape[2]))
    assert (x != z["x"][0, T - 1]).any()


def test_a_star_tie_breaking_and_no_path():
    grid = np.zeros((5, 5), dtype=np.int64)
    # equal f everywhere inside the rectangle: smaller g first, then smaller row, then smaller column; first pusher stays parent
    path, pops = gr.a_star(grid, (0, 0), (2, 2))
    assert path == [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)] and pops == 9
    grid[1, :] = 1
    assert gr.a_star(grid, (0, 0), (4, 4)) == ([(0, 0)], 5)                 # walled off: the start alone
    grid[1, 2] = 2                                                          # any non-zero value blocks
    assert gr.a_star(grid, (0, 0), (4, 4))[0] == [(0, 0)]
    assert gr.a_star(grid, (3, 3), (3, 3)) == ([(3, 3)], 1)
    grid[0, 0] = 1                                                          # the start cell is never tested
    assert gr.a_star(grid, (0, 0), (0, 3))[0] == [(0, 0), (0, 1), (0, 2), (0, 3)]


def test_unknown_guidance_raises_value_error():
    from magat_pathplanning_amd import BatchedEpisode, batched_fov_states
    m, p = torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(1, 2, 2, dtype=torch.int32)
    with pytest.raises(ValueError):
        batched_fov_states(m, p, p, guidance="nonsense")
    with pytest.raises(ValueError):
        BatchedEpisode(m, p, p, 10, comm_radius=7.0, guidance="GlobalG")
    with pytest.raises(ValueError):
        gr.guided_states(m.numpy(), p[0].numpy(), p[0].numpy(), "nonsense")


def test_guided_entry_is_declared_bound_and_built():
    import ctypes
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native, simulator
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "magat_sim_guided_states" in nat.EXPORTED_SYMBOLS and "sim_guidance.hip" in build_native.SOURCES
    assert re.search(r"int magat_sim_guided_states\(", hdr)
    assert len(nat._SIGNATURES["magat_sim_guided_states"][1]) == 14
    for name, val in (("LOCAL", nat.GUIDE_LOCAL), ("GLOBAL", nat.GUIDE_GLOBAL), ("SEMI", nat.GUIDE_SEMI)):
        assert int(re.search(r"#define MAGAT_GUIDE_%s (\d+)" % name, hdr).group(1)) == val
    assert int(re.search(r"#define MAGAT_TAG_SIM_GUIDED (\d+)", common).group(1)) == nat.TAG_SIM_GUIDED
    assert nat.TAGS[nat.TAG_SIM_GUIDED] == "sim_guided"
    assert int(re.search(r"#define MAGAT_FORM_SIM_GUIDED (\d+)", common).group(1)) == nat.FORMS["sim_guided"]
    assert set(simulator.GUIDANCE_MODES) == set(gr.GUIDANCE) | {"Project_G"}
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9
    assert lib.magat_form_count(nat.FORMS["sim_guided"]) >= 0
    c, ms = ctypes.c_longlong(0), ctypes.c_double(0)
    assert lib.magat_profile_read(nat.TAG_SIM_GUIDED, ctypes.byref(c), ctypes.byref(ms)) == 0
    # argument checks answer before anything touches a device: NULL pointers, shapes, the canvas limit
    one = ctypes.c_void_p(16)
    call = lib.magat_sim_guided_states
    assert call(None, 0, 20, 20, one, one, one, 9, 1, 4, nat.GUIDE_GLOBAL, 0, None, None) == -5
    assert call(one, 0, 20, 20, one, one, one, 8, 1, 4, nat.GUIDE_GLOBAL, 0, None, None) == -1      # even FOV
    assert call(one, 0, 20, 20, one, one, one, 9, 1, 4, 7, 0, None, None) == -2                     # unknown mode
    assert call(one, 0, 55, 20, one, one, one, 9, 1, 4, nat.GUIDE_GLOBAL, 0, None, None) == -2      # 55 + 10 > 64
    assert call(one, 0, 20, 55, one, one, one, 9, 1, 4, nat.GUIDE_SEMI, 0, one, None) == -2
    assert call(one, 0, 20, 20, one, one, one, 9, 1, 4, nat.GUIDE_SEMI, 0, None, None) == -5        # SemiLG without its memory
    assert call(one, 0, 20, 20, one, one, one, 31, 1, 4, nat.GUIDE_LOCAL, 0, None, None) == -2      # FOV + 2 > 32
