"""GPU: the A*-guided state encodings (csrc/sim_guidance.hip through batched_fov_states / BatchedEpisode) EQUAL the reference's
tensors - on every guid_* fixture (made by the real AgentState, tools/make_golden_guidance.py) and, on scenarios the fixtures
do not hold, the numpy restatement that tests/test_host_guidance.py pins against those fixtures.  No tolerance: equality."""
import os

import numpy as np
import pytest
import torch

import guidance_restatement as gr
from conftest import golden_paths

pytestmark = pytest.mark.gpu

FIXTURES = golden_paths("guid_")
IDS = [os.path.basename(p)[5:-4] for p in FIXTURES]


def fixture_guidance(path):
    return "_".join(os.path.basename(path).split("_")[1:3])


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def scenario(rng, N, H, W, density):
    m = (rng.random((H, W)) < density).astype(np.uint8)
    free = np.argwhere(m == 0)
    pos = free[rng.permutation(len(free))[:N]].astype(np.int32)
    goal = free[rng.permutation(len(free))[:N]].astype(np.int32)
    return m, pos, goal


def expected(maps, pos, goal, guidance, views=None):
    """Restatement over a batch; maps (H,W) or (B,H,W); views: list of per-instance memories (SemiLG), updated in place."""
    out = []
    for b in range(pos.shape[0]):
        m = maps if maps.ndim == 2 else maps[b]
        out.append(gr.guided_states(m, pos[b], goal[b], guidance, agent_view=None if views is None else views[b]))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_guided"]))


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_guided_states_equal_reference_fixture(gpu_device, path):
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    z = np.load(path, allow_pickle=False)
    g = fixture_guidance(path)
    m, goal = dev(z["map"], gpu_device), dev(z["goal"], gpu_device)
    B, H, W = z["map"].shape
    before = form_count()
    if g.startswith("SemiLG"):
        T, N = z["pos"].shape[1:3]
        view = new_agent_view(B, N, H, W, 9, gpu_device)
        for t in range(T):
            x = batched_fov_states(m, dev(z["pos"][:, t], gpu_device), goal, 9, guidance=g, agent_view=view)
            assert x.dtype == torch.float32
            assert torch.equal(x.cpu(), torch.from_numpy(z["x"][:, t].astype(np.float32))), "%s step %d" % (g, t)
        assert form_count() == before + T
    else:
        x = batched_fov_states(m, dev(z["pos"], gpu_device), goal, 9, guidance=g)
        assert x.dtype == torch.float32 and tuple(x.shape) == z["x"].shape
        assert torch.equal(x.cpu(), torch.from_numpy(z["x"].astype(np.float32))), g
        assert form_count() == before + 1


def test_project_g_through_the_new_argument_is_the_old_call(gpu_device):
    from magat_pathplanning_amd import batched_fov_states
    rng = np.random.default_rng(11)
    m, pos, goal = scenario(rng, 100, 50, 50, 0.1)
    m, pos, goal = dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device)
    before = form_count()
    a = batched_fov_states(m, pos, goal, 9)
    b = batched_fov_states(m, pos, goal, 9, guidance="Project_G")
    c = batched_fov_states(m, pos, goal, FOV=9, guidance="Project_G", agent_view=None)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert form_count() == before                    # the existing kernel, not the new one


@pytest.mark.parametrize("guidance", gr.GUIDANCE)
def test_single_agent_and_batched_maps(gpu_device, guidance):
    """N = 1, and a batch with one map PER instance (B,H,W), non-square."""
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    rng = np.random.default_rng(101)
    for N, B, H, W in ((1, 5, 17, 23), (7, 4, 23, 17)):
        scen = [scenario(rng, N, H, W, 0.15) for _ in range(B)]
        maps, pos, goal = (np.stack([s[i] for s in scen]) for i in range(3))
        semi = guidance.startswith("SemiLG")
        views = [gr.new_agent_view(N, H, W) for _ in range(B)] if semi else None
        dview = new_agent_view(B, N, H, W, 9, gpu_device) if semi else None
        for step in range(3 if semi else 1):
            p = np.clip(pos + step, 0, [H - 1, W - 1]).astype(np.int32)      # (walks over obstacles too: any cell is a legal input)
            x = batched_fov_states(dev(maps, gpu_device), dev(p, gpu_device), dev(goal, gpu_device), 9, guidance=guidance,
                                   agent_view=dview)
            assert torch.equal(x.cpu(), expected(maps, p, goal, guidance, views)), (guidance, N, step)
        if semi:
            assert torch.equal(dview.cpu(), torch.from_numpy(np.stack(views)))      # the memory itself, after three steps


@pytest.mark.parametrize("guidance", ["LocalG_S", "LocalG_SD"])
def test_thousand_agents_local(gpu_device, guidance):
    from magat_pathplanning_amd import batched_fov_states
    rng = np.random.default_rng(1000)
    m, pos, goal = scenario(rng, 1000, 50, 50, 0.1)
    x = batched_fov_states(dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device), 9, guidance=guidance)
    assert torch.equal(x.cpu(), expected(m, pos[None], goal[None], guidance))


@pytest.mark.parametrize("guidance", ["GlobalG_S", "GlobalG_SD", "SemiLG_SD"])
def test_largest_canvas_and_a_wall(gpu_device, guidance):
    """54 x 54 map = the 64 x 64 canvas limit; and a map cut in two by a wall (goals behind it: the whole reachable half is
    searched and the path is the start cell alone)."""
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    rng = np.random.default_rng(54)
    m, pos, goal = scenario(rng, 60, 54, 54, 0.12)
    pos[0], goal[0] = (0, 0), (53, 53)
    pos[1], goal[1] = (53, 0), (0, 53)
    m[0, 0] = m[53, 53] = m[53, 0] = m[0, 53] = 0
    wall = (rng.random((54, 54)) < 0.05).astype(np.uint8)
    wall[:, 27] = 1
    free = np.argwhere(wall == 0)
    wpos = free[rng.permutation(len(free))[:60]].astype(np.int32)
    wgoal = free[rng.permutation(len(free))[:60]].astype(np.int32)
    assert ((wpos[:, 1] < 27) != (wgoal[:, 1] < 27)).sum() > 10
    maps, pos, goal = np.stack([m, wall]), np.stack([pos, wpos]), np.stack([goal, wgoal])
    semi = guidance.startswith("SemiLG")
    views = [gr.new_agent_view(60, 54, 54) for _ in range(2)] if semi else None
    dview = new_agent_view(2, 60, 54, 54, 9, gpu_device) if semi else None
    x = batched_fov_states(dev(maps, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device), 9, guidance=guidance,
                           agent_view=dview)
    assert torch.equal(x.cpu(), expected(maps, pos, goal, guidance, views))


def test_map_over_the_limit_is_refused_before_launch(gpu_device):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    rng = np.random.default_rng(55)
    m, pos, goal = scenario(rng, 8, 55, 54, 0.1)
    args = (dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device), 9)
    before = form_count()
    for g in ("GlobalG_S", "GlobalG_SD", "SemiLG_S", "SemiLG_SD"):
        view = new_agent_view(1, 8, 55, 54, 9, gpu_device) if g.startswith("SemiLG") else None
        with pytest.raises(nat.MagatNativeError, match="unsupported"):
            batched_fov_states(*args, guidance=g, agent_view=view)
        if view is not None:
            assert int(view.sum()) == 0
    assert form_count() == before                    # nothing was launched
    with pytest.raises(ValueError):
        batched_fov_states(*args, guidance="SemiLG_S")                   # no agent_view
    # LocalG searches the window only: any map size
    x = batched_fov_states(*args, guidance="LocalG_SD")
    assert torch.equal(x.cpu(), expected(m, pos[None], goal[None], "LocalG_SD"))
    assert form_count() == before + 1


def test_semilg_through_batched_episode(gpu_device):
    """The episode owns the memory: its states() over the fixture's 8 steps equal the reference's, and a second episode
    started later does not see what the first one has seen."""
    from magat_pathplanning_amd import BatchedEpisode
    path = [p for p in FIXTURES if "SemiLG_SD_n10_map20" in p][0]
    z = np.load(path, allow_pickle=False)
    m, goal = dev(z["map"], gpu_device), dev(z["goal"], gpu_device)
    T = z["pos"].shape[1]
    ep = BatchedEpisode(m, dev(z["pos"][:, 0], gpu_device), goal, 50, comm_radius=7.0, guidance="SemiLG_SD")
    assert ep.agent_view is not None and int(ep.agent_view.sum()) == 0
    other = None
    for t in range(T):
        ep.pos.copy_(dev(z["pos"][:, t], gpu_device))
        assert torch.equal(ep.states().cpu(), torch.from_numpy(z["x"][:, t].astype(np.float32))), t
        if t == T - 2:
            other = BatchedEpisode(m, dev(z["pos"][:, T - 1], gpu_device), goal, 50, comm_radius=7.0, guidance="SemiLG_SD")
    assert other.agent_view.data_ptr() != ep.agent_view.data_ptr()
    fresh = expected(z["map"], z["pos"][:, T - 1], z["goal"], "SemiLG_SD",
                     [gr.new_agent_view(z["pos"].shape[2], 20, 20) for _ in range(z["map"].shape[0])])
    assert torch.equal(other.states().cpu(), fresh)
    assert not torch.equal(other.agent_view, ep.agent_view)
    # the other guidance strings keep no memory; the default episode is 'Project_G'
    assert BatchedEpisode(m, dev(z["pos"][:, 0], gpu_device), goal, 50, comm_radius=7.0, guidance="GlobalG_S").agent_view is None
    base = BatchedEpisode(m, dev(z["pos"][:, 0], gpu_device), goal, 50, comm_radius=7.0)
    assert base.guidance == "Project_G" and base.agent_view is None


def test_guided_launch_is_counted_by_tag_and_form(gpu_device, tag_counts):
    from magat_pathplanning_amd import batched_fov_states
    rng = np.random.default_rng(3)
    m, pos, goal = scenario(rng, 20, 30, 30, 0.1)
    before = form_count()
    with tag_counts() as tc:
        batched_fov_states(dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device), 9, guidance="GlobalG_SD")
        batched_fov_states(dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device), 9, guidance="LocalG_S")
    assert tc["sim_guided"] == 2 and form_count() == before + 2
