"""GPU: the closed loop on maps up to 256 x 256 - the wide A*-guided state encodings (csrc/sim_guidance_wide.hip) EQUAL the
reference's tensors on every guidw_* fixture and the restatement's on the scenes of tests/test_host_wide_loop.py; the wide move
step (sim_move_kernel<WIDE>) equals oracle/sim_oracle.py; and generator -> solver -> guided episode runs at 200 x 200.  Integer
equality everywhere: no tolerance."""
import os

import numpy as np
import pytest
import torch

import guidance_restatement as gr
import test_host_wide_loop as hw
from oracle import sim_oracle as so

pytestmark = pytest.mark.gpu

IDS = [os.path.basename(p)[6:-4] for p in hw.FIXTURES]
FOV = hw.FOV


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def form_count():
    from magat_pathplanning_amd import _native as nat
    return int(nat.lib().magat_form_count(nat.FORMS["sim_guided"]))


def guided_wide_direct(m, pos, goal, mode, dyn, view=None, ws_bytes=None, null_ws=False):
    """magat_sim_guided_states_wide itself, whatever the shape.  Returns (return code, x)."""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    B, N, _ = pos.shape
    H, W = m.shape[-2:]
    x = torch.full((B, N, 3, FOV + 2, FOV + 2), -7.0, dtype=torch.float32, device=pos.device)
    need = int(lib.magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=pos.device)
    rc = lib.magat_sim_guided_states_wide(nat.ptr(m), 1 if m.dim() == 3 else 0, H, W, nat.ptr(pos), nat.ptr(goal), nat.ptr(x), FOV, B,
                                          N, mode, dyn, nat.ptr(view), None if null_ws else nat.ptr(ws),
                                          need if ws_bytes is None else ws_bytes, nat.current_stream(pos.device))
    return rc, x


# ---- guidance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", hw.FIXTURES, ids=IDS)
def test_wide_guided_states_equal_reference_fixture(gpu_device, path):
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    z = np.load(path, allow_pickle=False)
    g = hw.fixture_guidance(path)
    m, goal = dev(z["map"], gpu_device), dev(z["goal"], gpu_device)
    B, H, W = z["map"].shape
    before = form_count()
    if g.startswith("SemiLG"):
        T, N = z["pos"].shape[1:3]
        view = new_agent_view(B, N, H, W, FOV, gpu_device)
        host_view = [gr.new_agent_view(N, H, W, FOV) for _ in range(B)]
        for t in range(T):
            x = batched_fov_states(m, dev(z["pos"][:, t], gpu_device), goal, FOV, g, view, wide=True)
            assert torch.equal(x.cpu(), torch.from_numpy(z["x"][:, t].astype(np.float32))), (g, t)
            for b in range(B):
                gr.guided_states(z["map"][b], z["pos"][b, t], z["goal"][b], g, FOV, host_view[b])
        assert form_count() == before + T
        assert np.array_equal(view.cpu().numpy(), np.stack(host_view))
    else:
        x = batched_fov_states(m, dev(z["pos"], gpu_device), goal, FOV, g, wide=True)
        assert torch.equal(x.cpu(), torch.from_numpy(z["x"].astype(np.float32))), g
        assert form_count() == before + 1


@pytest.mark.parametrize("name,guidance", [(n, g) for n in hw.SCENES for g in hw.SCENE_GUIDANCE[n]])
def test_wide_guided_states_equal_restatement(gpu_device, name, guidance):
    from magat_pathplanning_amd import batched_fov_states, new_agent_view
    m, pos, goal = hw.scene(name)
    want, want_view, _ = hw.expected(name, guidance)
    view = None
    if guidance.startswith("SemiLG"):
        view = new_agent_view(1, len(pos), m.shape[0], m.shape[1], FOV, gpu_device)
    x = batched_fov_states(dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device), FOV, guidance, view, wide=True)
    got = x[0].cpu().numpy()
    bad = np.nonzero((got != want.astype(np.float32)).any(axis=(1, 2, 3)))[0]
    assert bad.size == 0, "agents %s differ" % bad.tolist()
    if view is not None:
        assert np.array_equal(view[0].cpu().numpy(), want_view)


@pytest.mark.parametrize("size", [20, 54])
def test_wide_keyword_keeps_the_narrow_route_and_the_wide_kernel_agrees(gpu_device, size):
    from magat_pathplanning_amd import _native as nat, batched_fov_states, new_agent_view
    m, pos, goal = hw.random_scene(size, size, size, 12)
    md, pd, gd = dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device)
    for g in ("GlobalG_S", "GlobalG_SD", "SemiLG_SD", "LocalG_SD", "Project_G"):
        va = vb = None
        if g.startswith("SemiLG"):
            va, vb = (new_agent_view(1, len(pos), size, size, FOV, gpu_device) for _ in range(2))
        a = batched_fov_states(md, pd, gd, FOV, g, va)
        b = batched_fov_states(md, pd, gd, FOV, g, vb, wide=True)
        assert torch.equal(a, b), g
        if va is not None:
            assert torch.equal(va, vb)
    if size == 20:      # the wide kernel itself on a shape the narrow one takes
        for g, (mode, dyn) in (("GlobalG_S", (nat.GUIDE_GLOBAL, 0)), ("GlobalG_SD", (nat.GUIDE_GLOBAL, 1)), ("SemiLG_SD", (nat.GUIDE_SEMI, 1))):
            va = vb = None
            if mode == nat.GUIDE_SEMI:
                va, vb = (new_agent_view(1, len(pos), size, size, FOV, gpu_device) for _ in range(2))
            a = batched_fov_states(md, pd, gd, FOV, g, va)
            rc, b = guided_wide_direct(md, pd, gd, mode, dyn, vb)
            assert rc == 0 and torch.equal(a, b), g
            if va is not None:
                assert torch.equal(va, vb)


def test_more_agents_than_workgroups(gpu_device):
    """4 x 300 agents on 65 x 65: 1200 > the 1024 workgroups of a launch, so workgroups walk two agents; the same instances in
    two calls of 2 x 300 (one agent a workgroup) give the same tensors."""
    from magat_pathplanning_amd import batched_fov_states
    from magat_pathplanning_amd.simulator import guided_wide_geometry
    B, N, S = 4, 300, 65
    rng = np.random.default_rng(65)
    maps = (rng.random((B, S, S)) < 0.1).astype(np.uint8)
    pos, goal = np.zeros((B, N, 2), np.int32), np.zeros((B, N, 2), np.int32)
    for b in range(B):
        free = np.argwhere(maps[b] == 0)
        idx = rng.permutation(len(free))
        pos[b], goal[b] = free[idx[:N]], free[idx[N:2 * N]]
    groups, walk = guided_wide_geometry(B, N, S, S, FOV)
    assert groups == hw.GUIDE_CAP and walk == 2
    assert guided_wide_geometry(2, N, S, S, FOV) == (600, 1)
    md, pd, gd = dev(maps, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device)
    x = batched_fov_states(md, pd, gd, FOV, "GlobalG_SD", wide=True)
    halves = [batched_fov_states(md[i:i + 2].contiguous(), pd[i:i + 2].contiguous(), gd[i:i + 2].contiguous(), FOV, "GlobalG_SD",
                                 wide=True) for i in (0, 2)]
    assert torch.equal(x, torch.cat(halves))
    # and the last instance against the restatement: its agents 900 .. 1023 are a workgroup's first, 1024 .. 1199 its second
    want = gr.guided_states(maps[3], pos[3], goal[3], "GlobalG_SD", FOV)
    assert np.array_equal(x[3].cpu().numpy(), want.astype(np.float32))


def test_wide_guidance_refusals_and_graph_capture(gpu_device):
    from magat_pathplanning_amd import _native as nat, batched_fov_states
    m, pos, goal = hw.scene("first_refused_55x54")
    md, pd, gd = dev(m, gpu_device), dev(pos[None], gpu_device), dev(goal[None], gpu_device)
    before = form_count()
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # without the keyword: refused as before
        batched_fov_states(md, pd, gd, FOV, "GlobalG_SD")
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        batched_fov_states(torch.zeros(257, 20, dtype=torch.uint8, device=gpu_device), pd, gd, FOV, "GlobalG_SD", wide=True)
    need = int(nat.lib().magat_sim_guided_states_wide_workspace_bytes(1, len(pos), 55, 54, FOV))
    assert need == hw.documented_guided_workspace_bytes(1, len(pos), 55, 54)
    for kwargs, code in ((dict(ws_bytes=need - 1), -2), (dict(null_ws=True), -5)):
        rc, x = guided_wide_direct(md, pd, gd, nat.GUIDE_GLOBAL, 1, **kwargs)
        torch.cuda.synchronize()
        assert rc == code and bool((x == -7.0).all())
    assert form_count() == before
    eager = batched_fov_states(md, pd, gd, FOV, "GlobalG_SD", wide=True)      # (the workspace is cached from here on)
    ps = pd.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = batched_fov_states(md, ps, gd, FOV, "GlobalG_SD", wide=True)
    ps.copy_(gd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, batched_fov_states(md, gd, gd, FOV, "GlobalG_SD", wide=True))
    ps.copy_(pd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert np.array_equal(eager[0].cpu().numpy(), hw.expected("first_refused_55x54", "GlobalG_SD")[0].astype(np.float32))


# ---- move -------------------------------------------------------------------------------------------------------------------------
def move_wide_direct(m, pos, actions, goal, ws_bytes=None, null_ws=False):
    """magat_sim_move_wide itself, whatever the shape; pos is advanced in place.  Returns (return code, dict)."""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    B, N, _ = pos.shape
    H, W = m.shape[-2:]
    d = pos.device
    out = dict(actions=torch.full((B, N), -7, dtype=torch.int32, device=d), moves=torch.empty(B, N, 2, dtype=torch.int8, device=d),
               reached=torch.empty(B, N, dtype=torch.uint8, device=d), flags=torch.empty(B, dtype=torch.int32, device=d))
    need = int(lib.magat_sim_move_wide_workspace_bytes(B, H, W, N))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=d)
    rc = lib.magat_sim_move_wide(None, nat.ptr(actions), nat.ptr(m), 1 if m.dim() == 3 else 0, H, W, nat.ptr(pos), nat.ptr(goal),
                                 nat.ptr(out["actions"]), nat.ptr(out["moves"]), nat.ptr(out["reached"]), nat.ptr(out["flags"]), B, N,
                                 None if null_ws else nat.ptr(ws), need if ws_bytes is None else ws_bytes, nat.current_stream(d))
    return rc, out


def oracle_states(m, pos, goal, maxstep):
    return [so.EpisodeState(m if m.ndim == 2 else m[b], pos[b], goal[b], maxstep) for b in range(len(pos))]


def oracle_step(states, t, keys=None, logits=None, policy=0, uniforms=None):
    """episode_step on every instance; returns moves (B,N,2) and flag bits (B,) of the step (zeros where the step is skipped)."""
    moves, bits = [], []
    for b, st in enumerate(states):
        lg = np.eye(5, dtype=np.float32)[keys[b]] if logits is None else logits[b]
        before = st.pos.copy()
        live = int(np.count_nonzero(st.reach_goal)) != len(st.pos) and t < st.maxstep
        k = so.sample_actions(lg, policy, None if uniforms is None else uniforms[b])
        _, fl = so.shield_moves(st.map, before, so.MOVES[k])
        so.episode_step(st, lg, t, policy, None if uniforms is None else uniforms[b])
        moves.append(st.pos - before)
        bits.append(hw.oracle_flag_bits(fl) if live else 0)
    return np.stack(moves), np.array(bits)


def compare_episode(ep, states, what):
    for key, want in (("pos", [s.pos for s in states]), ("reach_goal", [s.reach_goal for s in states]),
                      ("first_move", [s.first_move for s in states]), ("end_step", [s.end_step for s in states])):
        assert np.array_equal(getattr(ep, key).cpu().numpy().astype(np.int64), np.stack(want).astype(np.int64)), (what, key)


def run_move_scene(name, gpu_device, wide, direct=False):
    """30 steps of seeded random keys through BatchedEpisode.step and batched_move (or magat_sim_move_wide itself), then 10 steps
    of logits under each policy, all against the oracle.  Returns the flag bits seen and everything compared, for equality
    between routes."""
    from magat_pathplanning_amd import BatchedEpisode
    from magat_pathplanning_amd.simulator import batched_move
    m, pos, goal = hw.move_inputs(name) if isinstance(name, str) else name
    B, N, _ = pos.shape
    H, W = m.shape[-2:]
    md, gd = dev(m, gpu_device), dev(goal, gpu_device)
    rng = np.random.default_rng(7)
    record, seen = [], 0
    T = 30
    ep = BatchedEpisode(md, dev(pos, gpu_device), gd, maxstep=T, comm_radius=7.0, wide=wide)
    states = oracle_states(m, pos, goal, T)
    for t in range(T + 1):
        keys = rng.integers(0, 5, (B, N))
        if t % 3 == 0:
            keys[:, :4] = hw.corner_keys(H, W)
        kd = dev(keys.astype(np.int32), gpu_device)
        loose = ep.pos.clone()                                   # the same step through the call without bookkeeping
        if direct:
            rc, mv = move_wide_direct(md, loose, kd, gd)
            assert rc == 0
        else:
            mv = batched_move(md, loose, actions=kd, goal=gd, wide=wide)
        ep.step(actions=kd)
        want_moves, want_bits = oracle_step(states, t, keys=keys)
        compare_episode(ep, states, (name, t))
        live = t < T and not bool(ep.done.all())
        if live:
            assert np.array_equal(ep.actions.cpu().numpy(), keys) and np.array_equal(ep.moves.cpu().numpy(), want_moves), t
            assert np.array_equal(ep.flags.cpu().numpy(), want_bits), (t, ep.flags.tolist(), want_bits)
            assert torch.equal(loose, ep.pos) and torch.equal(mv["moves"], ep.moves) and torch.equal(mv["flags"], ep.flags), t
            assert torch.equal(mv["actions"], kd)
            assert np.array_equal(mv["reached"].cpu().numpy().astype(bool), (ep.pos == gd).all(-1).cpu().numpy())
            seen |= int(np.bitwise_or.reduce(want_bits))
        record.append((ep.pos.cpu().numpy().copy(), ep.flags.cpu().numpy().copy(), ep.moves.cpu().numpy().copy()))
    assert [int(v) for v in ep.makespan.tolist()] == [s.makespan for s in states]
    assert [int(v) for v in ep.flowtime.tolist()] == [s.flowtime for s in states]
    for policy, select in enumerate(("soft_max", "sum_multinorm", "exp_multinorm")):
        ep = BatchedEpisode(md, dev(pos, gpu_device), gd, maxstep=10, comm_radius=7.0, action_select=select, wide=wide)
        states = oracle_states(m, pos, goal, 10)
        for t in range(11):
            logits = rng.random((B, N, 5)).astype(np.float32) + 0.05
            uni = rng.random((B, N))
            ep.step(logits=dev(logits, gpu_device), uniforms=dev(uni, gpu_device) if policy else None)
            want_moves, want_bits = oracle_step(states, t, logits=logits, policy=policy, uniforms=uni)
            compare_episode(ep, states, (name, select, t))
            if t < 10:
                assert np.array_equal(ep.moves.cpu().numpy(), want_moves) and np.array_equal(ep.flags.cpu().numpy(), want_bits)
            record.append((ep.pos.cpu().numpy().copy(), ep.flags.cpu().numpy().copy(), ep.actions.cpu().numpy().copy()))
        assert [int(v) for v in ep.makespan.tolist()] == [s.makespan for s in states]
        assert [int(v) for v in ep.flowtime.tolist()] == [s.flowtime for s in states]
    return seen, record


@pytest.mark.parametrize("name", list(hw.MOVE_SCENES))
def test_wide_move_equals_oracle(gpu_device, name):
    seen, _ = run_move_scene(name, gpu_device, wide=True, direct=name == "256x40_batched")
    assert seen == 15, seen      # out of the arena, swap, obstacle, cell conflict


def test_wide_move_on_a_narrow_shape_equals_the_narrow_route(gpu_device):
    scene = hw.move_scene(60, 60, False, 60)
    _, narrow = run_move_scene(scene, gpu_device, wide=False)
    _, keyword = run_move_scene(scene, gpu_device, wide=True)
    _, direct = run_move_scene(scene, gpu_device, wide=True, direct=True)
    for a, b, c in zip(narrow, keyword, direct):
        for u, v, w in zip(a, b, c):
            assert np.array_equal(u, v) and np.array_equal(u, w)


def test_wide_move_refusals_and_graph_capture(gpu_device):
    from magat_pathplanning_amd import _native as nat, BatchedEpisode
    from magat_pathplanning_amd.simulator import batched_move
    m, pos, goal = hw.move_inputs("205x205")
    md, pd, gd = dev(m, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device)
    keys = dev(np.random.default_rng(3).integers(0, 5, pos.shape[:2]).astype(np.int32), gpu_device)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):      # without the keyword: the LDS limit as before
        batched_move(md, pd.clone(), actions=keys)
    with pytest.raises(nat.MagatNativeError, match="unsupported"):
        batched_move(torch.zeros(257, 200, dtype=torch.uint8, device=gpu_device), pd.clone(), actions=keys, wide=True)
    need = hw.documented_move_workspace_bytes(3, 205, 205, 40)
    for kwargs, code in ((dict(ws_bytes=need - 1), -2), (dict(null_ws=True), -5)):
        p = pd.clone()
        rc, out = move_wide_direct(md, p, keys, gd, **kwargs)
        torch.cuda.synchronize()
        assert rc == code and torch.equal(p, pd) and bool((out["actions"] == -7).all())
    eager = BatchedEpisode(md, pd, gd, maxstep=50, comm_radius=7.0, wide=True)
    eager.step(actions=keys)
    ep = BatchedEpisode(md, pd, gd, maxstep=50, comm_radius=7.0, wide=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ep.step(actions=keys)                                    # allocates the episode's workspace outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ep.pos.copy_(pd)
    ep.reach_goal.zero_(), ep.first_move.zero_(), ep.end_step.zero_()
    ep.currentstep = 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ep.step(actions=keys)
    ep.pos.copy_(pd)
    ep.reach_goal.zero_(), ep.first_move.zero_(), ep.end_step.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for key in ("pos", "actions", "moves", "flags", "reach_goal", "first_move", "end_step"):
        assert torch.equal(getattr(ep, key), getattr(eager, key)), key


# ---- pipeline -----------------------------------------------------------------------------------------------------------------------
# Chosen on the CPU: cases_restatement.generate("maze", 3, 200, 200, 20, 0.1, 0.01, seed) then mapf_restatement.solve_batch at the
# default horizon 820.  Seed 1, the first tried, has three valid cases, all solved in their first plan, makespans 330, 276, 302;
# the restatements took 0.5 s to generate and 385 s to solve them, so they are not run here.
PIPELINE_SEED = 1
PIPELINE_MAKESPANS = [330, 276, 302]


def test_pipeline_at_200x200(gpu_device):
    """Generator -> solver -> guided episode at 200 x 200, 3 cases of 20 agents.  The seed was chosen on the CPU so that
    tests/cases_restatement.py + tests/mapf_restatement.py solve all three cases: see PIPELINE_SEED's comment."""
    from magat_pathplanning_amd import (BatchedEpisode, expert_schedule, expert_stats, generate_cases, solve_cases, solved_pack)
    cases = generate_cases(3, 200, 200, 20, 0.1, seed=PIPELINE_SEED, device=gpu_device, wide=True)
    assert bool(cases["valid"].all())
    res = solve_cases(cases["map"], cases["start"], cases["goal"], wide=True)
    assert bool(res["solved"].all())
    assert res["makespan"].tolist() == PIPELINE_MAKESPANS
    pack = solved_pack(res)
    T = pack["T"]
    sched = expert_schedule(pack["paths"], pack["lengths"], pack["goal"], pack["makespan"], T=T, check=True)
    keys = sched["target"].argmax(-1).to(torch.int32)
    keys[sched["valid"] == 0] = 4
    stats = expert_stats(sched["target"], pack["start"], pack["goal"], sched["valid"])
    ep = BatchedEpisode(cases["map"], pack["start"], pack["goal"], maxstep=T + 2, comm_radius=7.0, guidance="GlobalG_SD", wide=True)
    ep.currentstep = 1
    x0 = ep.states()
    want = gr.guided_states(cases["map"][0].cpu().numpy(), pack["start"][0].cpu().numpy(), pack["goal"][0].cpu().numpy(),
                            "GlobalG_SD", FOV)
    assert np.array_equal(x0[0, :5].cpu().numpy(), want[:5].astype(np.float32))
    for t in range(T):
        ep.step(actions=keys[:, t].contiguous())
        assert int((ep.flags & 15).max()) == 0, t
        x = ep.states()
    assert tuple(x.shape) == (3, 20, 3, FOV + 2, FOV + 2)
    ep.step(actions=torch.full_like(keys[:, 0], 4))
    assert bool(ep.done.all()) and bool(ep.reach_goal.all()) and torch.equal(ep.pos, pack["goal"])
    assert torch.equal(ep.makespan, stats["makespanTarget"])
