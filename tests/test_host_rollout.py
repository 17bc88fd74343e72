"""CPU-only checks of the case pool (magat_pathplanning_amd/rollout.py, csrc/sim_pool.hip): the plain restatement
(tests/rollout_restatement.py) against the fixtures the real reference made - rollout_* (the agent's loop with per-case limits,
the real MonitoringMultiAgentPerformance) and simepisode_* -, its independence of the slot count, the refill order written out by
hand, reference_maxstep, the turn and uniforms kernels compiled for the host (tools/host_wave) against the restatement, and the
host side of the entries: header / loader / build lists / refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import audit_restatement as ar
import rollout_cases as rc
import rollout_restatement as rr
from conftest import ROOT


def fixture_policy(z, by_case_step):
    """logits / uniforms of a fixture gathered by (slot_case, slot_step); an idle slot gets zeros."""
    def logits(pool):
        return np.stack([by_case_step("logits", c, t) if c >= 0 else np.zeros((pool.N, 5), np.float32)
                         for c, t in zip(pool.slot_case, pool.slot_step)])

    def uniforms(pool):
        return np.stack([by_case_step("uniforms", c, t) if c >= 0 else np.zeros(pool.N) for c, t in zip(pool.slot_case, pool.slot_step)])
    return logits, uniforms


def run_fixture(pool, logits, uniforms):
    while not pool.finished():
        pool.step(logits=logits(pool), uniforms=uniforms(pool) if pool.policy else None)
        assert pool.calls < 10000
    return pool.rows


# ---- the restatement against the reference's fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", rc.ROLLOUT, ids=[os.path.basename(p)[:-4] for p in rc.ROLLOUT])
def test_restatement_equals_the_reference_loop_and_monitor(path):
    from magat_pathplanning_amd import summarize_rollouts
    z = np.load(path)
    C, N = z["start"].shape[:2]
    assert (z["steps"] >= z["maxstep"]).any() and len(set(z["maxstep"].tolist())) > 1
    for c in range(C):                                        # each case's limit is the reference's own product
        assert z["maxstep"][c] == rr.reference_maxstep(z["makespanTarget"][c], N, float(z["rate_maxstep"]))
    logits, uniforms = fixture_policy(z, lambda key, c, t: z[key][c, t])
    pool = rr.Pool(z["map"], z["start"], z["goal"], z["maxstep"], 2, 7.0, policy=int(z["policy"]), first_step=1)
    rows = run_fixture(pool, logits, uniforms)
    rc.assert_rows_equal(rows, rc.rollout_rows(z), os.path.basename(path))
    log, s = rr.summary(rows, z["maxstep"], z["makespanTarget"], z["flowtimeTarget"], N)
    for key in rc.LOG_FIELDS:                                 # every log_result field, equal
        np.testing.assert_array_equal(np.array([l[key] for l in log]).astype(np.int64), z[key].astype(np.int64), err_msg=key)
    for key in rc.RATES:
        np.testing.assert_allclose(s[key], float(z["summary_" + key]), rtol=1e-12, atol=0, err_msg=key)
    np.testing.assert_array_equal(s["hist_numAgentReachGoal"], z["hist_numAgentReachGoal"])
    # the package's summary on the same rows (arrays on the host)
    res = {key: pool.column(key) for key in ("all_reach", "num_reach", "steps", "makespan", "flowtime", "predicted_collision", "end_pos")}
    rc.assert_summary_equals_fixture(summarize_rollouts(dict(res, maxstep=z["maxstep"]), z["makespanTarget"], z["flowtimeTarget"]), z)


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("path", rc.EPISODE, ids=[os.path.basename(p)[:-4] for p in rc.EPISODE])
def test_restatement_equals_the_episode_fixtures(path, slots):
    z = np.load(path)
    assert len(rc.EPISODE) == 8
    B = z["pos0"].shape[0]
    logits, uniforms = fixture_policy(z, lambda key, c, t: z[key][c, t])
    pool = rr.Pool(z["map"], z["pos0"], z["goal"], int(z["maxstep"]), min(slots, B), 7.0, policy=int(z["policy"]), first_step=0)
    rows = run_fixture(pool, logits, uniforms)
    assert len(pool.refills) == B and pool.calls > max(r["steps"] for r in rows)      # refills happened
    rc.assert_rows_equal(rows, rc.episode_rows(z), os.path.basename(path))


def alone_rows(slots, policy, record=False):
    maps, start, goal = rc.alone_cases_numpy()
    a = rc.ALONE
    pool = rr.Pool(maps, start, goal, a["maxstep"], slots, a["comm_radius"], policy=policy, seed=a["pool_seed"], first_step=1,
                   record=record)
    rr.run(pool, lambda p: rc.push_logits_numpy(p.pos(), p.slot_goal()))
    return pool


@pytest.mark.parametrize("policy", [0, 2])
def test_a_case_does_not_depend_on_the_slot_count(policy):
    ref = alone_rows(1, policy).rows
    assert [r["steps"] for r in ref][4] == 1 and {r["all_reach"] for r in ref} == {0, 1}
    for slots in (3, rc.ALONE["C"]):
        got = alone_rows(slots, policy).rows
        for c, (g, w) in enumerate(zip(got, ref)):
            for key in rr.COLUMNS:
                np.testing.assert_array_equal(np.asarray(g[key]), np.asarray(w[key]), err_msg="slots %d case %d %s" % (slots, c, key))


def test_refill_order_by_hand():
    """5 slots over 9 cases whose agents never move (their key is stop, the goals lie elsewhere): a case ends at the call whose
    step number reaches its limit.  Slots 1 and 3 finish together at call 2; four slots finish together at call 5 with one case
    left."""
    maxstep = [5, 2, 5, 2, 5, 3, 1, 4, 4]
    m = np.zeros((6, 6), np.uint8)
    start = np.tile(np.array([[0, 0], [0, 2]]), (9, 1, 1))
    goal = np.tile(np.array([[5, 5], [5, 3]]), (9, 1, 1))
    pool = rr.Pool(m, start, goal, maxstep, 5, 7.0, first_step=1)
    seen = []
    while not pool.finished():
        pool.step(keys=np.full((5, 2), 4))
        seen.append((list(pool.slot_case), list(pool.slot_step)))
    assert pool.refills == [(0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 3, 3), (0, 4, 4), (2, 1, 5), (2, 3, 6), (3, 3, 7), (5, 0, 8)]
    assert seen[0] == ([0, 1, 2, 3, 4], [2, 2, 2, 2, 2])
    assert seen[1] == ([0, 5, 2, 6, 4], [3, 1, 3, 1, 3])
    assert seen[2] == ([0, 5, 2, 7, 4], [4, 2, 4, 1, 4])
    assert seen[4][0] == [8, -1, -1, 7, -1] and seen[4][1][0] == 1 and seen[4][1][3] == 3
    assert pool.calls == 9 and seen[-1][0] == [-1] * 5
    assert [r["steps"] for r in pool.rows] == maxstep and not any(r["all_reach"] for r in pool.rows)


def test_reference_maxstep():
    from magat_pathplanning_amd import reference_maxstep
    assert reference_maxstep(7, 19, 2) == 14 and reference_maxstep(7, 20, 2) == 21 and reference_maxstep(7, 100, 1.5) == 21
    assert reference_maxstep(7, 19, 2.5) == 17 and reference_maxstep(9, 4, 1.3) == 11      # 17.5, 11.700000000000001: truncated
    np.testing.assert_array_equal(reference_maxstep(np.array([7, 8, 13]), 10, 2.5), [17, 20, 32])
    np.testing.assert_array_equal(reference_maxstep(torch.tensor([7, 8]), 30, 2.5), [21, 24])
    for mk, n, rate in ((7, 19, 2), (7, 20, 2), (9, 4, 1.3), (13, 8, 2.5)):
        assert reference_maxstep(mk, n, rate) == rr.reference_maxstep(mk, n, rate) == int(torch.tensor(mk).type(torch.int32) * (3 if n >= 20 else rate))


def test_trajectories_of_the_alone_set_pass_the_audit():
    """The shield's own moves are a valid schedule: no vertex or swap conflict, no obstacle, one of the five moves per step."""
    maps, start, goal = rc.alone_cases_numpy()
    for policy in (0, 2):
        pool = alone_rows(3, policy, record=True)
        for c in range(rc.ALONE["C"]):
            cells = np.stack(pool.traj[c])                    # (L,N,2)
            L = len(cells)
            assert L == pool.rows[c]["steps"] - 1 + 1 and (cells[0] == start[c]).all()
            np.testing.assert_array_equal(cells[-1], pool.rows[c]["end_pos"])
            out = ar.audit(maps[c], start[c], cells[-1], cells.transpose(1, 0, 2), np.full(rc.ALONE["N"], L))
            assert out["status"] == 0, (policy, c, out)


# ---- the kernels themselves, compiled for the host (tools/host_wave) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "sim_pool_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-pthread", "-I", os.path.join(ROOT, "tools", "host_wave"), "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "sim_pool_check.cpp"), "-o", exe], check=True)
    return exe


def stand_in_step(pool, H):
    """tools/host_wave/sim_pool_check.cpp's rule on the restatement's pool."""
    for b in range(pool.B):
        pool.over[b] = False
        c, t = pool.slot_case[b], pool.slot_step[b]
        if c < 0:
            continue
        st = pool.state[b]
        pool.over[b] = t >= st.maxstep
        pool.done[b] = bool((c + t) % 2)
        st.makespan, st.flowtime = 100 + t, 200 + c + t
        if pool.over[b]:
            continue
        pool.sticky[b] |= 1 << (t % 6)
        for n in range(pool.N):
            st.pos[n, 0] = (st.pos[n, 0] + 1) % H
            if (n + t) % 3 == 0:
                st.reach_goal[n] = 1
                if st.end_step[n] == 0:
                    st.end_step[n] = t
            if n % 2 == 0 and st.first_move[n] == 0:
                st.first_move[n] = t
    pool._turn()
    pool.calls += 1


@pytest.mark.parametrize("first_step,slots", [(1, 3), (0, 5), (1, 1)])
def test_host_kernels_equal_the_restatement(pool_check, tmp_path, first_step, slots):
    rng = np.random.default_rng(5 + slots)
    C, N, H, W, seed, radius = 7, 5, 9, 12, 0xDEADBEEFCAFE, 1.5
    maps = (rng.random((C, H, W)) < 0.2).astype(np.uint8)
    start = np.stack([np.stack([rng.permutation(H)[:N], rng.permutation(W)[:N]], 1) for _ in range(C)])
    start[3] = [[0, 0], [0, 11], [8, 0], [8, 11], [4, 6]]      # far apart: the radius grows many times
    goal = np.stack([np.stack([rng.permutation(H)[:N], rng.permutation(W)[:N]], 1) for _ in range(C)])
    maxstep = np.array([3, 1, 4, 2, 6, 1, 2])
    cells = int(maxstep.max()) - first_step + 1
    pool = rr.Pool(maps, start, goal, maxstep, slots, radius, seed=seed, first_step=first_step, record=True)
    calls = 0
    sim = rr.Pool(maps, start, goal, maxstep, slots, radius, seed=seed, first_step=first_step)
    while not sim.finished():
        stand_in_step(sim, H)
        calls += 1
    calls += 2                                               # idle turns behind the end
    text = "%d %d %d %d %d %d 1 %d %d %d %d %r\n" % (slots, N, H, W, C, first_step, cells, rr.RADIUS_MAX_STEPS, calls, seed, radius)
    text += "\n".join(" ".join(str(int(v)) for v in np.asarray(a).reshape(-1)) for a in (maps, start, goal, maxstep)) + "\n"
    (tmp_path / "case.txt").write_text(text)
    out = subprocess.run([pool_check, str(tmp_path / "case.txt")], check=True, capture_output=True, text=True).stdout.split("\n")
    ints = lambda s: [int(v) for v in s.split()]              # noqa: E731
    floats = lambda s: [float.fromhex(v) for v in s.split()]  # noqa: E731
    assert int(out[0]) == 0
    k = 1
    for call in range(calls):
        assert floats(out[k]) == pool.uniforms().reshape(-1).tolist(), "uniforms, call %d" % call
        stand_in_step(pool, H)
        assert ints(out[k + 1]) == pool.slot_case, call
        active = [b for b in range(slots) if pool.slot_case[b] >= 0]
        assert [ints(out[k + 2])[b] for b in active] == [pool.slot_step[b] for b in active]
        assert [ints(out[k + 3])[b] for b in active] == [pool.state[b].maxstep for b in active]
        assert floats(out[k + 4]) == pool.radii                # bit for bit
        assert ints(out[k + 5]) == [pool.next, pool.remaining]
        assert ints(out[k + 6]) == pool.pos().reshape(-1).tolist()
        k += 7
    assert pool.finished() and all(c == -1 for c in pool.slot_case)
    rows = np.array(ints(out[k])).reshape(9, C)
    for i, name in enumerate(rr.COLUMNS[:9]):
        np.testing.assert_array_equal(rows[i], pool.column(name), err_msg=name)
    assert floats(out[k + 1]) == [r["radius"] for r in pool.rows]
    assert max(floats(out[k + 1])) > radius * 1.1 ** 5
    for j, name in ((2, "end_pos"), (3, "first_move"), (4, "end_step")):
        assert ints(out[k + j]) == pool.column(name).reshape(-1).tolist(), name
    steps = pool.column("steps")
    assert ints(out[k + 5]) == (steps - first_step + 1).tolist()
    traj = np.array(ints(out[k + 6])).reshape(C, N, cells)
    for c in range(C):
        want = np.stack(pool.traj[c])                         # (L,N,2)
        assert len(want) == steps[c] - first_step + 1
        np.testing.assert_array_equal(traj[c, :, :len(want)], (want[:, :, 0] << 8 | want[:, :, 1]).T)
    u = np.array(floats(out[1]))
    assert ((u >= 0) & (u < 1)).all() and len(set(u.tolist())) == len(u)
    assert any((float(v) * 2 ** 53) % 2 == 1 for v in u)      # the 53rd bit is drawn


def test_uniforms_are_keyed_on_the_case_not_the_slot():
    a = rr.case_uniforms(7, 3, 5, 4)
    assert (a == rr.case_uniforms(7, 3, 5, 4)).all() and (a != rr.case_uniforms(7, 4, 5, 4)).all()
    assert (a != rr.case_uniforms(7, 3, 6, 4)).all() and (a != rr.case_uniforms(8, 3, 5, 4)).all()
    assert ((a >= 0) & (a < 1)).all()


# ---- the host side of the entries --------------------------------------------------------------------------------------------------------
def test_pool_entries_are_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    src = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "sim_pool.hip")).read()
    front = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "sim_frontend.hip")).read()
    assert "sim_pool.hip" in build_native.SOURCES
    for name, nargs in (("magat_sim_pool_step", 7), ("magat_sim_pool_step_wide", 9), ("magat_sim_pool_turn", 3),
                        ("magat_sim_pool_uniforms", 7)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl and name in nat.EXPORTED_SYMBOLS and re.search(r'extern "C" int %s\(' % name, src)
        res, sig = nat._SIGNATURES[name]
        assert res is ctypes.c_int and len(decl.group(1).split(",")) == len(sig) == nargs
    # ONE copy of the move step: the pool launches sim_frontend.hip's kernel, it has none of its own
    assert len(re.findall(r"void sim_move_kernel\(", front)) == 1 and "sim_move_kernel" not in src and "magat_sim_step_slots" in src
    assert "wave_sum_int" in src and "sim_graph_connected" in src and "sim_dist2_bound" in src and "draw32" in src
    fields = re.search(r"typedef struct magat_sim_pool_desc \{(.*?)\} magat_sim_pool_desc;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:, (\w+))?(?:, (\w+))?(?:, (\w+))?(?:, (\w+))?(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", fields))
    assert [n for g in names for n in g if n] == [f for f, _ in nat.SimPoolDesc._fields_]
    cols = re.findall(r"#define MAGAT_POOL_(\w+) (\d+)", hdr)
    assert [c.lower() for c, _ in cols[:9]] == ["retired", "all_reach", "num_reach", "steps", "makespan", "flowtime", "predicted",
                                                "flag_bits", "status"]
    assert [int(v) for _, v in cols[:10]] == list(range(10)) and len(nat.POOL_COLUMNS) == 9
    assert nat.POOL_STATUS_DISCONNECTED == int(dict(cols)["STATUS_DISCONNECTED"]) == 2
    for name in ("EpisodePool", "evaluate_cases", "reference_maxstep", "summarize_rollouts"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                           # loads without a GPU
    assert lib.magat_abi_version() == 9
    p = 16
    assert lib.magat_sim_pool_turn(None, 0, None) == -5 and lib.magat_sim_pool_uniforms(None, p, p, 0, 2, 2, None) == -5
    assert lib.magat_sim_pool_uniforms(p, p, p, 0, 0, 2, None) == -1
    assert lib.magat_sim_pool_step(None, p, p, p, p, p, None) == -5
    d = nat.SimStepDesc()
    assert lib.magat_sim_pool_step(ctypes.byref(d), p, p, p, p, None, None) == -5


def test_python_surface_refuses_on_the_host():
    from magat_pathplanning_amd import EpisodePool
    from magat_pathplanning_amd import _native as nat
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)       # noqa: E731
    m = torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(nat.MagatNativeError, match="device tensor"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), 5, 2, 7.0)
    with pytest.raises(ValueError, match="slots"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), 5, 5, 7.0)
    with pytest.raises(ValueError, match="slots"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), 5, 0, 7.0)
    with pytest.raises(ValueError, match="maxstep"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), 0, 2, 7.0)
    with pytest.raises(ValueError, match="action_select"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), 5, 2, 7.0, action_select="greedy")
    with pytest.raises(nat.MagatNativeError, match="device"):
        EpisodePool(m, i32(4, 3, 2), i32(4, 3, 2), torch.tensor([5, 5, 5, 5]), 2, 7.0)
