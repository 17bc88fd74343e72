"""GPU: the four kernels of csrc/sim_frontend.hip that every closed loop passes through - gso_kernel<MASK>, sim_radius_kernel,
fov_states_kernel (Project_G) and the narrow sim_move_kernel - beyond the reference's own shapes: more than 300 agents, every LDS
form of the GSO, non-square and per-instance maps, every odd FOV up to 13, ragged chunk splits, the LDS limits and the refusals.
Against oracle/sim_oracle.py, which tests/test_sim_oracle_golden.py pins to the reference at these shapes."""

import numpy as np
import pytest
import torch

import gso_lanczos_restatement as gl
import test_host_sim_sizes as hs
from oracle import sim_oracle as so

pytestmark = pytest.mark.gpu

ERR_BAD_SHAPE, ERR_UNSUPPORTED = -1, -2


def dev(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)      # (a copy: the shared inputs are read-only)


def refused(code):
    return pytest.raises(Exception, match=r"\(code %d\)" % code)


# ---- GSO ---------------------------------------------------------------------------------------------------------------------------
def oracle_lambda(ref, symmetric_norm):
    """The eigenvalue the oracle divided by, from one edge of its result (0.0 for an edgeless instance)."""
    edges = np.argwhere(ref != 0)
    if len(edges) == 0:
        return 0.0
    i, j = edges[0]
    if not symmetric_norm:
        return 1.0 / ref[i, j]
    deg = (ref != 0).sum(1).astype(np.float64)
    return float(np.sqrt(1.0 / deg[i]) * np.sqrt(1.0 / deg[j]) / ref[i, j])


@pytest.mark.parametrize("index", range(10), ids=["N%d" % n for n in hs.gso_sizes()])
def test_gso_at_the_sizes_of_its_forms(gpu_device, index):
    """Edge structure exact, values at rtol 1e-9 in float64 and 1e-6 in float32, lambda_max at 1e-9, both normalisations.
    Measured on an MI355X, relative error of lambda_max: with the walk cut off at 160 steps the chains missed the gate (544
    agents 1.8e-6, 961 and 1000 agents 3.0e-6, the R = 7 band of 1000 agents 1.5e-6, 2048 agents 2.2e-6) and the random graphs
    under the symmetric normalisation came close (960 agents 7.1e-10); walking on up to N steps, 1.8e-13 on the chain of 2048
    agents under the symmetric normalisation and at most 4.4e-15 everywhere else."""
    from magat_pathplanning_amd.simulator import batched_gso
    N, pos, radii, kinds = hs.gso_case(index)
    dpos = dev(pos, gpu_device)
    R = dev(radii, gpu_device) if len(set(radii)) > 1 else float(radii[0])
    for sym in (False, True):
        refs = [so.gso_from_positions(pos[b], radii[b], symmetric_norm=sym) for b in range(len(kinds))]
        lams = [oracle_lambda(r, sym) for r in refs]
        for kind, lam in zip(kinds, lams):
            assert (lam == 0.0) == (kind == "lattice") and hs.well_conditioned(N, lam), (N, kind, sym, lam)
        S, lam = batched_gso(dpos, R, symmetric_norm=sym, return_lambda=True)
        S32 = batched_gso(dpos, R, symmetric_norm=sym, dtype=torch.float32)
        S, lam, S32 = S.cpu().numpy(), lam.cpu().numpy(), S32.cpu().numpy()
        for b, kind in enumerate(kinds):
            print("gso N=%d %s R=%g sym=%d: lambda_max relative error %.2e" %
                  (N, kind, radii[b], sym, abs(lam[b] - lams[b]) / lams[b] if lams[b] else abs(lam[b])))
        for b, kind in enumerate(kinds):
            what = "N=%d %s R=%g sym=%s" % (N, kind, radii[b], sym)
            np.testing.assert_array_equal(S[b] != 0, refs[b] != 0, err_msg=what)
            np.testing.assert_allclose(lam[b], lams[b], rtol=1e-9, atol=0, err_msg=what)
            np.testing.assert_allclose(S[b], refs[b], rtol=1e-9, atol=0, err_msg=what)
            np.testing.assert_array_equal(S32[b] != 0, refs[b] != 0, err_msg=what)
            np.testing.assert_allclose(S32[b], refs[b].astype(np.float32), rtol=1e-6, atol=0, err_msg=what)
    W = batched_gso(dpos, R, normalize=False).cpu().numpy()
    np.testing.assert_array_equal(W, np.stack(refs) != 0)


def test_gso_refuses_more_than_2048_agents_and_writes_nothing(gpu_device):
    from magat_pathplanning_amd import _native as nat
    N = gl.MAX_AGENTS + 1
    pos = dev(hs.gso_graph("path", N, None)[None].astype(np.int32), gpu_device)
    S = torch.full((1, N, N), -7.0, dtype=torch.float64, device=gpu_device)
    lam = torch.full((1,), -7.0, dtype=torch.float64, device=gpu_device)
    radii = torch.full((1,), 4.0, dtype=torch.float64, device=gpu_device)
    with torch.cuda.device(gpu_device):
        stream = nat.current_stream(pos.device)
        assert nat.lib().magat_sim_gso(nat.ptr(pos), 4.0, 0, 1, nat.ptr(S), 1, nat.ptr(lam), 1, N, stream) == ERR_UNSUPPORTED
        assert nat.lib().magat_sim_gso_radii(nat.ptr(pos), nat.ptr(radii), 1, 1, nat.ptr(S), 1, nat.ptr(lam), 1, N,
                                             stream) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((S == -7.0).all()) and float(lam[0]) == -7.0


# ---- connect_radius ------------------------------------------------------------------------------------------------------------------
def radius_case(N):
    """Uniform random (connected after a few steps; denser from 1000 agents on), a block of stacked agents (connected at once;
    not at 5461) and - for the smallest N only - two lattices 40 cells apart that meet after 36 steps: the oracle rebuilds its
    N x N matrix every step and walks every edge in Python."""
    rng = np.random.default_rng(N)
    side = int(np.ceil(np.sqrt(N / (0.55 if N < 1000 else 0.8))))
    pos = [rng.integers(0, side, size=(N, 2))]
    if N < 5000:
        pos.append(rng.integers(0, max(side // 3, 2), size=(N, 2)))
    if N < 1000:
        k = np.arange(N)
        far = np.stack([k % 8, k // 8], 1)
        far[N // 2:, 0] += 47
        pos.append(far)
    return np.stack(pos).astype(np.int32)


@pytest.mark.parametrize("N", [257, 1000, 5461])
def test_connect_radius_beyond_one_pass_of_threads(gpu_device, N):
    from magat_pathplanning_amd.simulator import batched_connect_radius
    assert 12 * N <= 65536 and (N != 5461 or 12 * (N + 1) > 65536)          # 5461: the last size whose 12 N bytes fit
    pos = radius_case(N)
    want = [so.connect_radius(p, 1.5) for p in pos]
    radii, steps = batched_connect_radius(dev(pos, gpu_device), 1.5, return_steps=True)
    print("connect_radius N=%d: growth steps %s" % (N, [s for _, s in want]))
    np.testing.assert_array_equal(radii.cpu().numpy(), np.array([r for r, _ in want]))        # the same float64 products
    np.testing.assert_array_equal(steps.cpu().numpy(), np.array([s for _, s in want]))
    assert N >= 1000 or want[2][1] >= 30


def test_connect_radius_refuses_5462_agents(gpu_device):
    from magat_pathplanning_amd.simulator import batched_connect_radius
    with refused(ERR_UNSUPPORTED):
        batched_connect_radius(torch.zeros(1, 5462, 2, dtype=torch.int32, device=gpu_device), 1.5)


# ---- Project_G states ---------------------------------------------------------------------------------------------------------------
def poison(shape, device):
    """The call under test allocates its result itself, uninitialised: fill the block the allocator will hand out next with
    NaN, so that an element the kernel leaves unwritten cannot pass for a zero."""
    del_me = torch.full(shape, float("nan"), dtype=torch.float32, device=device)
    del del_me


def fov_split(B, N):
    """The workgroups an instance's tensor is spread over (magat_sim_fov_states): doubled while fewer than 512 are in flight and
    each still has at least eight agents' worth."""
    split = 1
    while split < 32 and B * split < 512 and N // (2 * split) >= 4:
        split *= 2
    return split


# (B, N, FOV, H, W, one map per instance)
FOV_CASES = [(2, 1, 3, 17, 40, False), (3, 9, 5, 40, 17, True), (2, 100, 7, 17, 40, True), (2, 255, 9, 40, 17, False),
             (1, 256, 11, 17, 40, False), (1, 257, 13, 40, 17, True), (1, 1000, 9, 17, 40, False), (512, 9, 3, 40, 17, False),
             (2, 40, 13, 17, 40, False)]


def test_fov_cases_cover_every_split_and_ragged_chunks():
    splits = {fov_split(B, N) for B, N, *_ in FOV_CASES}
    assert {1, 2, 16, 32} <= splits
    ragged = [(B, N, F) for B, N, F, *_ in FOV_CASES if (N * 3 * (F + 2) ** 2) % fov_split(B, N)]
    assert len(ragged) >= 3 and any(fov_split(B, N) == 32 for B, N, _ in ragged)
    assert {F for _, _, F, *_ in FOV_CASES} == {3, 5, 7, 9, 11, 13} and {N for _, N, *_ in FOV_CASES} >= {1, 255, 256, 257, 1000}
    assert {(H, W, per) for *_, H, W, per in FOV_CASES} == {(17, 40, False), (17, 40, True), (40, 17, False), (40, 17, True)}


def fov_inputs(B, N, FOV, H, W, per_instance, seed):
    """Agents (stacked where N exceeds the free cells) and goals on free cells inside the map; the first agents get a goal on their
    own cell and goals one cell outside the window on either axis."""
    rng = np.random.default_rng(seed)
    maps = (rng.random((B if per_instance else 1, H, W)) < 0.1).astype(np.uint8)
    pos, goal = np.zeros((B, N, 2), np.int32), np.zeros((B, N, 2), np.int32)
    for b in range(B):
        free = np.argwhere(maps[b if per_instance else 0] == 0)
        pos[b] = free[rng.integers(0, len(free), N)] if N > len(free) else free[rng.permutation(len(free))[:N]]
        goal[b] = free[rng.integers(0, len(free), N)]
        goal[b, 0] = pos[b, 0]
        if N >= 3:
            goal[b, 1] = np.clip(pos[b, 1] + (FOV // 2 + 1, 0), 0, (H - 1, W - 1))
            goal[b, 2] = np.clip(pos[b, 2] - (0, FOV // 2 + 1), 0, (H - 1, W - 1))
    return (maps if per_instance else maps[0]), pos, goal


@pytest.mark.parametrize("case", FOV_CASES, ids=["B%d_N%d_fov%d_%dx%d%s" % (c[:5] + ("_maps" if c[5] else "",)) for c in FOV_CASES])
def test_project_g_states_off_the_square_map(gpu_device, case):
    from magat_pathplanning_amd.simulator import batched_fov_states
    B, N, FOV, H, W, per_instance = case
    m, pos, goal = fov_inputs(B, N, FOV, H, W, per_instance, seed=B * 1000 + N)
    dm, dp, dg = dev(m, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device)
    poison((B, N, 3, FOV + 2, FOV + 2), gpu_device)
    x = batched_fov_states(dm, dp, dg, FOV).cpu().numpy()
    assert x.shape == (B, N, 3, FOV + 2, FOV + 2) and x.dtype == np.float32 and np.isin(x, (0.0, 1.0)).all()
    for b in (range(B) if B <= 3 else (0, 1, B // 2, B - 1)):
        want = so.fov_states(m[b] if per_instance else m, pos[b], goal[b], FOV)
        np.testing.assert_array_equal(x[b], want.astype(np.float32), err_msg="instance %d" % b)
    if B > 3:      # the instances the oracle did not replay: every goal channel holds one mark, the agent sees itself
        assert (x[:, :, 1].sum((-1, -2)) == 1).all() and (x[:, :, 2, FOV // 2 + 1, FOV // 2 + 1] == 1).all()


@pytest.mark.parametrize("FOV", [3, 9, 13])
def test_project_g_goal_rose(gpu_device, FOV):
    """Every agent on the centre of a 41 x 41 map, a goal at every offset in [-20, 20]^2: all octants, the diagonals, and every
    half-to-even tie of the projection."""
    from magat_pathplanning_amd.simulator import batched_fov_states
    off = np.arange(-20, 21)
    goal = (np.stack(np.meshgrid(off, off, indexing="ij"), -1).reshape(1, -1, 2) + 20).astype(np.int32)
    pos = np.full_like(goal, 20)
    m = np.zeros((41, 41), np.uint8)
    dist = (FOV + 2) // 2
    d = (goal[0] - 20).astype(np.int64)
    big = np.maximum(np.abs(d[:, 0]), np.abs(d[:, 1]))
    outside = big > FOV // 2
    assert ((2 * dist * np.minimum(np.abs(d[:, 0]), np.abs(d[:, 1])))[outside] % (2 * big[outside]) == big[outside]).sum() >= 8   # ties
    x = batched_fov_states(dev(m, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device), FOV).cpu().numpy()
    np.testing.assert_array_equal(x[0], so.fov_states(m, pos[0], goal[0], FOV).astype(np.float32))


def test_project_g_at_the_lds_limit_and_refusals(gpu_device):
    """The agent bitmap (a bit a cell) and four bytes an agent share 64 KiB: 512 x 1000 cells and 384 agents fill it to the byte."""
    from magat_pathplanning_amd.simulator import batched_fov_states
    H, W, N, FOV = 512, 1000, 384, 9
    assert 4 * ((H * W + 31) // 32) + 4 * N == 65536
    rng = np.random.default_rng(512)
    m = (rng.random((H, W)) < 0.05).astype(np.uint8)
    pos = np.stack([rng.integers(H - 12, H, N + 1), rng.integers(W - 40, W, N + 1)], 1).astype(np.int32)[None]     # the last words
    pos[0, :4] = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    goal = np.stack([rng.integers(0, H, N + 1), rng.integers(0, W, N + 1)], 1).astype(np.int32)[None]
    goal[0, 4:40] = np.clip(pos[0, 4:40] + rng.integers(-6, 7, (36, 2)), 0, (H - 1, W - 1))
    dm, dp, dg = dev(m, gpu_device), dev(pos, gpu_device), dev(goal, gpu_device)
    x = batched_fov_states(dm, dp[:, :N], dg[:, :N], FOV).cpu().numpy()
    np.testing.assert_array_equal(x[0], so.fov_states(m, pos[0, :N], goal[0, :N], FOV).astype(np.float32))
    with refused(ERR_UNSUPPORTED):
        batched_fov_states(dm, dp, dg, FOV)                                   # one agent more: 65540 bytes
    with refused(ERR_UNSUPPORTED):
        batched_fov_states(torch.zeros(H + 1, W, dtype=torch.uint8, device=gpu_device), dp[:, :N], dg[:, :N], FOV)
    for even in (2, 8, 10):
        with refused(ERR_BAD_SHAPE):
            batched_fov_states(dm, dp[:, :N], dg[:, :N], even)


# ---- narrow move --------------------------------------------------------------------------------------------------------------------
def test_narrow_move_with_the_grid_above_64_kib(gpu_device):
    """190 x 100: 4 H W + 16 N bytes of LDS is past the 64 KiB a kernel gets without asking."""
    import test_gpu_wide_loop as wl
    import test_host_wide_loop as hw
    from magat_pathplanning_amd.simulator import move_needs_wide
    scene = hw.move_scene(190, 100, True, 190100)
    assert 4 * 190 * 100 + 16 * scene[1].shape[1] > 65536 and not move_needs_wide(190, 100, scene[1].shape[1])
    seen, _ = wl.run_move_scene(scene, gpu_device, wide=False)
    assert seen == 15, seen      # out of the arena, swap, obstacle, cell conflict


def test_narrow_move_with_more_agents_than_threads(gpu_device):
    """1100 agents: every per-agent loop of the 1024-thread workgroup takes a second pass."""
    import test_gpu_wide_loop as wl
    scene = hs.crowd_scene(60, 64, 1100, 48, 6064)
    assert scene[1].shape[1] > 1024 and 4 * 60 * 64 + 16 * scene[1].shape[1] <= 65536
    seen, _ = wl.run_move_scene(scene, gpu_device, wide=False)
    assert seen == 15, seen
