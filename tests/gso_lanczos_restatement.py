"""numpy restatement of the lambda_max rule of gso_kernel (csrc/sim_frontend.hip) for more than 128 agents, and of its LDS sizes.
TEST INFRASTRUCTURE: imported by tests/test_host_sim_sizes.py and tests/test_gpu_sim_sizes.py.

The rule: Lanczos on W (or D^-1/2 W D^-1/2) from the all-ones vector, no re-orthogonalisation; the largest eigenvalue of the
tridiagonal T_steps is located every 8 steps up to 160 steps, then every 32, then every eighth of the largest power of two below
the step count; stop at the second location in a row that moved by at most 1e-13 relative, at an invariant subspace, or after
N steps.  `cap` puts an upper limit on the steps: cap=160 is the rule the kernel had before it walked on.

The location here is the same 256-probe multisection on the pivot form of the Sturm count as the kernel's."""
import numpy as np

LDS_LIMIT = 160 * 1024
DYN_LDS = 64 * 1024
LMIN = 160
MAX_AGENTS = 2048


def lanczos_cap(N):
    return max(N, LMIN)


def gso_lds_bytes(N, mask):
    """gso_lds_bytes of csrc/sim_frontend.hip for N > 128: int32 coordinates, v / y / inv, 16 reduction slots, alpha [cap] and
    beta [cap + 2], and with `mask` the bit rows of W."""
    b = 2 * N * 4 + 8 + 3 * N * 8 + (16 + 2 * lanczos_cap(N) + 2) * 8
    if mask:
        b += N * ((N + 31) // 32) * 4
    return b


def uses_mask(N):
    return gso_lds_bytes(N, True) <= LDS_LIMIT


def last_size_within(limit, mask=True):
    """The largest N whose instance fits `limit` bytes."""
    N = 129
    while gso_lds_bytes(N + 1, mask) <= limit:
        N += 1
    return N


def adjacency(pos, R, symmetric_norm):
    """(edge rows i, edge columns j, inv [N], the float64 matrix the eigenvalue belongs to)."""
    pos = np.asarray(pos, np.float64)
    d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
    W = d < R
    np.fill_diagonal(W, False)
    deg = W.sum(1)
    inv = np.ones(len(pos))
    if symmetric_norm:
        inv = np.where(deg > 0, np.sqrt(1.0 / np.maximum(deg, 1)), 0.0)
    i, j = np.nonzero(W)
    return i, j, inv, inv[:, None] * W * inv[None, :]


def tridiagonal_max(alpha, beta, steps):
    """Largest eigenvalue of T_steps (diagonal alpha[0..steps), off-diagonal beta[1..steps)): multisection from the Gershgorin
    interval, 256 probes a pass, eigenvalues below a probe = negative pivots of T - x I."""
    a, b = np.asarray(alpha[:steps]), np.abs(np.asarray(beta[:steps + 1]))
    off = np.zeros(steps)
    off[1:] += b[1:steps]
    off[:-1] += b[1:steps]
    lo, hi = float((a - off).min()), float((a + off).max())
    for _ in range(12):
        if not hi - lo > 4e-16 * max(abs(lo), abs(hi)):
            break
        x = lo + (hi - lo) * np.arange(1, 257) / 257.0
        d = np.ones(256)
        below = np.zeros(256, np.int64)
        for r in range(steps):
            d = (a[r] - x) - (b[r] * b[r] / d if r else 0.0)
            d[d == 0.0] = 1e-300
            below += d < 0.0
        ge = np.nonzero(below < steps)[0]
        bt = int(ge.max()) if len(ge) else -1
        nlo = lo + (hi - lo) * (bt + 1) / 257.0 if bt >= 0 else lo
        nhi = lo + (hi - lo) * (bt + 2) / 257.0 if bt + 1 < 256 else hi
        lo, hi = nlo, nhi
    return 0.5 * (lo + hi)


def check_stride(steps):
    if steps <= LMIN:
        return 8
    return max(32, (1 << (steps.bit_length() - 1)) >> 3)


def lambda_max(pos, R, symmetric_norm=False, cap=None):
    """(lambda_max by the kernel's rule, Lanczos steps taken); 0.0 for an edgeless instance."""
    i, j, inv, _ = adjacency(pos, R, symmetric_norm)
    N = len(pos)
    if len(i) == 0:
        return 0.0, 0
    cap = lanczos_cap(N) if cap is None else cap
    v, vprev = np.full(N, 1.0 / np.sqrt(float(N))), np.zeros(N)
    alpha, beta = [], [0.0]
    prev, stable, lam, steps = -1.0, 0, 0.0, 0
    for k in range(cap):
        w = inv * np.bincount(i, weights=(inv * v)[j], minlength=N) - beta[k] * vprev
        ak = float(v @ w)
        w = w - ak * v
        bn = float(np.sqrt(w @ w))
        alpha.append(ak)
        beta.append(bn)
        steps = k + 1
        breakdown = not bn > 1e-13 * (abs(ak) + beta[k] + 1.0)
        vprev = v
        if not breakdown:
            v = w / bn
        if breakdown or steps % check_stride(steps) == 0 or steps == cap or steps >= N:
            lam = tridiagonal_max(alpha, beta, steps)
            if breakdown or steps >= N:
                break
            if abs(lam - prev) <= 1e-13 * abs(lam):
                stable += 1
                if stable >= 2:
                    break
            else:
                stable = 0
            prev = lam
    return lam, steps
