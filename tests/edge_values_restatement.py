"""The GSO's values on the edge structure, restated in numpy: what magat_gso_edge_values (csrc/gso_edge_values.hip) must produce.
TEST INFRASTRUCTURE: imported by tests/test_host_edge_values.py and tests/test_gpu_edge_values.py.

Nothing new is stated here: the arrays are edges_restatement's (rule 0), lambda_max is gso_lanczos_restatement.lambda_max - the rule
of gso_kernel for more than 128 agents, which the new kernel follows at every size - and the values are gso_kernel's expressions
in float64, rounded to float32 once: 1 / div, or (inv[i] * inv[j]) / div under symmetric_norm, inv = sqrt(1 / degree) (0 for an
isolated agent), div = lambda_max when the instance has an edge and normalize is set, else 1."""
import numpy as np

import edges_restatement as er
import gso_lanczos_restatement as lr


def edge_values(pos, radii, symmetric_norm=False, normalize=True):
    """pos (B,N,2) integers, radii one number or (B,) -> dict(rowptr, colidx, nnz as edges_restatement.edge_arrays; lam (B,)
    float64, vals (nnz,) float32 in CSR order, steps (B,) Lanczos steps taken)"""
    pos = np.asarray(pos)
    B, N, _ = pos.shape
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (B,))
    A = er.edge_pattern(pos, radii, 0)
    out = er.arrays_of_pattern(A)
    lam, steps, vals = np.zeros(B), np.zeros(B, dtype=np.int64), []
    for b in range(B):
        deg = A[b].sum(1)
        inv = np.ones(N)
        if symmetric_norm:
            inv = np.where(deg > 0, np.sqrt(1.0 / np.maximum(deg, 1)), 0.0)
        i, j = np.nonzero(A[b])
        if normalize and len(i):
            lam[b], steps[b] = lr.lambda_max(pos[b], radii[b], symmetric_norm)
        div = lam[b] if normalize and len(i) else 1.0
        v = (inv[i] * 1.0 * inv[j]) / div if symmetric_norm else np.full(len(i), 1.0 / div)
        vals.append(v.astype(np.float32))
    out.update(lam=lam, steps=steps, vals=np.concatenate(vals) if vals else np.zeros(0, np.float32))
    return out


def matrix(pos, radius, symmetric_norm=False):
    """the float64 matrix lambda_max belongs to: W, or D^-1/2 W D^-1/2"""
    return lr.adjacency(pos, radius, symmetric_norm)[3]


def ulps32(got, want):
    """distance of two float32 arrays in units of the last place of `want`"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ---- the cases of tests/test_host_edge_values.py, tests/test_gpu_edge_values.py and tools/host_wave/gso_edge_values_check.cpp ------
def case_positions(B, N, seed=0):
    """edges_restatement.case_positions' cells (about 12 neighbours at radius 7; instance 0 with its cluster of 65 agents) under
    per-instance radii: a batch of three is typical, edgeless (0.5: distinct cells), one clique (a radius beyond the map); a batch
    of two typical and clique.  -> (pos (B,N,2) int32, radii (B,) float64)"""
    pos, _ = er.case_positions(B, N, seed)
    radii = np.full(B, 7.0)
    if B == 2:
        radii[1] = 1.0e6
    elif B >= 3:
        radii[1], radii[2] = 0.5, 1.0e6
    return pos, radii


def lattice(a, b):
    """a x b cells of a grid, one agent each: under radius 1.2 the 4-neighbour grid graph, lambda_max = 2 cos(pi / (a + 1)) +
    2 cos(pi / (b + 1)) (the sum of two path graphs); under symmetric_norm 1 (no agent is isolated)"""
    r, c = np.divmod(np.arange(a * b), b)
    return np.stack([r, c], axis=1).astype(np.int32)[None]


def lattice_lambda(a, b):
    return 2.0 * np.cos(np.pi / (a + 1)) + 2.0 * np.cos(np.pi / (b + 1))


def random_cells(N, side=256, seed=0):
    """N distinct cells of a side x side map -> (1,N,2) int32"""
    cells = np.random.default_rng(seed + 7 * N).permutation(side * side)[:N]
    return np.stack([cells // side, cells % side], axis=1).astype(np.int32)[None]


def dump_case(arrays, B, N, cap, symmetric_norm, normalize, lds_limit=128 * 1024):
    """the text file of tools/host_wave/gso_edge_values_check.cpp from edge_arrays' dict"""
    kept = arrays["colidx"][:cap]
    return "%d %d %d %d %d %d %d\n%s\n%s\n" % (B, N, cap, int(symmetric_norm), int(normalize), lds_limit, arrays["nnz"],
                                             " ".join(str(int(v)) for v in arrays["rowptr"]), " ".join(str(int(v)) for v in kept))


def parse_result(text):
    lines = text.split("\n")
    return dict(rc=int(lines[0]), lam=np.array([float.fromhex(w) for w in lines[1].split()]),
                vals=np.array([float.fromhex(w) if "nan" not in w else np.nan for w in lines[2].split()], dtype=np.float32))
