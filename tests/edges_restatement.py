"""The communication graph from agent positions, restated in numpy: what magat_gso_edges_build (csrc/gso_edges.hip) must produce.

The rule is the reference's own (utils/new_simulator.py, computeAdjacencyMatrix): (i, j), i != j, is an edge when the float64
square root of the squared differences is < r; the diagonal is zero; edge rule 1 (GAT_origin, GAT_Similarity: |float(S) + I| > 1e-9)
adds every (i, i).  The arrays follow include/magat_hip.h, magat_gso_csr_build's conventions: rowptr [B*(N+1)] absolute offsets,
colidx ascending in j per row, and per in-edge of a column, in ascending source row, the source (cscsrc) and the position of that
edge in CSR order (cscpos), with cscptr [B*(N+1)] the columns' absolute offsets.  Nothing here uses the graph's symmetry: the column
view is made by sorting the edges."""
import numpy as np


def edge_pattern(pos, radii, rule=0):
    """pos (B,N,2) integers, radii one number or (B,) -> bool (B,N,N)"""
    pos = np.asarray(pos)
    B, N, _ = pos.shape
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (B,))
    out = np.zeros((B, N, N), dtype=bool)
    p = pos.astype(np.float64)
    for b in range(B):
        for i0 in range(0, N, 512):      # (row blocks: 4096 agents are 16.7 M pairs)
            d = p[b, i0:i0 + 512, None, :] - p[b, None, :, :]
            out[b, i0:i0 + 512] = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) < radii[b]
        idx = np.arange(N)
        out[b, idx, idx] = bool(rule)
    return out


def arrays_of_pattern(A, cap=None):
    """bool (B,N,N) -> dict(rowptr, colidx, cscptr, cscsrc, cscpos, nnz); with `cap`, the index arrays keep their first cap entries"""
    B, N, _ = A.shape
    rowptr, cscptr = np.zeros((B, N + 1), dtype=np.int64), np.zeros((B, N + 1), dtype=np.int64)
    colidx, cscsrc, cscpos = [], [], []
    base = 0
    for b in range(B):
        rows, cols = np.nonzero(A[b])                      # row-major: CSR order
        rowptr[b] = base + np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=N))))
        cscptr[b] = base + np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=N))))
        order = np.lexsort((rows, cols))                   # by column, then by source row
        colidx.append(cols)
        cscsrc.append(rows[order])
        cscpos.append(base + order)
        base += len(rows)
    cat = lambda parts: np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)      # noqa: E731
    out = dict(rowptr=rowptr.reshape(-1).astype(np.int32), cscptr=cscptr.reshape(-1).astype(np.int32), colidx=cat(colidx),
               cscsrc=cat(cscsrc), cscpos=cat(cscpos), nnz=int(base))
    if cap is not None:
        for k in ("colidx", "cscsrc", "cscpos"):
            out[k] = out[k][:cap]
    return out


def edge_arrays(pos, radii, rule=0, cap=None):
    return arrays_of_pattern(edge_pattern(pos, radii, rule), cap)


def dense(pos, radii, dtype=np.float32):
    """the 0 / 1 adjacency without the diagonal: what GraphEdges.dense() hands over"""
    return edge_pattern(pos, radii, 0).astype(dtype)


# ---- the cases of tests/test_gpu_edges.py and tools/host_wave/gso_edges_check.cpp ------------------------------------------------
def case_positions(B, N, seed=0):
    """B instances of N agents on a map sized for about 12 neighbours at radius 7, plus what the words' edges need: instance 0
    holds a clique (up to 65 agents inside one radius, side by side on one map row) whose members sit on indices 0 .. 64 - rows
    and columns 63 | 64 of the bit words; the last instance of a batch is edgeless at radius 0.5 (distinct cells).
    -> (pos (B,N,2) int32, radii (B,) float64)"""
    rng = np.random.default_rng(1000 * N + 10 * B + seed)
    side = max(int(np.ceil(np.sqrt(N * 13.0))), 8)
    pos = np.zeros((B, N, 2), dtype=np.int32)
    for b in range(B):
        cells = rng.permutation(side * side)[:N]
        pos[b, :, 0], pos[b, :, 1] = cells // side, cells % side
    radii = 7.0 + 0.37 * np.arange(B, dtype=np.float64)
    k = min(N, 65)
    pos[0, :k, 0], pos[0, :k, 1] = side + 40, np.arange(k) // 11          # 65 agents within 5 cells of one another, off the others
    if B > 1:
        radii[B - 1] = 0.5
    return pos, radii


CASE_N = (1, 2, 63, 64, 65, 128, 129, 1000, 1024, 1025, 2049, 4096)
CASE_B = (1, 3)


# ---- the text files of tools/host_wave/gso_edges_check.cpp -----------------------------------------------------------------------
def dump_case(pos, radii, rule, cap):
    """radii: one number (the entry's comm_radius) or (B,) per-instance radii"""
    pos = np.asarray(pos)
    per_instance = np.ndim(radii) > 0
    words = [float(r).hex() for r in (np.asarray(radii, dtype=np.float64).reshape(-1) if per_instance else [radii])]
    return "%d %d %d %d %d\n%s\n%s\n" % (pos.shape[0], pos.shape[1], rule, cap, int(per_instance), " ".join(words),
                                         " ".join(str(int(v)) for v in pos.reshape(-1)))


def parse_result(text):
    lines = text.split("\n")
    out = dict(rc=int(lines[0]), nnz=int(lines[1]))
    for k, ln in zip(("rowptr", "colidx", "cscptr", "cscsrc", "cscpos"), lines[2:7]):
        out[k] = np.array(ln.split(), dtype=np.int32)
    return out
