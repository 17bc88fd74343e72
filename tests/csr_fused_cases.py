"""Cases, probe weights, references and gates for the fused bf16 CSR layer (csrc/gat_csr_fused.hip: degree ranking, score
kernel, hop kernel, fragment pack), shared by tests/test_host_csr_fused_cases.py (properties of all this, on a CPU) and
tests/test_gpu_csr_fused_probes.py (the kernels against it).  No GPU is needed to import or to evaluate anything here.

The layer (KeyQuery, K = 2, G = F = 128, concat), written from the EDGE LISTS - independent of oracle.magat_oracle and of
graphml.py:

    q'_i,p = W_p^T x_i                      e_ij,p = q'_i,p . x_j      for the edges (i, j)
    a_ij,p = softmax over the out-edges of row i
    z_j,p  = sum over the in-edges (i -> j) of a_ij,p x_i
    y_j,p  = relu(H_p0 x_j + H_p1 z_j,p + bias)

PROBE WEIGHTS make one stage at a time readable at the precision of its own arithmetic (the data is chosen, the arithmetic
is the kernels' own):

    inputs   X in multiples of 1/4 in [-1, 1] (exact in bf16)
    probe Q  W_p = 1/2 x a signed permutation: q' is exact in any order and in bf16, every score is a sum of 128 multiples
             of 1/32 of magnitude <= 1/2 (exact in float32 in any order); only the float32 softmax remains
    probe U  W_p = 0: every score is 0, a_ij = 1 / outdeg(i)
    probe Z  H_p0 = 0, H_p1 = a signed permutation, no bias: y = relu(+-bf16(z)[perm]) - one rounding; run with both signs
    probe X  H_p0 = a signed permutation, H_p1 = 0: y = relu(+-x[perm] + bias) bit for bit

with a different permutation for every head and every tap.  The float32 RESTATEMENT (same formulas in float32, bf16 rounding
at q', z and y) supplies the arithmetic's own error, which the gates scale by 4."""
import functools
import math

import numpy as np
import torch

G = 128
LADDER = (0, 1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 62, 63, 64)      # degrees every ladder instance carries, out AND in
KR = 8                      # gat_csr_fused.hip: slots whose raw scores stay in registers
XCD, WAVES = 8, 8           # MAGAT_NUM_XCD, FUSED_WAVES
CUS = 256                   # compute units of an MI355X: what gat_csr_route.h sizes the fused grids by
CSR_BUILD_MAX_N = 1024      # magat_gso_csr_build (CsrStructure); beyond it the tests hand over the arrays made here

ATT_SUM_TOL = 1e-5          # row sums of the attention
ATT_REL_FLOOR = 3e-6        # max|a - a*| / max a* per row, or 4 x the restatement's own value on that row
MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------------- graphs
class Graph:
    """B instances of N agents as edge lists in CSR order: rows / cols are GLOBAL node numbers b N + i."""

    def __init__(self, N, instances):
        self.B, self.N = len(instances), N
        rows, cols = [], []
        for b, (src, dst) in enumerate(instances):
            src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
            key = np.unique(src * N + dst)                       # sorted by (row, column): the builders' CSR order
            rows.append(b * N + key // N)
            cols.append(b * N + key % N)
        self.rows = torch.from_numpy(np.concatenate(rows)) if rows else torch.zeros(0, dtype=torch.int64)
        self.cols = torch.from_numpy(np.concatenate(cols))
        self.nnz = int(self.rows.numel())
        BN = self.B * N
        self.outdeg = torch.bincount(self.rows, minlength=BN)
        self.indeg = torch.bincount(self.cols, minlength=BN)

    def arrays(self):
        """magat_gso_csr_build's conventions: rowptr / cscptr [B (N + 1)] absolute offsets, colidx ascending per row (local),
        cscsrc / cscpos per in-edge in ascending source row: the local source and the edge's CSR position."""
        B, N = self.B, self.N

        def ptr(deg):
            ends = torch.cumsum(deg, 0).view(B, N)
            p = torch.empty(B, N + 1, dtype=torch.int64)
            p[:, 1:] = ends
            p[0, 0] = 0
            p[1:, 0] = ends[:-1, -1]
            return p.reshape(-1).to(torch.int32)

        order = torch.argsort(self.cols * (B * N) + self.rows)             # (keys are unique: no tie to break)
        return {"rowptr": ptr(self.outdeg), "colidx": (self.cols % N).to(torch.int32), "cscptr": ptr(self.indeg),
                "cscsrc": (self.rows[order] % N).to(torch.int32), "cscpos": order.to(torch.int32)}

    def dense(self):
        S = torch.zeros(self.B * self.N, self.N)
        S[self.rows, self.cols % self.N] = 1.0
        return S.view(self.B, self.N, self.N)

    def last_out_edge(self):
        """index of the last stored edge of every row with more than KR edges, and those rows"""
        rows = torch.nonzero(self.outdeg > KR).reshape(-1)
        ends = torch.cumsum(self.outdeg, 0)
        return ends[rows] - 1, rows

    def last_in_edge(self):
        """CSR index of the last in-edge (largest source) of every column with more than KR in-edges, and those columns"""
        order = torch.argsort(self.cols * (self.B * self.N) + self.rows)
        cols = torch.nonzero(self.indeg > KR).reshape(-1)
        ends = torch.cumsum(self.indeg, 0)
        return order[ends[cols] - 1], cols


def _pairs(rng, rows, cols, count):
    """`count` distinct targets out of `cols` for every node of `rows` (count: one number per row)"""
    src, dst = [], []
    for r, c in zip(rows, count):
        pool = cols[cols != r]
        t = rng.choice(pool, size=min(int(c), len(pool)), replace=False)
        src.append(np.full(len(t), r))
        dst.append(t)
    return np.concatenate(src), np.concatenate(dst)


def ladder_instance(N, seed, hubs):
    """A directed graph whose out-degrees AND in-degrees each take every value of LADDER, set independently: node A[k] has
    out-degree LADDER[k] and in-degree LADDER[-1 - k] (the lightest row of the out-ranking is the heaviest column of the
    in-ranking), its partners are filler nodes, and the fillers have 0 .. 12 edges among themselves.  hubs: one filler row
    reaches every other node and one filler column is reached by every other node (N - 1 each) - every other degree of that
    instance is then one higher (no 0 in it: that is what the instance without hubs is for)."""
    rng = np.random.default_rng(seed)
    L = len(LADDER)
    nodes = rng.permutation(N)
    A, fill = nodes[:L], nodes[L + 2:]
    s1, d1 = _pairs(rng, A, fill, LADDER)
    d2, s2 = _pairs(rng, A, fill, LADDER[::-1])
    s3, d3 = _pairs(rng, fill, fill, rng.integers(0, 13, size=len(fill)))
    src, dst = [s1, s2, s3], [d1, d2, d3]
    if hubs:
        hr, hc = nodes[L], nodes[L + 1]
        others = np.arange(N)
        src += [np.full(N - 1, hr), others[others != hc]]
        dst += [others[others != hr], np.full(N - 1, hc)]
    return np.concatenate(src), np.concatenate(dst)


def random_instance(N, avg, seed, directed=True, hub=False, empty=0):
    """about `avg` edges per agent; hub: row N // 3 reaches everyone and column N // 2 is reached by everyone; empty: the
    first `empty` rows lose their out-edges.  N = 1: the self-loop alone."""
    rng = np.random.default_rng(seed)
    if N == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64)
    m = int(avg * N) if directed else int(avg * N) // 2
    src, dst = rng.integers(0, N, size=m), rng.integers(0, N, size=m)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    if not directed:
        src, dst = np.concatenate((src, dst)), np.concatenate((dst, src))
    if hub:
        o = np.arange(N)
        src = np.concatenate((src, np.full(N - 1, N // 3), o[o != N // 2]))
        dst = np.concatenate((dst, o[o != N // 3], np.full(N - 1, N // 2)))
    keep = src >= empty
    return src[keep], dst[keep]


def geometric_positions(B, N, side, seed):
    """(B, N, 2) distinct integer cells of a side x side map"""
    rng = np.random.default_rng(seed)
    cells = np.stack([rng.permutation(side * side)[:N] for _ in range(B)])
    return torch.from_numpy(np.stack((cells // side, cells % side), axis=-1).astype(np.int32))


def geometric_instance(pos, radius):
    """the simulator's edge test sqrt(d^2) < radius, no self-loops (pos (N, 2) integer cells)"""
    p = pos.to(torch.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    adj = (d2.double().sqrt() < radius) & ~torch.eye(p.shape[0], dtype=torch.bool)
    i, j = torch.nonzero(adj, as_tuple=True)
    return i.numpy(), j.numpy()


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    """name, B, N, P and how the graph is made; score_probes: the score weights its attention and hop gates run under;
    random: the random-weights gate runs on it too; probe X runs on every case with both result types, bias_on names the
    result type whose run carries the non-zero bias."""

    def __init__(self, name, B, N, P, make, score_probes=("Q", "U"), random=False, bias_on="f32", route="csr"):
        self.name, self.B, self.N, self.P, self._make = name, B, N, P, make
        self.score_probes, self.random, self.bias_on, self.route = score_probes, random, bias_on, route
        self.seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))

    def __repr__(self):
        return self.name

    @functools.cached_property
    def graph(self):
        g = Graph(self.N, [self._make(self, b) for b in range(self.B)])
        assert g.B == self.B
        return g

    @functools.cached_property
    def X(self):
        """(B N, 128) float32 multiples of 1/4 in [-1, 1]"""
        gen = torch.Generator().manual_seed(self.seed)
        return (torch.randint(-4, 5, (self.B * self.N, G), generator=gen).float() / 4.0)

    @functools.cached_property
    def probes(self):
        return Probes(self.P, self.seed)

    @functools.cached_property
    def positions(self):
        return geometric_positions(self.B, self.N, 40, self.seed) if self.route == "edges" else None


def _ladder(case, b):
    return ladder_instance(case.N, 100 + b, hubs=(b == 1))


def _rand(avg, directed=True, hub=False, empty=0):
    return lambda case, b: random_instance(case.N, avg, case.seed + b, directed, hub and b == 0, empty if b % 2 == 0 else 0)


def _single(case, b):                      # N = 1: instance 1 has no edge at all
    return (np.zeros(0, np.int64),) * 2 if b == 1 else random_instance(1, 0, 0)


EDGES_RADIUS = 3.5


def _geo(case, b):
    return geometric_instance(case.positions[b], EDGES_RADIUS)


CASES = [
    # the degree ladder: instance 0 without hubs (degree 0 both ways), instance 1 with a hub row and a hub column
    Case("ladder-P4", 2, 330, 4, _ladder, random=True),
    Case("ladder-P2", 2, 330, 2, _ladder, bias_on="bf16"),
    Case("ladder-P1", 2, 330, 1, _ladder),
    # N around the 32-row group and the 8-group chunk; B around the 8 XCDs
    Case("N1-B3-P4", 3, 1, 4, _single, bias_on="bf16"),
    Case("N31-B8-P2", 8, 31, 2, _rand(6, hub=True)),
    Case("N32-B9-P1", 9, 32, 1, _rand(6, directed=False), bias_on="bf16"),
    Case("N33-B17-P4", 17, 33, 4, _rand(5, empty=9)),
    Case("N255-B1-P2", 1, 255, 2, _rand(6, directed=False, hub=True), bias_on="bf16"),
    Case("N256-B1-P4", 1, 256, 4, _rand(6, empty=40)),
    Case("N257-B9-P4", 9, 257, 4, _rand(6, hub=True), random=True),          # nchunk = 2, two XCD rounds of instances
    Case("N1024-B1-P2", 1, 1024, 2, _rand(6, hub=True), bias_on="bf16"),
    # beyond the structure builder and the split form's tiled route: the arrays made here go to the kernels as they are
    Case("N2500-B1-P4", 1, 2500, 4, _rand(6, hub=True)),
    # ceil(64 / 8) * 5 = 40 items per XCD on 32 workgroups: a second trip of the persistent loops, waves rotated
    Case("trip2-B64-N1100-P2", 64, 1100, 2, _rand(4), score_probes=("U",), bias_on="bf16"),
    # the edge structure made from agent positions (addGSO(batched_edges(..)) hands these arrays to the same kernels)
    Case("edges-B2-N300-P4", 2, 300, 4, _geo, route="edges"),
]
CASE = {c.name: c for c in CASES}


def geometry(case, cus=CUS):
    """gat_csr_route.h, restated: groups, chunks, items per XCD and the two fused grids; trips of the persistent loops"""
    per_xcd = max(cus // XCD, 1)
    ng = (case.N + 31) // 32
    nchunk = (ng + WAVES - 1) // WAVES
    items = (case.B + XCD - 1) // XCD * nchunk
    ngrp = case.P // 2 if case.P >= 2 else 1
    per = max(per_xcd // ngrp, 1)
    return {"ng": ng, "nchunk": nchunk, "items": items, "grid_scores": XCD * min(items, per_xcd),
            "grid_hop": XCD * ngrp * min(items, per), "ngrp": ngrp,
            "trips_scores": -(-items // min(items, per_xcd)), "trips_hop": -(-items // min(items, per))}


# ---------------------------------------------------------------------------------------------------------------- probes
def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype) if x.dtype == torch.float32 else rne_bf16_f64(x)


def rne_bf16_f64(x):
    """round to 8 significant bits, ties to even, from float64 directly (no double rounding through float32); normal range"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


class Probes:
    """The probe weights of P heads.  W (P,128,128) is layer.weight[:, 0] (q'[h] = sum_g x[g] W[g][h]); H (P,128,2,128) is
    layer.filterWeight[:, :, 0] (y[f] = sum_g H[f][k][g] v_k[g])."""

    def __init__(self, P, seed):
        rng = np.random.default_rng(seed + 7)
        self.P = P
        self.perm_w = torch.from_numpy(np.stack([rng.permutation(G) for _ in range(P)]))
        self.sign_w = torch.from_numpy(rng.choice([-1.0, 1.0], size=(P, G))).float()
        self.perm_h = torch.from_numpy(np.stack([[rng.permutation(G) for _ in range(2)] for _ in range(P)]))     # (P,2,128)
        self.sign_h = torch.from_numpy(rng.choice([-1.0, 1.0], size=(P, 2, G))).float()
        self.bias = torch.from_numpy(rng.integers(-8, 9, size=G) / 8.0).float()                                 # [-1, 1] in 1/8

    def w_q(self):
        W = torch.zeros(self.P, G, G)
        for p in range(self.P):
            W[p, torch.arange(G), self.perm_w[p]] = 0.5 * self.sign_w[p]
        return W

    def w_u(self):
        return torch.zeros(self.P, G, G)

    def h(self, tap, flip=1.0):
        """H with the signed permutation of tap `tap` in place and the other tap zero"""
        H = torch.zeros(self.P, G, 2, G)
        for p in range(self.P):
            H[p, torch.arange(G), tap, self.perm_h[p, tap]] = flip * self.sign_h[p, tap]
        return H

    def read(self, v, tap, flip=1.0, bias=None):
        """what the layer must give for per-head vectors v (P, rows, 128) under h(tap, flip): (rows, P 128)"""
        out = []
        for p in range(self.P):
            t = (flip * self.sign_h[p, tap]).to(v.dtype) * v[p][:, self.perm_h[p, tap]]
            if bias is not None:
                t = t + bias.to(v.dtype)
            out.append(torch.relu(t))
        return torch.cat(out, dim=1)


def random_weights(P, seed):
    """the layer's own initialisation range, and a visible bias"""
    gen = torch.Generator().manual_seed(seed + 3)
    s = 1.0 / math.sqrt(G * P)
    W = (torch.rand(P, G, G, generator=gen) * 2 - 1) * s
    H = (torch.rand(P, G, 2, G, generator=gen) * 2 - 1) * s
    b = torch.randn(G, generator=gen) * 0.05
    return W, H, b


def random_inputs(case):
    gen = torch.Generator().manual_seed(case.seed + 5)
    return bf16(torch.randn(case.B * case.N, G, generator=gen) * 0.5)


# ------------------------------------------------------------------------------------------- the layer from the edge lists
def _edge_scores(q, X, rows, cols):
    out = torch.empty(q.shape[0], rows.numel(), dtype=q.dtype)
    for lo in range(0, rows.numel(), 1 << 16):
        r, c = rows[lo:lo + (1 << 16)], cols[lo:lo + (1 << 16)]
        out[:, lo:lo + (1 << 16)] = (q[:, r] * X[c].unsqueeze(0)).sum(-1)
    return out


def row_softmax(sc, rows, BN):
    a = torch.empty_like(sc)
    for p in range(sc.shape[0]):
        mx = torch.full((BN,), -math.inf, dtype=sc.dtype).scatter_reduce(0, rows, sc[p], "amax", include_self=True)
        e = torch.exp(sc[p] - mx[rows])
        sm = torch.zeros(BN, dtype=sc.dtype).index_add_(0, rows, e)
        a[p] = e / sm[rows]
    return a


def hop(a, X, rows, cols, BN):
    z = torch.zeros(a.shape[0], BN, G, dtype=X.dtype)
    for p in range(a.shape[0]):
        for lo in range(0, rows.numel(), 1 << 16):
            sl = slice(lo, lo + (1 << 16))
            z[p].index_add_(0, cols[sl], a[p, sl].unsqueeze(1) * X[rows[sl]])
    return z


def taps(X, z, H, bias):
    """relu(H_p0 x + H_p1 z_p + bias) -> (rows, P 128)"""
    y = torch.einsum("ng,pfg->npf", X, H[:, :, 0]) + torch.einsum("png,pfg->npf", z, H[:, :, 1])
    if bias is not None:
        y = y + bias.to(y.dtype).view(1, 1, G)
    return torch.relu(y).reshape(X.shape[0], -1)


class Stages:
    """q', scores, attention (P, nnz) and the hop (P, B N, 128) of one graph, inputs and score weights.
    dtype float64: the reference (no rounding anywhere, unless round16: RNE at q' and z - 'the same order');
    dtype float32: the restatement - bf16 rounding at q' (z is kept BEFORE its rounding as z, rounded as z16)."""

    def __init__(self, g, X, W, dtype, round16=None, mutate=None):
        round16 = (dtype == torch.float32) if round16 is None else round16
        BN = g.B * g.N
        X, W = X.to(dtype), W.to(dtype)
        self.q = torch.einsum("ng,pgh->pnh", X, W)
        if round16:
            self.q = bf16(self.q)
        self.scores = _edge_scores(self.q, X, g.rows, g.cols)
        sc = self.scores
        if mutate == "softmax":                     # the last out-edge of every row with more than KR edges is left out
            sc = sc.clone()
            sc[:, g.last_out_edge()[0]] = -math.inf
        self.att = row_softmax(sc, g.rows, BN)
        if mutate == "heads":                       # heads 1 and 2 exchanged
            self.att = self.att[[0, 2, 1, 3]]
        a = self.att
        if mutate == "hop":                         # the last in-edge of every column with more than KR in-edges is left out
            a = a.clone()
            a[:, g.last_in_edge()[0]] = 0.0
        self.z = hop(a, X, g.rows, g.cols, BN)
        self.z16 = bf16(self.z) if round16 else self.z


def online_softmax_f32(g, scores):
    """The score kernel's softmax, restated in float32 in its slot order: running maximum and rescaled sum edge by edge, the
    exponential as exp2(x * log2 e) with the product and the result rounded to float32, a = exp(s - max) * (1 / sum)."""
    sc = scores.to(torch.float32).numpy()
    P = sc.shape[0]
    BN = g.B * g.N
    deg = g.outdeg.numpy()
    start = np.concatenate(([0], np.cumsum(deg)[:-1]))
    l2e = np.float32(1.4426950408889634)

    def ex(x):
        with np.errstate(invalid="ignore"):
            t = (x.astype(np.float32) * l2e).astype(np.float32)
            return np.exp2(t.astype(np.float64)).astype(np.float32)

    mx = np.full((P, BN), -np.inf, np.float32)
    sm = np.zeros((P, BN), np.float32)
    byrank = np.argsort(-deg, kind="stable")
    sdeg = deg[byrank]
    for k in range(int(deg.max()) if BN else 0):
        act = byrank[:np.searchsorted(-sdeg, -k, side="left")]            # rows with more than k edges
        s = sc[:, start[act] + k]
        m2 = np.maximum(mx[:, act], s)
        sm[:, act] = (sm[:, act] * ex(mx[:, act] - m2)).astype(np.float32) + ex(s - m2)
        mx[:, act] = m2
    with np.errstate(divide="ignore"):
        inv = np.where(sm > 0, np.float32(1.0) / sm, np.float32(0.0)).astype(np.float32)
    rows = g.rows.numpy()
    return torch.from_numpy((ex(sc - mx[:, rows]) * inv[:, rows]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def stages(name, probe, dtype):
    """cached per (case, 'Q' | 'U', dtype)"""
    case = CASE[name]
    W = case.probes.w_q() if probe == "Q" else case.probes.w_u()
    return Stages(case.graph, case.X, W, dtype)


# ----------------------------------------------------------------------------------------------------------------- gates
def _row_max(v, rows, BN):
    """per (head, row) maximum of the non-negative per-edge values v (P, nnz); 0 for rows without edges"""
    out = torch.zeros(v.shape[0], BN, dtype=v.dtype)
    for p in range(v.shape[0]):
        out[p].scatter_reduce_(0, rows, v[p], "amax", include_self=True)
    return out


def attention_error(g, a, ref):
    """per (head, row): max|a - a*| / max a*  (0 for rows without edges), in float64"""
    BN = g.B * g.N
    a, ref = a.double(), ref.double()
    top = _row_max(ref, g.rows, BN)
    err = _row_max((a - ref).abs(), g.rows, BN)
    return torch.where(top > 0, err / top.clamp_min(1e-300), torch.zeros_like(err))


def attention_gate(g, a, ref64, own):
    """DESIGN 4.5's per-edge gates, per head: row sums within 1e-5 of 1 (0 for a row without edges); per row with an edge
    max|a - a*| / max a* <= max(3e-6, 4 x `own`), own = attention_error of the arithmetic's restatement on that row.
    -> (bad (P, B N) bool, worst row-sum error, worst ratio error / bound, worst error)"""
    BN = g.B * g.N
    sums = torch.zeros(a.shape[0], BN, dtype=torch.float64)
    for p in range(a.shape[0]):
        sums[p].index_add_(0, g.rows, a[p].double())
    want = (g.outdeg > 0).double().unsqueeze(0)
    sum_err = (sums - want).abs()
    err = attention_error(g, a, ref64)
    bound = torch.clamp(MARGIN * own, min=ATT_REL_FLOOR)
    bad = (sum_err > ATT_SUM_TOL) | (err > bound)
    return bad, float(sum_err.max()) if BN else 0.0, float((err / bound).max()), float(err.max())


def uniform_gate(g, a):
    """probe U: every value within one float32 ulp of 1 / outdeg, exact where outdeg is a power of two -> edges that miss"""
    d = g.outdeg[g.rows]
    want = (1.0 / d.double()).float()
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, 2.0)) - want).double()
    diff = (a.double() - want.double().unsqueeze(0)).abs()
    pow2 = (d & (d - 1)) == 0
    return (diff > ulp.unsqueeze(0)) | (pow2.unsqueeze(0) & (diff > 0))


def hop_bound(case, st64, st32):
    """per (head, column): t = 4 x the restatement's own distance from float64 before rounding, floor 1e-6 max|x|"""
    own = (st32.z.double() - st64.z).abs().amax(dim=2)
    return torch.clamp(MARGIN * own, min=1e-6 * float(case.X.abs().max()))


def hop_gate(case, y, st64, t, flip):
    """probe Z: |y - relu(+-z*[perm])| <= 2^-8 |z*| + t for every element (the RNE bound of the one bf16 rounding plus the
    arithmetic's own error), rows without in-edges exactly 0.  y (B N, P 128).
    -> (bad (B N, P) bool per column and head, worst excess / bound)"""
    pr = case.probes
    want = pr.read(st64.z, 1, flip)
    mag = torch.cat([st64.z[p][:, pr.perm_h[p, 1]].abs() for p in range(case.P)], dim=1)
    tt = torch.repeat_interleave(t.t(), G, dim=1)                                   # (B N, P 128)
    bound = 2.0 ** -8 * mag + tt
    diff = (y.double() - want).abs()
    bad = diff > bound
    lone = (case.graph.indeg == 0).unsqueeze(1)
    bad |= lone & (y != 0)
    BN = y.shape[0]
    return bad.view(BN, case.P, G).any(dim=2), float((diff / bound).max())


# --------------------------------------------------------------------------------------------- random weights, per row
def emulation(case, W, H, bias, X):
    """the oracle's emulation of the fused order (dense GSO; the yardstick the existing tests use) -> (B N, P 128)"""
    from oracle import magat_oracle as orc
    B, N, P = case.B, case.N, case.P
    params = {"weight": W.unsqueeze(1), "filterWeight": H.unsqueeze(2), "bias": bias.view(G, 1)}
    y, _ = orc.gat_layer_forward_bf16_fused(X.view(B, N, G).permute(0, 2, 1).contiguous(), case.graph.dense().unsqueeze(1), params)
    return y.permute(0, 2, 1).reshape(B * N, P * G).contiguous()


def same_order_f64(case, W, H, bias, X):
    """float64 arithmetic from the edge lists with RNE to bf16 where the kernels round: operands, q', z, y"""
    st = Stages(case.graph, X.double(), bf16(W).double(), torch.float64, round16=True)
    return rne_bf16_f64(taps(X.double(), st.z16, bf16(H).double(), bias.double()))


def row_budget(y_emul, y_same):
    """c and floor of the per-row gate  max_f |y - y_emul| <= c max(row scale, floor), row scale = max_f |y_emul|, from the
    emulation's own distance d to the float64 evaluation of the same order: floor = the largest d of any row (a row whose
    scale is below it cannot be held to anything finer), c = 4 x the largest d / max(row scale, floor)."""
    d = (y_emul.double() - y_same).abs().amax(dim=1)
    scale = y_emul.double().abs().amax(dim=1)
    floor = float(d.max())
    c = MARGIN * float((d / scale.clamp_min(max(floor, 1e-30))).max())
    return c, floor
