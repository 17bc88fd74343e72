"""Cases, inputs and references of the inference tests of the graph layers on the CSR kernels (csrc/gat_csr_f32.hip) and of every
layer type past 1024 agents.  tests/test_gpu_large_graph.py runs them on the device, tests/test_host_large_graph.py checks on
the CPU that every case still has the property it was made for and computes the float32 composite's own error.

Three lists, one case type:
  FORCED   the per-edge kernels (csr_scores_kernel, csr_hop_kernel, csr_k1_kernel, the in-call csr_transpose_kernel and
           csr_sort_columns_kernel) at their smallest shapes; the test switches the LDS-tiled kernels off (option CSR_TILED = 0)
  TILED    the FORCED cases the tiled kernels accept (`tiled_route`), plus hubs / dense / half-empty graphs at the ends of the
           tiled range; run with CSR_TILED = 3
  LARGE    every layer type at 1025 ... 8190 agents through the module, nothing forced; `train` marks the ones that also run one
           forward + backward in train() mode

Yardstick: graphml._composite in float64 on the CPU for y and the attention values (GraphFilterBatch: the float64 hop algebra of
train_graph_cases.gnn_reference), bf16 storage: oracle.magat_oracle.gat_layer_forward_bf16_storage.  Every input is a float32
value.  The attention tensor is kept on the edges only, (edges, P) in CSR order - the order the kernels store it in; the edge list
itself is the definition of the layer's rule, restated here with torch (`edge_mask`), not taken from the composite."""
import functools
import types

import torch

import train_graph_cases as tg
from similarity_train_cases import gso_no_edge_row

KQ, GM, GO, SIM, GNN = tg.KQ, tg.GM, tg.GO, "GAT_Similarity", "GNN"
Y_GATE = 2e-5            # of max(1, max|want|): the figure of test_gat_csr_path_vs_oracle
ATT_ABS = 3e-6           # absolute, every attention value: the figure of test_gat_csr_path_vs_oracle
ATT_ROW = 3e-6           # per row with edges: max_j |a - a*| / max_j a*
ATT_SUM = 1e-5           # every row with edges sums to 1
BF16_EMUL, BF16_FP32, BF16_ATT = 2.0 ** -7, 2e-2, 4e-3       # the budgets of test_gat_csr_bf16_storage
TRAIN_GATE = tg.GATE
TILED_MIN_N, TILED_MAX_N, MAX_N = 8, 1024, 8190
ZERO_ROW, TINY_ROW = (0, 12), (0, 14)        # (instance, agent) of the GAT_Similarity cases: |x| = 0 and x scaled by 1e-12


# ---- GSOs -----------------------------------------------------------------------------------------------------------------------
def gso_tiny(B, N, seed):
    """N = 1: a self-loop, nothing, a -3e-9 self-loop.  N = 3: rows of degree 1, 3, 0 / 1 (the -3e-9; 5e-10 is none), 0, 2 / full."""
    S = torch.zeros(B, N, N, dtype=torch.float64)
    if N == 1:
        S[0, 0, 0], S[2, 0, 0] = 0.5, -3e-9
    else:
        S[0] = torch.tensor([[0, 0.5, 0], [0.3, 0.2, 0.5], [0, 0, 0]])
        S[1] = torch.tensor([[0, 5e-10, -3e-9], [0, 0, 0], [0.4, 0, 0.6]])
        S[2] = tg.gso_full(1, N, seed)[0]
    return S


def gso_degrees(B, N, seed):
    """N >= 18.  Nodes 18 .. N-1: ~3 directed edges per row among themselves.  Node 0 is isolated; nodes 1, 2, 3 only send (1, 2, 3
    edges, to 12 .. 14); nodes 4, 5, 6 only receive (1, 2, 3 edges, from 15 .. 17); (7, 8) holds 5e-10 - no edge - and (8, 7) holds
    -3e-9 - an edge."""
    S = torch.zeros(B, N, N, dtype=torch.float64)
    if N > 18:
        S[:, 18:, 18:] = tg._background(B, N - 18, 3, tg._gen(seed))
    for d in (1, 2, 3):
        S[:, d, 12:12 + d] = 0.3 / d
        S[:, 15:15 + d, 3 + d] = -0.25
    S[:, 7, 8], S[:, 8, 7] = 5e-10, -3e-9
    return S


def _kind(kind):
    """The graphs of test_tiled_csr_kernels_against_the_per_edge_kernels, directed and with values: ~3 edges per row plus a row and
    a column of degree N (hubs), ~40 per row (dense), ~1 per row in the second half and none in the first (empty)."""
    def gso(B, N, seed):
        g = tg._gen(seed)
        dens = {"dense": min(0.5, 40.0 / N), "hubs": 3.0 / N, "empty": 1.0 / N}[kind]
        m = torch.rand(B, N, N, generator=g) < dens
        v = ((torch.rand(B, N, N, generator=g) * 0.8 + 0.2) / max(1.0, dens * N)).double()
        S = m * v * (torch.randint(0, 2, (B, N, N), generator=g) * 2 - 1)
        if kind == "hubs":
            S[:, N // 3, :] = 1.0 / N
            S[:, :, N // 2] = 1.0 / N
        if kind == "empty":
            S[:, : N // 2, :] = 0
        return S
    gso.__name__ = "gso_" + kind
    return gso


gso_khubs, gso_kdense, gso_kempty = _kind("hubs"), _kind("dense"), _kind("empty")


def gso_past(B, N, seed):
    """Past 1024 agents: ~4 directed edges per row; node 3 points at every node and every node points at node 7 (instance 0; in
    instance 1 the hubs are 4 and 8); node 5 is isolated, node 9 only sends; (20, 21) holds 5e-10 and (21, 20) holds -3e-9."""
    S = tg._background(B, N, 4, tg._gen(seed))
    for b in range(B):
        S[b, 3 + b, :] = 1.0 / N
        S[b, :, 7 + b] = 1.0 / N
    S[:, 5, :] = 0
    S[:, :, 5] = 0
    S[:, :, 9] = 0
    S[:, 9, 30:34] = 0.1
    S[:, 20, 21], S[:, 21, 20] = 5e-10, -3e-9
    return S


def gso_limit(B, N, seed):
    """~4 directed edges per row, a row (node 3) and a column (node 7) of degree exactly N, five rows (40 .. 44) whose only edge is
    the one into node 7, an edge (30, N - 1) in the last column, and the two rule-sensitive entries."""
    S = tg._background(B, N, 4, tg._gen(seed))
    S[:, 40:45, :] = 0
    S[:, 20, 21], S[:, 21, 20] = 5e-10, -3e-9
    S[:, 30, N - 1] = 0.3
    S[:, 3, :] = 1.0 / N
    S[:, :, 7] = 1.0 / N
    return S


def gso_structure(B, N, seed):
    """gso_limit with rows 40 .. 44 empty altogether (node 7's column has N - 5 edges) - for the structure kernels."""
    S = gso_limit(B, N, seed)
    S[:, 40:45, :] = 0
    return S


@functools.lru_cache(maxsize=None)
def gso_of(fn, B, N, seed, f64):
    """The GSO of a case in the dtype it is handed over in; made once per process and shared by the cases that name the same one."""
    S = fn(B, N, seed)
    return S if f64 else S.float()


def edge_mask(S, mode):
    """(B,N,N) bool, the layer's edge rule on the GSO as handed over: |S| > 1e-9 in S's dtype; GAT_origin and GAT_Similarity:
    |float(S) + I| > 1e-9; GraphFilterBatch: float(S) != 0."""
    if mode in (GO, SIM):
        return (S.float() + torch.eye(S.shape[-1])).abs() > 1e-9
    if mode == GNN:
        return S.float() != 0
    return S.abs() > 1e-9


def tiled_route(opt, mode, N, G, F, K, bf16, att):
    """tiled_ok and its callers in csrc/gat_csr_route.h, restated: (scores tiled, hops tiled) under option CSR_TILED = opt.  The tiled score
    kernel serves KeyQuery only (GAT_Similarity and the rank-1 modes keep the per-edge one, GraphFilterBatch has no scores); a
    kernel is tiled when its bit of the option is set, 8 <= N <= 1024 and a row of its width is a multiple of 128 bytes."""
    esz = 2 if bf16 else 4
    size = TILED_MIN_N <= N <= TILED_MAX_N
    scores = bool(opt & 1) and size and mode == KQ and (G * esz) % 128 == 0 and (K > 1 or att)
    hops = bool(opt & 2) and size and mode != SIM and (F * esz) % 128 == 0 and K > 1
    return scores, hops


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _case(group, mode, concat, gso, B, N, G, K, P, F=None, f64=False, att=True, bf16=False, distinct=False, train=False,
          gseed=None, tiny=False):
    return types.SimpleNamespace(group=group, mode=mode, concat=concat, gso=gso, B=B, N=N, G=G, F=F or G, K=K, P=P, f64=f64, att=att,
                                 bf16=bf16, distinct=distinct, train=train, gseed=gseed, tiny=tiny, nin=N, clamp=tiny)


def _index(cases, first_seed):
    out = {}
    for k in cases:
        k.id = "%s-%s-%s-%s-B%dN%dG%dK%dP%d" % (k.group, k.mode, "cat" if k.concat else "mean", k.gso.__name__[4:], k.B, k.N, k.G,
                                                 k.K, k.P)
        k.id += ("F%d" % k.F if k.F != k.G else "") + ("-f64" if k.f64 else "") + ("" if k.att else "-noatt") + \
                ("-bf16" if k.bf16 else "")
        assert k.id not in out, k.id
        k.seed = first_seed + len(out)
        if k.gseed is None:
            k.gseed = k.seed
        out[k.id] = k
    return out


def _forced_cases():
    c = []
    # row tiles and their tails: scores 32 rows per block (64 at width 16), hops 4; N = 1, 3, 33, 65; degrees 0 .. 3 both ways
    c += [_case("tails", KQ, True, gso_tiny, 3, 1, 256, 3, 2),
          _case("tails", GM, False, gso_tiny, 3, 3, 16, 2, 3),
          _case("tails", GO, True, gso_tiny, 3, 3, 256, 3, 1, att=False),
          _case("tails", KQ, False, gso_degrees, 2, 33, 16, 3, 4),
          _case("tails", KQ, True, gso_degrees, 2, 33, 32, 2, 4, f64=True),
          _case("tails", GM, True, gso_degrees, 2, 65, 16, 3, 1),
          _case("tails", GO, False, gso_degrees, 2, 33, 128, 2, 2, f64=True),
          _case("tails", GM, False, gso_degrees, 3, 65, 256, 2, 4, att=False),
          _case("tails", KQ, True, gso_degrees, 2, 65, 64, 4, 3),
          _case("tails", GO, True, gso_degrees, 2, 65, 16, 5, 2)]
    # rows and columns of degree N, all pairs, no edges, the -1 diagonal that cancels GAT_origin's self-loop
    c += [_case("degree", KQ, True, tg.gso_hubs, 2, 130, 64, 3, 2),
          _case("degree", GM, False, tg.gso_hubs, 2, 130, 32, 2, 1),
          _case("degree", GO, True, tg.gso_hubs, 2, 130, 64, 3, 4, f64=True),
          _case("degree", KQ, False, tg.gso_full, 1, 70, 128, 2, 3),
          _case("degree", GM, True, tg.gso_full, 1, 70, 64, 3, 2),
          _case("degree", GO, False, tg.gso_full, 1, 70, 32, 2, 4, att=False),
          _case("degree", KQ, True, tg.gso_edgeless, 2, 8, 64, 3, 1),
          _case("degree", GO, True, tg.gso_edgeless, 2, 8, 128, 2, 1),
          _case("degree", GM, True, tg.gso_first_edgeless, 2, 8, 128, 3, 3),
          _case("degree", GO, False, gso_no_edge_row, 2, 12, 32, 3, 3)]
    # depth: K = 1 with the attention (scores + csr_k1_kernel) and without (csr_k1_kernel alone); K = 4, 5: both hop buffers
    c += [_case("depth", KQ, True, gso_degrees, 2, 33, 32, 1, 2),
          _case("depth", GM, False, gso_degrees, 2, 33, 64, 1, 3, att=False),
          _case("depth", KQ, False, tg.gso_rounds, 3, 21, 128, 5, 4),
          _case("depth", GM, True, tg.gso_rounds, 3, 21, 256, 4, 3)]
    # instance index past the first and the second round of eight
    c += [_case("rounds", KQ, True, tg.gso_rounds, 9, 10, 32, 3, 3, distinct=True),
          _case("rounds", GM, False, tg.gso_rounds, 17, 10, 64, 2, 2, distinct=True),
          _case("rounds", GO, True, tg.gso_rounds, 9, 10, 16, 3, 4, distinct=True)]
    # GraphFilterBatch: the edge values are the weights, every non-zero float(S) is an edge (5e-10 too), G != F
    c += [_case("gnn", GNN, True, gso_degrees, 2, 33, 32, 3, 1, F=64, f64=True, att=False),
          _case("gnn", GNN, True, tg.gso_hubs, 2, 130, 64, 2, 1, F=16, att=False)]
    # bf16 storage: the u16 instantiations of the per-edge kernels
    c += [_case("bf16", KQ, True, tg.gso_hubs, 2, 130, 32, 3, 2, bf16=True),
          _case("bf16", GM, False, gso_degrees, 2, 65, 64, 2, 4, bf16=True),
          _case("bf16", KQ, True, gso_degrees, 2, 33, 128, 2, 4, bf16=True),
          _case("bf16", GO, True, tg.gso_hubs, 2, 130, 128, 3, 1, bf16=True)]
    return _index(c, 5000)


FORCED = _forced_cases()


def _tiled_cases():
    c = [_case("tiled", KQ, True, gso_khubs, 2, 255, 128, 2, 4),
         _case("tiled", KQ, False, gso_kdense, 2, 513, 64, 3, 1),
         _case("tiled", GM, True, gso_kempty, 3, 9, 64, 2, 2),
         _case("tiled", GO, True, gso_khubs, 1, 1024, 32, 3, 2),
         _case("tiled", KQ, True, gso_kempty, 1, 1024, 256, 4, 1, f64=True),
         _case("tiled", GNN, True, gso_kdense, 2, 255, 32, 3, 1, F=64, att=False),
         _case("tiled", KQ, True, gso_khubs, 2, 513, 64, 3, 2, bf16=True),
         _case("tiled", GM, False, gso_kdense, 3, 9, 128, 2, 4, bf16=True)]
    out = {cid: k for cid, k in FORCED.items() if any(tiled_route(3, k.mode, k.N, k.G, k.F, k.K, k.bf16, k.att))}
    out.update(_index(c, 5500))
    return out


TILED = _tiled_cases()


def _large_cases():
    s1025, s1100, s2048, s8190 = 6001, 6002, 6003, 6004        # one GSO per size, shared by the cases of that size
    c = [_case("past", KQ, True, gso_past, 1, 1025, 32, 3, 2, gseed=s1025, train=True),
         _case("past", GM, False, gso_past, 1, 1025, 128, 2, 4, gseed=s1025, f64=True),
         _case("past", GO, True, gso_past, 1, 1100, 64, 4, 2, gseed=s1100),
         _case("past", KQ, True, gso_past, 2, 2048, 256, 2, 1, gseed=s2048),
         _case("past", SIM, True, gso_past, 1, 1025, 16, 2, 1, gseed=s1025, tiny=True, train=True),
         _case("past", SIM, True, gso_past, 1, 1025, 64, 3, 1, gseed=s1025, tiny=True, f64=True),
         _case("past", GNN, True, gso_past, 1, 1025, 32, 3, 1, F=64, gseed=s1025, att=False, train=True),
         _case("past", GO, False, gso_past, 1, 1025, 64, 2, 2, gseed=s1025, train=True),
         _case("limit", GNN, True, gso_limit, 1, 8190, 16, 2, 1, gseed=s8190, att=False),
         _case("limit", KQ, True, gso_limit, 1, 8190, 16, 3, 1, gseed=s8190, train=True),
         _case("limit", GO, True, gso_limit, 1, 8190, 16, 2, 1, gseed=s8190),
         # bf16 storage one agent past the fused form's reach (config 5's layer), and at 2048 agents
         _case("past", KQ, True, gso_past, 1, 1025, 128, 2, 4, gseed=s1025, bf16=True),
         _case("past", KQ, True, gso_past, 1, 2048, 64, 2, 2, gseed=s2048, bf16=True)]
    return _index(c, 6100)


LARGE = _large_cases()
CASES = dict(FORCED)
CASES.update(TILED)
CASES.update(LARGE)
# GAT_origin at 1025 agents with the mean of two heads exists for the training test alone; every other LARGE case runs inference
TRAIN_ONLY = ("past-GAT_origin-mean-past-B1N1025G64K2P2",)
LARGE_INFER = [cid for cid in LARGE if cid not in TRAIN_ONLY]
LARGE_TRAIN = [cid for cid, k in LARGE.items() if k.train]


# ---- layers, inputs, references -------------------------------------------------------------------------------------------------
def make_layer(k, state=None, **kw):
    from magat_pathplanning_amd import GraphFilterBatch, GraphFilterBatchSimilarityAttentional
    if k.mode == GNN:
        layer = GraphFilterBatch(k.G, k.F, k.K)
    elif k.mode == SIM:
        layer = GraphFilterBatchSimilarityAttentional(k.G, k.G, k.K, 1, concatenate=k.concat, **kw)
    else:
        layer = tg.gat_layer(k)
    if state is not None:
        layer.load_state_dict(state)
    return layer


def out_width(k):
    return k.F if k.mode == GNN or not k.concat else k.P * k.G


def result(k, r, dtype, grads=False):
    """The yardstick in `dtype` on the CPU: {"y", "att" (edges, P) in CSR order | None} and, with grads, "dx" and the parameters'
    gradients (None where the mode has none) of sum(y * wgt)."""
    from magat_pathplanning_amd.graphml import _composite
    layer = make_layer(k, r.state).to(dtype)
    x = r.x.to(dtype).requires_grad_(grads)
    with torch.enable_grad() if grads else torch.no_grad():
        if k.mode == GNN:       # x S^h by h, S = float(S) (graphML.py:5485-5579), as train_graph_cases.gnn_reference
            Sd = r.S.float().to(dtype)
            z, y = x, torch.einsum("bgn,fg->bfn", x, layer.weight[:, 0, 0])
            for h in range(1, k.K):
                z = torch.matmul(z, Sd)
                y = y + torch.einsum("bgn,fg->bfn", z, layer.weight[:, 0, h])
            y, att = y + layer.bias, None
        else:
            y, A = _composite(layer, x, r.S.unsqueeze(1))
            att = A.detach()[:, :, 0].permute(0, 2, 3, 1)[r.mask]
            r.off_edges = max(getattr(r, "off_edges", 0.0), float((A.detach()[:, :, 0] * ~r.mask.unsqueeze(1)).abs().max()))
            del A
        if grads:
            (y * r.wgt.to(dtype)).sum().backward()
    out = {"y": y.detach(), "att": att}
    if grads:
        out["dx"] = x.grad.detach()
        out.update({n: None if p.grad is None else p.grad.detach().clone() for n, p in layer.named_parameters()})
    return out


def attention_errors(got, want, rowid, nrows):
    """got, want (edges, P) float64 in CSR order, rowid (edges,) the row b * N + i of every edge.  Returns (largest |got - want|,
    largest |row sum of got - 1|, largest over rows and heads of max_j |got - want| / max_j want)."""
    if got.shape[0] == 0:
        return 0.0, 0.0, 0.0
    got, want = got.double().cpu(), want.double()
    d = (got - want).abs()
    idx = rowid.unsqueeze(1).expand_as(d)
    zeros = torch.zeros(nrows, d.shape[1], dtype=torch.float64)
    has = torch.zeros(nrows, dtype=torch.bool)
    has[rowid] = True
    sums = zeros.clone().scatter_add_(0, idx, got)[has]
    dmax = zeros.clone().scatter_reduce_(0, idx, d, "amax")[has]
    wmax = zeros.clone().scatter_reduce_(0, idx, want, "amax")[has]
    return float(d.max()), float((sums - 1).abs().max()), float((dmax / wmax).max())


def y_error(got, want):
    """max|got - want| / max(1, max|want|)"""
    return float((got.double().cpu() - want.double()).abs().max()) / max(1.0, float(want.abs().max()))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """reference_of the case of this file called `cid`; computed once per process."""
    return reference_of(CASES[cid])


def reference_of(k):
    """Inputs (float32 values), the edge list of the layer's rule and the float64 yardstick of a case, the float32 composite's own
    error against it and the gates that follow.  (tests/gat_csr_route_cases.py brings cases of its own.)"""
    g = tg._gen(k.seed)
    with torch.random.fork_rng(devices=[]):      # (the layers draw their initial parameters from the global generator)
        torch.manual_seed(k.seed)
        layer = make_layer(k)
    with torch.no_grad():
        if k.mode in (KQ, GM):
            layer.weight_bias.uniform_(-0.3, 0.3, generator=g)
    r = types.SimpleNamespace(case=k, state={n: v.detach().clone() for n, v in layer.state_dict().items()})
    r.x = torch.randn(k.B, k.G, k.N, generator=g) * 0.6
    if k.tiny:
        r.x[ZERO_ROW[0], :, ZERO_ROW[1]] = 0.0
        r.x[TINY_ROW[0], :, TINY_ROW[1]] *= 1e-12
    r.S = gso_of(k.gso, k.B, k.N, k.gseed, k.f64)
    r.wgt = torch.randn(k.B, out_width(k), k.N, generator=g)
    r.mask = edge_mask(r.S, k.mode)
    b, i, j = torch.nonzero(r.mask, as_tuple=True)          # row-major: the CSR order, columns ascending inside a row
    r.rowid, r.colidx, r.nnz = b * k.N + i, j, int(b.numel())
    r.rowptr = torch.zeros(k.B * k.N + 1, dtype=torch.int64)
    r.rowptr[1:] = torch.cumsum(r.mask.sum(2).reshape(-1), 0)
    r.row_deg, r.col_deg = int(r.mask.sum(2).max()), int(r.mask.sum(1).max())
    r.clamped = torch.zeros(k.B, k.N, dtype=torch.bool)
    if k.tiny:
        r.clamped[ZERO_ROW], r.clamped[TINY_ROW] = True, True
    r.want = result(k, r, torch.float64, grads=k.train)
    f32 = result(k, r, torch.float32)
    r.f32_y = y_error(f32["y"], r.want["y"])
    r.y_gate = max(Y_GATE, 4 * r.f32_y)
    r.f32_att = (0.0, 0.0, 0.0)
    if r.want["att"] is not None:
        r.f32_att = attention_errors(f32["att"], r.want["att"], r.rowid, k.B * k.N)
    r.att_gate = max(ATT_ROW, 4 * r.f32_att[2])
    if k.bf16:
        from oracle import magat_oracle as orc
        y, a = orc.gat_layer_forward_bf16_storage(r.x, r.S.unsqueeze(1), r.state, k.mode, k.concat)
        r.emul = {"y": y, "att": a[:, :, 0].permute(0, 2, 3, 1)[r.mask]}
        r.emul_off_edges = float((a[:, :, 0] * ~r.mask.unsqueeze(1)).abs().max())
    return r


def csr_rowptr(r):
    """The rowptr the device builders hand out: [B * (N + 1)] absolute offsets (every instance repeats its predecessor's end)."""
    k = r.case
    ends = r.rowptr[1:].view(k.B, k.N)
    starts = r.rowptr[:-1].view(k.B, k.N)
    return torch.cat((starts, ends[:, -1:]), dim=1).reshape(-1)
