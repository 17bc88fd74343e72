"""Inputs, the float64 yardstick and a torch restatement of the backward rule for the training path of attentionMode
'GAT_Similarity' on the HIP kernels (GraphFilterBatchSimilarityAttentional(hip_backward=True), _GatCosTrainFunction).
tests/test_host_similarity_train.py checks all of it on the CPU, tests/test_gpu_similarity_train.py runs the cases on the device.

Yardstick: graphml._composite in float64 on the CPU (tests/test_host_similarity.py pins it to reference-made gradients).
Every number handed to the device is a float32 value, and every |x_m| and |q_m| is exactly 0, at most 1e-11 or at least 1e-6, so
that float32 and float64 agree on which rows the 1e-9 clamp of the cosine touches.

The restatement (`restated_result`) is the rule the kernels implement, written with dense torch ops and no autograd:
    forward   Z = X Bt^T;  n = |v|, c = max(n, 1e-9), v^ = v / c  for v = x_m, q_m;  E_ij = x^_i . q^_j on the edges of
              |float(S) + I| > 1e-9;  A = row softmax;  T_{K-1} = U_{K-1}, T_k = U_k + A^T T_{k+1};  Ypre = T_0 + bias
    backward  dT_0 = dYpre, dT_{k+1} = A dT_k, dA_ij = sum_k T_{k+1}[i] . dT_k[j], dE = A (dA - rowsum(A dA)),
              dx^ = dE q^, dq^ = dE^T x^, then per row  dv = (1/c) (dv^ - (dv^ . v^) u),  u = v^ (c/n) if n > 0 else 0
              dX = dx + dq W + sum_k dU_k H_k,  dW = dq^T X,  dH_k = dU_k^T X,  dbias = sum dYpre
"""
import functools
import types

import torch

import train_graph_cases as tg

EPS = 1e-9
GATE = tg.GATE


def gso_no_edge_row(B, N, seed):
    """gso_rounds with, in instance 0, a node whose row is empty and whose diagonal is -1: S.float() + I cancels its self-loop, the
    row has no edge at all (others still point at it); in instance 1 the same -1 on a node that keeps its other edges."""
    S = tg.gso_rounds(B, N, seed)
    S[0, 4, :] = 0
    S[0, 4, 4] = -1.0
    S[0, 6, 4] = 0.5
    S[1, 2, 2] = -1.0
    return S


def _case(group, gso, B, N, G, K, concat=True, nin=None, clamp=False, row_deg=0, col_deg=0, distinct=False):
    return types.SimpleNamespace(group=group, gso=gso, B=B, N=N, G=G, K=K, concat=concat, nin=nin or N, clamp=clamp,
                                 row_deg=row_deg, col_deg=col_deg, distinct=distinct)


def _cases():
    c = []
    # instance index past a round of eight
    c += [_case("rounds", tg.gso_rounds, 9, 10, 32, 3, True, distinct=True),
          _case("rounds", tg.gso_rounds, 17, 10, 32, 3, False, distinct=True)]
    # rows and columns longer than two wave strides
    c += [_case("long", tg.gso_hubs, 2, 130, 64, 3, row_deg=129, col_deg=129),
          _case("long", tg.gso_full, 1, 70, 64, 3, False, row_deg=65, col_deg=65)]
    # N past one pass of the transpose
    c += [_case("wide", tg.gso_wide, 2, 300, 32, 2, col_deg=65)]
    # widths: masked lanes (16), two and four floats per lane (128, 256); N not a multiple of 4
    c += [_case("width", tg.gso_rounds, 3, 21, 16, 3), _case("width", tg.gso_rounds, 3, 21, 128, 3, False),
          _case("width", tg.gso_rounds, 3, 21, 256, 2)]
    # depth: three kept hop results, and no graph term at all
    c += [_case("depth", tg.gso_rounds, 3, 12, 32, 5), _case("depth", tg.gso_rounds, 3, 12, 32, 1, False)]
    # few edges: only self-loops, none but self-loops in the first instance, a row without any edge
    c += [_case("edgeless", tg.gso_edgeless, 2, 8, 32, 3), _case("edgeless", tg.gso_first_edgeless, 2, 8, 32, 3, False),
          _case("edgeless", gso_no_edge_row, 2, 8, 32, 3)]
    # the clamp: a zero row and a row scaled by 1e-12, both with edges and both someone's neighbour; padded inputs (zero rows)
    c += [_case("clamp", tg.gso_rounds, 3, 12, 32, 3, clamp=True), _case("clamp", tg.gso_rounds, 3, 12, 32, 3, False, nin=10)]
    out = {}
    for k in c:
        k.id = "%s-%s-%s-B%dN%dG%dK%d%s%s" % (k.group, "cat" if k.concat else "mean", k.gso.__name__[4:], k.B, k.N, k.G, k.K,
                                              "-tiny" if k.clamp else "", "-nin%d" % k.nin if k.nin != k.N else "")
        assert k.id not in out
        k.seed = 3000 + len(out)
        out[k.id] = k
    return out


CASES = _cases()
ZERO_ROW, TINY_ROW = (0, 3), (2, 7)          # (instance, agent) of the "clamp" case


def make_layer(k, state=None, hip_backward=False):
    from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional
    kw = {"hip_backward": True} if hip_backward else {}
    layer = GraphFilterBatchSimilarityAttentional(k.G, k.G, k.K, 1, concatenate=k.concat, **kw)
    if state is not None:
        layer.load_state_dict(state)
    return layer


def _grads(module):
    return {n: None if p.grad is None else p.grad.detach().clone() for n, p in module.named_parameters()}


def padded(k, x):
    return x if k.nin == k.N else torch.cat((x, torch.zeros(k.B, k.G, k.N - k.nin, dtype=x.dtype)), dim=2)


def composite_result(k, r, dtype):
    """One forward + backward of the composite in `dtype` on the CPU: {"y", "dx", parameter names (None: no gradient)}."""
    from magat_pathplanning_amd.graphml import _composite
    layer = make_layer(k, r.state).to(dtype)
    x = r.x.to(dtype).requires_grad_(True)
    y, _ = _composite(layer, padded(k, x), r.S.unsqueeze(1))
    y = y[:, :, :k.nin]
    (y * r.wgt.to(dtype)).sum().backward()
    out = {"y": y.detach(), "dx": x.grad.detach()}
    out.update(_grads(layer))
    return out


def edge_mask(S):
    """(B,N,N) bool: |float(S) + I| > 1e-9, the layer's edge rule."""
    N = S.shape[-1]
    return (S.float() + torch.eye(N)).abs() > EPS


def rows_and_maps(k, r, dtype=torch.float64):
    """X (B,N,G) rows (padded) and Q = X W^T in `dtype`."""
    X = padded(k, r.x.to(dtype)).transpose(1, 2)
    return X, X @ r.state["weight"][0, 0].to(dtype).t()


def norm_backward(dvh, vh, n):
    """dv = (1/c) (dv^ - (dv^ . v^) u),  u = v^ (c/n) if n > 0 else 0;  rows on the last axis, n (...,)."""
    c = n.clamp_min(EPS)
    s = torch.where(n > 0, c / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
    dot = (dvh * vh).sum(-1, keepdim=True)
    return (dvh - dot * vh * s.unsqueeze(-1)) / c.unsqueeze(-1)


def restated_result(k, r, dtype=torch.float64):
    """The rule of the module docstring in `dtype`, no autograd: the same keys as composite_result (mixer, weight_bias: None)."""
    W = r.state["weight"][0, 0].to(dtype)                       # (G,G): q = W x
    H = r.state["filterWeight"][0, :, 0].to(dtype)              # (F,K,G)
    bias = r.state["bias"].to(dtype).view(-1)
    K = k.K
    X, Q = rows_and_maps(k, r, dtype)
    nx, nq = X.norm(dim=2), Q.norm(dim=2)
    xh, qh = X / nx.clamp_min(EPS).unsqueeze(2), Q / nq.clamp_min(EPS).unsqueeze(2)
    M = edge_mask(r.S)
    E = torch.einsum("big,bjg->bij", xh, qh).masked_fill(~M, float("-inf"))
    A = torch.nan_to_num(torch.softmax(E, dim=2), nan=0.0) * M  # (a row without edges: zeros)
    U = [X @ H[:, h].t() for h in range(K)]
    T = [None] * K
    T[K - 1] = U[K - 1]
    for h in range(K - 2, -1, -1):
        T[h] = U[h] + A.transpose(1, 2) @ T[h + 1]
    ypre = T[0] + bias
    y = torch.relu(ypre).transpose(1, 2)[:, :, :k.nin]
    dy = padded(k, r.wgt.to(dtype)).transpose(1, 2)
    if k.nin != k.N:
        dy = dy.clone()
        dy[:, k.nin:] = 0
    dT = [dy * (ypre > 0)]
    dA = torch.zeros_like(A)
    for h in range(K - 1):
        dA = dA + torch.einsum("big,bjg->bij", T[h + 1], dT[h])
        dT.append(A @ dT[h])
    dE = A * (dA - (A * dA).sum(2, keepdim=True))
    dx = norm_backward(dE @ qh, xh, nx)
    dq = norm_backward(dE.transpose(1, 2) @ xh, qh, nq)
    dX = dx + dq @ W + sum(dT[h] @ H[:, h] for h in range(K))
    dH = torch.stack([torch.einsum("bnf,bng->fg", dT[h], X) for h in range(K)], dim=1)
    out = {"y": y, "dx": dX.transpose(1, 2)[:, :, :k.nin], "mixer": None, "weight_bias": None,
           "weight": torch.einsum("bnf,bng->fg", dq, X).view(1, 1, k.G, k.G), "filterWeight": dH.view(1, k.G, 1, K, k.G),
           "bias": dT[0].sum(dim=(0, 1)).view(-1, 1)}
    return out


def clamped_rows(k, r):
    """(B, nin) bool: agents whose |x| or |W x| lies under the clamp (their dx is of the order 1e9)."""
    X, Q = rows_and_maps(k, r)
    return ((X.norm(dim=2) < EPS) | (Q.norm(dim=2) < EPS))[:, :k.nin]


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Inputs (float32 values) and the float64 composite's y, dx and parameter gradients of a case; computed once per process."""
    k = CASES[cid]
    g = torch.Generator().manual_seed(k.seed)
    with torch.random.fork_rng(devices=[]):      # (the layer draws its initial parameters from the global generator)
        torch.manual_seed(k.seed)
        layer = make_layer(k)
    r = types.SimpleNamespace(case=k, state={n: v.detach().clone() for n, v in layer.state_dict().items()})
    r.x = torch.randn(k.B, k.G, k.nin, generator=g) * 0.6
    if k.clamp:
        r.x[ZERO_ROW[0], :, ZERO_ROW[1]] = 0.0
        r.x[TINY_ROW[0], :, TINY_ROW[1]] *= 1e-12
    r.S = k.gso(k.B, k.N, k.seed).float().double()
    r.wgt = torch.randn(k.B, k.G, k.nin, generator=g)
    r.row_deg, r.col_deg = tg.degrees(r.S, tg.GO)
    r.clamped = clamped_rows(k, r)
    r.want = composite_result(k, r, torch.float64)
    return r


def compare(cid, got, want, clamped, gate=GATE, again=None, show=True):
    """got within gate * max(1, max|want|) of want, tensor by tensor; the clamped rows of dx apart, at gate * their own max|want|;
    a parameter without gradient in `want`: None or zeros.  With `again`: got == again bit for bit.  Returns the worst error
    over all tensors, each relative to its scale."""
    worst, fails = {}, []
    for name, b in want.items():
        a = got[name]
        if again is not None:
            a2 = again[name]
            assert (a is None) == (a2 is None) and (a is None or torch.equal(a, a2)), (cid, name, "differs from run to run")
        if b is None or not b.any():
            assert a is None or not a.any(), (cid, name, "the reference has no gradient here")
            continue
        assert a is not None and a.shape == b.shape, (cid, name)
        a, b = a.detach().cpu().double(), b.double()
        parts = [(name, a, b, max(1.0, float(b.abs().max())))]
        if name == "dx" and clamped.any():
            keep = (~clamped).unsqueeze(1).expand_as(b)
            bo, bc = b[keep], b[~keep]
            parts = [(name, a[keep], bo, max(1.0, float(bo.abs().max()))),
                     (name + "[clamped rows]", a[~keep], bc, float(bc.abs().max()))]
        for label, aa, bb, scale in parts:
            err = float((aa - bb).abs().max()) / scale if scale > 0 else float((aa - bb).abs().max())
            worst[label] = err
            if not err <= gate:
                fails.append((label, err))
    if show:
        print("%s: worst error / scale: %s" % (cid, "  ".join("%s %.2e" % kv for kv in worst.items())))
    assert not fails, (cid, fails)
    return max(worst.values())
