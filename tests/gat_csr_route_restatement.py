"""What one call of the CSR graph layer does, restated in Python from the dispatcher as it stood BEFORE csrc/gat_csr_route.h
existed (csr_forward, train_forward, ws_layout, csr_tiled_ok, csr_fused_form of csrc/gat_csr_f32.hip; magat_gat_csr_fused_supported
and the grids of magat_gat_csr_fused_forward in csrc/gat_csr_fused.hip): refusals in the order the entries answered them, the
form, the launches and their grids, the workspace layout.  tests/test_host_gat_csr_route.py holds the header against it on the
CPU, tests/test_gpu_gat_csr_routes.py predicts launch counts from it.  Nothing here is derived from the header."""
from gat_route_restatement import pack_columns, supported_width

KQ, GAT_MODIFIED, GAT_ORIGIN, GNN, SIMILARITY = 0, 1, 2, 3, 4
PASSES = ("infer", "train", "train_cos")
REFUSALS = ("none", "dims", "mode", "cosine", "gnn", "shape", "agents", "ldy", "xalign", "grid", "bf16_maps")
OK, BAD_SHAPE, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3        # MAGAT_OK, MAGAT_ERR_* of include/magat_hip.h
CODES = dict(none=OK, dims=BAD_SHAPE, mode=UNSUPPORTED, cosine=UNSUPPORTED, gnn=BAD_SHAPE, shape=UNSUPPORTED, agents=UNSUPPORTED,
             ldy=BAD_SHAPE, xalign=UNSUPPORTED, grid=BAD_SHAPE, bf16_maps=UNSUPPORTED)
MAPS = ("none", "auto", "f32", "bf16")
GRAPHS = ("none", "edge", "tiled")
K1S = ("none", "alone", "after_scores")
DEFAULT_OPT = dict(CSR_TILED=3, CSR_FUSED=1)
MAX_N, XCD, INT_MAX = 8190, 8, 0x7fffffff
WS_ORDER = ("status", "z", "cscptr", "cscsrc", "cscpos", "csctmp", "att", "t0", "t1", "ytmp", "order", "xhat", "total")
GRIDS = ("grid_transpose", "grid_sort", "grid_scores", "grid_k1", "grid_hop", "grid_mean", "grid_fused_rank", "grid_fused_scores",
         "grid_fused_hop")


def _rounds(B):
    return (B + XCD - 1) // XCD * XCD


def fused_form(i):
    """csr_fused_form: bf16 storage, the column view brought, and magat_gat_csr_fused_supported"""
    return bool(i["esz"] == 2 and i["have_csc"] and i["opt"]["CSR_FUSED"] and i["mode"] == KQ and i["K"] == 2 and i["G"] == 128
                and i["F"] == 128 and i["concat"] and i["P"] in (1, 2, 4))


def workspace(i, fused):
    """ws_layout: every piece rounded up to 256 bytes"""
    B, N, nnz, G, F, K, P, esz = i["B"], i["N"], i["nnz"], i["G"], i["F"], i["K"], i["P"], i["esz"]
    sizes = dict(status=256, z=0 if fused else B * N * pack_columns(G, F, K, P, i["mode"]) * esz)
    own = not i["have_csc"]
    sizes.update(cscptr=B * (N + 1) * 4 * own, cscsrc=nnz * 4 * own, cscpos=nnz * 4 * own, csctmp=nnz * 4 * own, att=P * nnz * 4)
    tb = B * N * P * F * esz
    sizes.update(t0=tb if K > 2 else 0, t1=tb if K > 3 else 0, ytmp=0 if i["concat"] else tb, order=2 * B * N * 4 if fused else 0,
                 xhat=B * N * G * 4 if i["mode"] == SIMILARITY else 0)
    w, o = {}, 0
    for name in WS_ORDER[:-1]:
        w[name] = o
        o += (sizes[name] + 255) // 256 * 256
    w["total"] = o
    return w


def workspace_bytes(B, N, nnz, G, F, K, P, mode, concat, esz, have_csc, opt=DEFAULT_OPT):
    """the three *_workspace_bytes exports"""
    if B <= 0 or N <= 0 or nnz < 0 or G <= 0 or F <= 0 or K <= 0 or P <= 0:
        return 0
    i = dict(B=B, N=N, nnz=nnz, G=G, F=F, K=K, P=P, mode=mode, concat=concat, esz=esz, have_csc=have_csc, opt=opt)
    return workspace(i, fused_form(i))["total"]


def tiled_ok(i, width, which):
    return bool(i["opt"]["CSR_TILED"] & which) and 8 <= i["N"] <= 1024 and (width * i["esz"]) % 128 == 0


def _edge_grids(i):
    lanes = min(i["G"] // 4, 8)
    rows = 256 // lanes
    return _rounds(i["B"]) * i["P"] * ((i["N"] + rows - 1) // rows), _rounds(i["B"]) * i["P"] * ((i["N"] + 3) // 4)


def _blank():
    r = dict(refusal="none", fused=False, maps="none", prepare=False, cos_train_note=False, transpose=False, transpose_booked=False,
             scores="none", k1="none", hops=0, hop_kind="none", hop_buffers=0, head_mean=False, act_relu=0)
    r.update({g: 0 for g in GRIDS})
    return r


def route(i):
    """-> dict; with a refusal before the workspace check only {"refusal"}; "bf16_maps" comes with the whole route, since the
    workspace check stands in front of it"""
    return _train(i) if i["pass"] != "infer" else _infer(i)


def _train(i):
    """train_forward (magat_gat_train_forward_f32, magat_gat_train_forward_cos_f32)"""
    B, N, G, F, K, P, mode = i["B"], i["N"], i["G"], i["F"], i["K"], i["P"], i["mode"]
    if B <= 0 or N <= 0 or i["nnz"] < 0 or K <= 0 or P <= 0:
        return dict(refusal="dims")
    if mode < KQ or mode > GAT_ORIGIN:
        return dict(refusal="mode")
    if G != F or not supported_width(G):
        return dict(refusal="shape")
    if N > MAX_N:
        return dict(refusal="agents")
    scores, hop = _edge_grids(i)
    if B * N > INT_MAX or hop > INT_MAX:
        return dict(refusal="grid")
    r = _blank()
    cos = i["pass"] == "train_cos"
    r.update(maps="f32", prepare=cos, cos_train_note=cos, transpose=True, scores="edge", grid_transpose=B, grid_sort=(B * N + 3) // 4,
             grid_scores=scores, NC=pack_columns(G, F, K, P, mode), ws={k: 0 for k in WS_ORDER})
    if K == 1:
        r.update(k1="after_scores", grid_k1=2048)
    else:
        r.update(hops=K - 1, hop_kind="edge", grid_hop=hop)
    return r


def _infer(i):
    """csr_forward behind the six forward entry points"""
    B, N, G, F, K, P, mode, concat = i["B"], i["N"], i["G"], i["F"], i["K"], i["P"], i["mode"], i["concat"]
    if B <= 0 or N <= 0 or i["nnz"] < 0 or G <= 0 or F <= 0 or K <= 0 or P <= 0:
        return dict(refusal="dims")
    if mode < KQ or mode > SIMILARITY:
        return dict(refusal="mode")
    gnn, cosine = mode == GNN, mode == SIMILARITY
    if cosine and (i["esz"] != 4 or P != 1 or G != F):
        return dict(refusal="cosine")
    if gnn and (P != 1 or (i["nnz"] > 0 and K > 1 and not i["edge_vals"]) or G % 4):
        return dict(refusal="gnn")
    if (not gnn and G != F) or not supported_width(F):
        return dict(refusal="shape")
    if N > MAX_N:
        return dict(refusal="agents")
    if i["ldy"] < (P * F if concat else F) or i["ldy"] % 4:
        return dict(refusal="ldy")
    if not i["x_aligned"]:
        return dict(refusal="xalign")
    r = _blank()
    r["fused"] = fused_form(i)
    r["ws"] = workspace(i, r["fused"])
    r["NC"] = pack_columns(G, F, K, P, mode)
    if r["fused"]:
        per_xcd = max(1, i["cus"] // XCD)
        nchunk = ((N + 31) // 32 + 7) // 8
        items = _rounds(B) // XCD * nchunk
        ngrp = P // (2 if P >= 2 else 1)
        r.update(act_relu=1, grid_fused_rank=B, grid_fused_scores=XCD * min(items, per_xcd),
                 grid_fused_hop=XCD * ngrp * min(items, max(1, per_xcd // ngrp)))
        return r
    r["maps"] = "f32" if cosine else "bf16" if i["esz"] == 2 else "auto"
    if r["maps"] == "bf16" and (r["NC"] % 32 or G % 32):
        r["refusal"] = "bf16_maps"
    r.update(prepare=cosine, act_relu=0 if gnn else int(bool(concat)), head_mean=not concat,
             hop_buffers=2 if K > 3 else 1 if K > 2 else 0)
    scores, hop = _edge_grids(i)
    tiled = _rounds(B) * P
    if K == 1 and (not i["attention"] or gnn):
        r.update(k1="alone", grid_k1=2048)
    else:
        if K > 1 and not i["have_csc"]:
            r.update(transpose=True, transpose_booked=True, grid_transpose=B, grid_sort=(B * N + 3) // 4)
        if not gnn:
            t = mode == KQ and tiled_ok(i, G, 1)
            r.update(scores="tiled" if t else "edge", grid_scores=tiled if t else scores)
        if K == 1:
            r.update(k1="after_scores", grid_k1=2048)
        else:
            t = not cosine and tiled_ok(i, F, 2)
            r.update(hops=K - 1, hop_kind="tiled" if t else "edge", grid_hop=tiled if t else hop)
    if not concat:
        r["grid_mean"] = min(4096, (B * N * (F // 4) + 255) // 256)
    return r


def return_code(r, workspace_ok=True):
    """what the entry answers: the refusal's code; the workspace check stands in front of "bf16_maps" only.  (A grid beyond an int
    is refused by the inference entries where they would launch it, behind earlier launches: not restated.)"""
    if r["refusal"] not in ("none", "bf16_maps"):
        return CODES[r["refusal"]]
    return WORKSPACE if not workspace_ok else CODES[r["refusal"]]


def launches(r, split_guard=True):
    """-> ({profiling tag: launches}, {form counter: notes}) of an admitted route.  split_guard: the float32 maps of the inference
    entries take the guarded split GEMM (options GAT_SPLIT, RANGE_GUARD at their defaults and NC, G multiples of 32), whose
    predicated re-run and bookkeeping kernel run under MAGAT_TAG_RANGE_GUARD."""
    tags = dict(GSO_CSR=0, GAT_MAPS=0, GAT_PREPARE=0, GAT_GRAPH=0, HEAD_MEAN=0, GAT_CAST=0)
    forms = dict(CSR_FUSED=0, GAT_COS_TRAIN=int(r["cos_train_note"]))
    if r["fused"]:
        tags["GAT_GRAPH"], forms["CSR_FUSED"] = 3, 1       # csr_rank_kernel, scores, hop
        return tags, forms
    tags["GAT_MAPS"] = 1
    tags["GAT_PREPARE"] = int(r["prepare"])
    tags["GSO_CSR"] = 1 if r["transpose_booked"] else 0     # (one span around both kernels)
    tags["GAT_GRAPH"] = int(r["scores"] != "none") + r["hops"]       # (csr_k1_kernel runs untagged)
    tags["HEAD_MEAN"] = int(r["head_mean"])
    return tags, forms
