"""Which launches a call of the dense graph layer takes, restated in Python from the dispatcher as it stood before csrc/gat_route.h
existed (gat_forward_impl in gat_f32.hip, the *_supported predicates and the launchers of gat_mfma.hip / gat_small.hip /
gat_mid.hip, magat_gat_maps_gemm): the predicates first, then the dispatcher top to bottom.  tests/test_host_gat_route.py holds the
header against it on the CPU, tests/test_gpu_gat_routes.py the library's launch counts and form counters on the GPU."""
KEYQUERY, GAT_MODIFIED, GAT_ORIGIN, GNN, SIMILARITY = range(5)
DEFAULT_OPT = dict(GAT_MFMA=1, GAT_SPLIT=1, RANGE_GUARD=1, GAT_WIDE_FROM=103, GAT_PACK=1, GAT_CHUNK_MB=2048)
REFUSALS = ("none", "dims", "mode", "shape", "tiles")
FORMS = ("one_mfma", "one_small", "one_mid", "two_launch")
GUARDS = ("none", "one", "one_tail", "two", "slim")
MAPS = ("none", "split", "split_guard", "f32")
BOOKS = ("none", "maps", "one", "graph", "mean")
LDS = 160 * 1024
ONE_LAUNCH, T_MAPS, T_GRAPH, T_PREPARE, T_MEAN, T_GUARD = ("gat_layer (one launch)", "gat_maps_gemm", "gat_graph", "gat_prepare",
                                                           "head_mean", "range_guard")
COUNTERS = ("gat_pack", "gat_hsplit", "gat_persist", "gat_mid", "actions_tail")


def supported_width(w):
    return w in (16, 32, 64, 128, 256)


def dense_lds(N, G, F, nwaves):
    rw, lda = max(G, F), N | 1
    return 4 * (2 * N * rw + N * lda + 2 * ((N + 3) & ~3)) + 4 * 128 * nwaves + 4 * 4 * N + 16


def block_threads(N):
    return 128 if N <= 16 else 256 if N <= 32 else 512 if N <= 64 else 1024


def mfma_lds(N, ksi):
    sa, r8 = 2 * 16 * ksi + 16, (N + 7) & ~7
    return 2 * N * 256 + 2 * r8 * sa + 2 * 128 * sa


def mfma_class(N):
    if N <= 0:
        return -1
    c = 0 if N <= 32 else 1 if N <= 64 else 2
    ksi = (2, 4, 7)[c]
    return c if N <= 16 * ksi and mfma_lds(N, ksi) <= LDS else -1


def mfma_supported(N, G, F, K, mode):
    if mode < KEYQUERY or mode > GAT_ORIGIN or G != 128 or F != 128 or K not in (2, 3):
        return False
    return mfma_class(N) >= 0


def small_supported(N, G, F, K, mode):
    return mode in (KEYQUERY, SIMILARITY) and 1 <= N <= 32 and G == F and G in (32, 64) and K in (2, 3)


def mid_supported(N, G, F, K, mode, opt):
    if mode not in (KEYQUERY, SIMILARITY) or G != F or K not in (2, 3) or N > 128:
        return False
    if G == 128 and mode == SIMILARITY:
        return 97 <= N <= 105
    if G == 128:
        return N >= max(103, opt["GAT_WIDE_FROM"])
    return N >= 33 and G in (32, 64)


def one_launch(N, G, F, K, mode, opt):
    if mode == SIMILARITY:
        return bool(opt["GAT_MFMA"] and opt["GAT_SPLIT"] and opt["RANGE_GUARD"] != 0 and
                    (small_supported(N, G, F, K, mode) or mid_supported(N, G, F, K, mode, opt)))
    return bool(opt["GAT_MFMA"] and opt["GAT_SPLIT"] and
                (mfma_supported(N, G, F, K, mode) or small_supported(N, G, F, K, mode) or mid_supported(N, G, F, K, mode, opt)))


def one_launch_supported(N, G, F, K, mode, opt):
    """magat_gat_one_launch_supported"""
    if N <= 0 or G != F or not supported_width(G) or N > 128:
        return False
    return one_launch(N, G, F, K, mode, opt)


def dense_supported(N, G, F):
    """magat_gat_dense_supported"""
    if N <= 0 or N > 128 or G != F or not supported_width(G):
        return False
    return dense_lds(N, G, F, block_threads(N) // 64) <= LDS


def pack_columns(G, F, K, P, mode):
    if mode in (KEYQUERY, SIMILARITY):
        return P * G + P * K * F
    if mode == GNN:
        return (P * K * F + 31) & ~31
    c2off = P * K * F + P
    return (c2off + P + 31) & ~31


def chunk_instances(B, N, ldz, mb):
    per = N * ldz * 4
    return min(max(int(mb * 1048576.0) // max(per, 1), 8), B)


def route(i):
    """i: B N G F K P mode concat attention y_aligned tail tail_cout tail_m tail_k opt conv_direct cus -> dict of the decisions"""
    B, N, G, F, K, P, mode, concat, opt, cus = (i[k] for k in ("B", "N", "G", "F", "K", "P", "mode", "concat", "opt", "cus"))
    if min(B, N, G, F, K, P) <= 0:
        return dict(refusal="dims")
    cosine = mode == SIMILARITY
    if (mode < KEYQUERY or mode > GAT_ORIGIN) and not cosine:
        return dict(refusal="mode")
    if G != F or not supported_width(G) or N > 128 or (cosine and P != 1):
        return dict(refusal="shape")
    threads = block_threads(N)
    lds = dense_lds(N, G, F, threads // 64)
    slim = lds > LDS
    one_ok = not i["attention"] and one_launch(N, G, F, K, mode, opt) and i["y_aligned"]
    if slim and cosine:
        return dict(refusal="tiles")
    if slim and not (G == 128 and F == 128 and mode == KEYQUERY and one_ok):
        return dict(refusal="tiles")
    NC = pack_columns(G, F, K, P, mode)
    ldz = NC + 32
    chunk = chunk_instances(B, N, ldz, opt["GAT_CHUNK_MB"])
    r = dict(refusal="none", form="two_launch", cls=0, pack=False, hsplit=False, persist=False, grid=0, guard="none", rerun_grid=0,
             maps="none", prepare=False, slim=slim, ztiles=False, all_fused=False, head_mean=False, book="none", NC=NC, ldz=ldz,
             chunk=chunk, nchunks=(B + chunk - 1) // chunk, threads=threads, lds=lds)
    rerun_only = False
    if one_ok:
        guard = opt["RANGE_GUARD"] != 0
        if G == 128 and mfma_supported(N, G, F, K, mode):
            r["form"], r["cls"] = "one_mfma", mfma_class(N)
            pack = opt["GAT_PACK"]
            if r["cls"] == 0 and pack and (pack >= 2 or B >= 2 * cus):       # launch_class -> launch_pack
                r["pack"], r["grid"] = True, min((B + 3) // 4, cus)
            else:                                                            # launch
                unsplit = ((B + cus - 1) // cus) * (12 + 36 * P)
                split = ((B * P + cus - 1) // cus) * (12 + 36)
                ypre = not concat                                            # (the caller's scratch rows: always there for head mean)
                hs = (bool(concat) or ypre) and P > 1 and split < unsplit
                units = B * P if hs else B
                r["hsplit"], r["grid"] = hs, min(units, cus * (P if hs else 1))
                r["persist"] = units > r["grid"]
        elif G != 128 and N <= 32:
            r["form"] = "one_small"
        else:
            r["form"] = "one_mid"
            r["hsplit"] = not cosine and P > 1 and B * P <= 64
        if not guard:
            return r
        rerun_only = True
        if mode == KEYQUERY and G in (32, 64, 128) and B * P <= 64:
            with_tail = bool(i["tail"]) and i["tail_cout"] == 5 and i["tail_m"] == B * N and i["tail_k"] * 5 * 4 <= 64 * 1024
            r["guard"], r["book"] = ("one_tail" if with_tail else "one"), "one"
            r["rerun_grid"] = max((B * N + 15) // 16, B) if with_tail else B
            return r
        r["guard"] = "slim" if slim else "two"

    def hpb_for(cb):
        return P if G >= 64 and P > 1 and lds > 80 * 1024 and cb >= 256 else 1
    cbs = [min(chunk, B - b0) for b0 in range(0, B, chunk)]
    r["all_fused"] = (not concat) and G >= 64 and not slim and all(hpb_for(cb) == P for cb in cbs)
    r["ztiles"] = G == 128 and F == 128 and NC % 128 == 0 and bool(i["conv_direct"]) and bool(opt["GAT_SPLIT"])
    if rerun_only or cosine or not (opt["GAT_SPLIT"] and NC % 32 == 0 and G % 32 == 0):
        r["maps"] = "f32"
    else:
        r["maps"] = "split_guard" if opt["RANGE_GUARD"] != 0 else "split"
    r["prepare"] = cosine
    r["head_mean"] = (not concat) and not r["all_fused"]
    if rerun_only:
        r["book"] = "graph" if (concat or r["all_fused"]) else "mean"
    elif r["maps"] == "split_guard":
        r["book"] = "maps"

    def per_chunk(cb):
        hpb = hpb_for(cb)
        slots = (cb + 7) // 8 * 8
        if hpb == P and hpb > 1 and slots > 256:
            slots = 256
        if rerun_only and slots > 128:
            slots = 128
        blocks = min(cb * P, 128) if slim else slots * (P // hpb)
        return (cb, hpb, slots, blocks, cb * N * 128 if r["ztiles"] else 0)
    r["first"], r["last"] = per_chunk(cbs[0]), per_chunk(cbs[-1])
    return r


def launches(r):
    """-> ({profiling tag: launches}, {form counter: count}) of an admitted call whose input does not clamp or does: the predicated
    launches are counted either way."""
    tags = {t: 0 for t in (ONE_LAUNCH, T_MAPS, T_GRAPH, T_PREPARE, T_MEAN, T_GUARD)}
    forms = {c: 0 for c in COUNTERS}
    if r["form"] != "two_launch":
        tags[ONE_LAUNCH] = 1
        forms["gat_pack"] = int(r["pack"])
        forms["gat_hsplit"] = int(r["hsplit"])
        forms["gat_persist"] = int(r["persist"])
        forms["gat_mid"] = int(r["form"] == "one_mid")
    if r["guard"] in ("one", "one_tail"):
        tags[T_GUARD] = 1
        forms["actions_tail"] = int(r["guard"] == "one_tail")
    elif r["guard"] in ("two", "slim"):       # per chunk: maps, (prepare,) graph; then the head mean - all under the guard's tag
        tags[T_GUARD] = r["nchunks"] * (2 + int(r["prepare"])) + int(r["head_mean"])
    elif r["form"] == "two_launch":
        tags[T_MAPS] = tags[T_GRAPH] = r["nchunks"]
        tags[T_PREPARE] = r["nchunks"] * int(r["prepare"])
        tags[T_MEAN] = int(r["head_mean"])
        tags[T_GUARD] = r["nchunks"] * int(r["maps"] == "split_guard")
    return tags, forms
