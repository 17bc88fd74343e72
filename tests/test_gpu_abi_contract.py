"""The graph layer's C ABI (include/magat_hip.h, "Alignment") at the placements a foreign binding hands it: X at every 4-byte
offset inside a larger allocation (bf16: every 2-byte offset), Y as its own buffer, as a column block at column 0 of wider rows
and as a column block at an odd column offset.  Each call is held against the float64 oracle, the bytes of the Y allocation
outside the result block must keep the NaN poison written before the call (a 16-byte store that spills past a column block),
and a placement the header refuses must come back as the stated code with nothing launched.  Shapes reach every dense form
(gat_mfma, gat_small with instance packing, gat_mid, the two-launch form) and the CSR / CSC / bf16 / GNN entries."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED = 0, -2
MODES = {"KeyQuery": 0, "GAT_modified": 1, "GAT_origin": 2}
POISON = 0x7FC0DEAD                   # a quiet NaN no kernel computes
ONE, MAPS, GRAPH = "gat_layer (one launch)", "gat_maps_gemm", "gat_graph"
PLACES = ("own", "col0", "odd")


def _layer(G, K, P, mode, concat, seed):
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    torch.manual_seed(seed)
    if mode == "GAT_origin":      # (its own class: no weight_bias, scalar taps filterWeight (E, K), self loops in the mask)
        layer = GraphFilterBatchAttentional_Origin(G, G, K, P, concatenate=concat)
    else:
        layer = GraphFilterBatchAttentional(G, G, K, P, attentionMode=mode, concatenate=concat)
    with torch.no_grad():
        layer.bias.uniform_(-0.1, 0.1)
    return {k: v.detach().clone() for k, v in layer.state_dict().items()}


def _inputs(B, N, G, s64, seed):
    from magat_pathplanning_amd.synthetic import directed_gso
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, G, N, generator=g) * 0.7
    S = torch.nan_to_num(directed_gso(B, N, min(1.0, 8.0 / N), seed=seed, dtype=torch.float64 if s64 else torch.float32))
    if N > 3:
        S[0, 2, :] = 0                # an agent without out-edges
    return x, S


def _oracle(x, S, p, mode, concat):
    from oracle import magat_oracle as orc
    pd = {k: v.double() for k, v in p.items()}
    y, _ = orc.gat_layer_forward(x.double(), S.double().unsqueeze(1), pd, mode, concat)
    return y.permute(0, 2, 1).reshape(-1, y.shape[1])            # (B*N, width) rows


def _pack(p, G, K, P, mode, dev):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    t = {k: v.to(dev).contiguous() for k, v in p.items()}
    packed = torch.empty(lib.magat_gat_packed_floats(G, G, K, P, mode), dtype=torch.float32, device=dev)
    wb = t.get("weight_bias")
    mixer = t.get("mixer")
    rc = lib.magat_gat_pack_weights(t["weight"].data_ptr(), None if wb is None else wb.data_ptr(),
                                    None if mixer is None else mixer.data_ptr(), t["filterWeight"].data_ptr(), packed.data_ptr(),
                                    G, G, K, P, mode, torch.cuda.current_stream().cuda_stream)
    assert rc == OK
    return packed, t["bias"].reshape(-1).contiguous(), t


def _x_at(rows, off, dev, dtype=torch.float32):
    """rows (M, G) placed `off` elements into a larger allocation (the allocation itself is 256-byte aligned)"""
    base = torch.zeros(rows.numel() + 16, dtype=dtype, device=dev)
    X = base[off:off + rows.numel()].view(rows.shape)
    X.copy_(rows.to(dev, dtype))
    return base, X


def _y_at(M, width, place, dev, dtype=torch.float32):
    """(allocation, pointer of the block, ldy, column offset); the allocation holds the poison pattern"""
    ld = {"own": width, "col0": width + 8, "odd": width + 12}[place]
    col = 1 if place == "odd" else 0
    itype = torch.int32 if dtype == torch.float32 else torch.int16
    pat = POISON if dtype == torch.float32 else 0x7FCD
    buf = torch.full((M + 1, ld), pat, dtype=itype, device=dev)       # (one spare row below the block)
    esz = 4 if dtype == torch.float32 else 2
    return buf, buf.data_ptr() + col * esz, ld, col


def _block(buf, M, width, col, dtype=torch.float32):
    return buf[:M, col:col + width].contiguous().view(dtype).float().cpu()


def _poison_intact(buf, M, width, col, dtype=torch.float32):
    pat = POISON if dtype == torch.float32 else 0x7FCD
    b = buf.cpu().clone()
    b[:M, col:col + width] = pat
    return bool((b == pat).all())


def _run(fn, tc_factory):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    lib.magat_form_reset()
    with tc_factory() as tc:
        rc = fn()
    return rc, dict(tc.counts), int(lib.magat_form_count(nat.FORMS["gat_mid"]))


# (G, N, mode, K, P, concat, s64, B): every dense form, all three attention modes, both merges, K 1 .. 3, P 1 | 4, both GSO types
DENSE = [(128, 1, "KeyQuery", 2, 4, True, False, 3), (128, 10, "GAT_modified", 3, 1, False, True, 3),
         (128, 102, "GAT_modified", 2, 4, True, False, 2), (128, 103, "KeyQuery", 2, 4, False, True, 2),
         (128, 104, "KeyQuery", 3, 1, True, False, 2), (128, 105, "KeyQuery", 2, 4, True, True, 2),
         (128, 106, "KeyQuery", 3, 4, True, False, 2), (128, 128, "KeyQuery", 2, 1, False, True, 2),
         (32, 7, "KeyQuery", 2, 4, True, False, 40), (64, 32, "KeyQuery", 3, 1, False, True, 40),
         (32, 33, "KeyQuery", 3, 4, False, False, 3), (64, 100, "KeyQuery", 2, 4, True, True, 3),
         (32, 128, "KeyQuery", 2, 1, True, False, 2), (16, 20, "GAT_modified", 1, 4, True, False, 3),
         (256, 12, "KeyQuery", 3, 1, False, True, 3), (64, 50, "GAT_modified", 1, 1, False, False, 3),
         (128, 20, "GAT_origin", 3, 4, True, False, 3), (32, 12, "GAT_origin", 2, 1, False, True, 3)]


def _dense_expect(lib, G, N, K, mode, concat, xoff, place):
    """(rc, form) the header states: form 'one' / 'mid' / 'two'"""
    if xoff:
        return UNSUPPORTED, None
    # (tests/gat_route_restatement.py: the dispatcher restated; the form does not depend on the batch or the head count)
    import gat_route_restatement as rr
    r = rr.route(dict(B=1, N=N, G=G, F=G, K=K, P=1, mode=mode, concat=1 if concat else 0, attention=False, y_aligned=place != "odd",
                      tail=False, tail_cout=0, tail_m=0, tail_k=0, opt=rr.DEFAULT_OPT, conv_direct=True, cus=256))
    one = bool(lib.magat_gat_one_launch_supported(N, G, G, K, mode, 1 if concat else 0)) and place != "odd"
    assert one == (r.get("form", "two_launch") != "two_launch")
    assert bool(lib.magat_gat_dense_supported(N, G, G)) == rr.dense_supported(N, G, G)
    if r["refusal"] != "none":       # beyond the two-launch tiles: only the one-launch gat_mid form
        return UNSUPPORTED, None
    return OK, {"two_launch": "two", "one_mid": "mid"}.get(r["form"], "one")


@pytest.mark.parametrize("G,N,mode,K,P,concat,s64,B", DENSE,
                         ids=["G%d_N%d_%s_K%d_P%d_%s_%s" % (c[0], c[1], c[2], c[3], c[4], "cat" if c[5] else "mean",
                                                          "S64" if c[6] else "S32") for c in DENSE])
def test_dense_entries_under_every_placement(gpu_device, tag_counts, G, N, mode, K, P, concat, s64, B):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    dev = gpu_device
    md = MODES[mode]
    width = P * G if concat else G
    M = B * N
    x, S = _inputs(B, N, G, s64, seed=G + N + K)
    p = _layer(G, K, P, mode, concat, seed=N + P)
    ref = _oracle(x, S, p, mode, concat)
    scale = max(1.0, float(ref.abs().max()))
    packed, bias, _ = _pack(p, G, K, P, md, dev)
    Sd = S.to(dev).contiguous()
    ws = torch.zeros(lib.magat_gat_workspace_bytes(B, N, G, G, K, P, md, 1 if concat else 0), dtype=torch.uint8, device=dev)
    rows = x.permute(0, 2, 1).reshape(M, G)
    stream = torch.cuda.current_stream().cuda_stream
    base = None
    for entry in ("packed", "tail"):
        for place in PLACES:
            for xoff in (0, 1, 2, 3):
                if entry == "tail" and xoff not in (0, 1):
                    continue
                xb, X = _x_at(rows, xoff, dev)
                yb, yp, ldy, col = _y_at(M, width, place, dev)
                args = (X.data_ptr(), Sd.data_ptr(), 1 if s64 else 0, packed.data_ptr(), bias.data_ptr(), yp, ldy)
                tail_args = (ws.data_ptr(), ws.numel(), B, N, G, G, K, P, md, 1 if concat else 0)
                if entry == "packed":
                    fn = lambda: lib.magat_gat_forward_packed_f32(*args, None, *tail_args, stream)
                else:
                    done = ctypes.c_int(7)
                    fn = lambda: lib.magat_gat_forward_tail_f32(*args, *tail_args, None, ctypes.byref(done), stream)
                rc, tc, mid = _run(fn, tag_counts)
                want_rc, form = _dense_expect(lib, G, N, K, md, concat, xoff, place)
                what = (entry, place, xoff, rc, tc)
                assert rc == want_rc, what
                assert _poison_intact(yb, M, width, col), what
                if entry == "tail":
                    assert done.value == 0, what              # (no tail handed over: nothing else was written)
                if rc != OK:
                    assert sum(tc.values()) == 0, what        # refused before anything was launched
                    continue
                if form == "two":
                    assert tc.get(ONE, 0) == 0 and tc.get(MAPS, 0) >= 1 and tc.get(GRAPH, 0) >= 1, what
                else:
                    assert tc.get(ONE, 0) == 1 and tc.get(MAPS, 0) == 0 and tc.get(GRAPH, 0) == 0, what
                    assert mid == (1 if form == "mid" else 0), what
                y = _block(yb, M, width, col)
                err = float((y.double() - ref).abs().max())
                assert err <= 1e-5 * scale, (what, err)
                if base is None:
                    assert (entry, place, xoff) == ("packed", "own", 0)
                    base = (y, form)
                elif form == base[1]:
                    assert torch.equal(y, base[0]), what       # same kernel form: the same bits wherever the buffers sit
                else:
                    assert float((y - base[0]).abs().max()) <= 2e-5 * scale, what
    if G == 128 and N == 10:
        # magat_gat_forward_dense_f32 (raw reference-layout weights, packed into the workspace tail) once, odd column block
        t = {k: v.to(dev).contiguous() for k, v in p.items()}
        wsd = torch.zeros(ws.numel() + 4 * lib.magat_gat_packed_floats(G, G, K, P, md) + 256, dtype=torch.uint8, device=dev)
        for xoff, place in ((0, "odd"), (2, "own")):
            xb, X = _x_at(rows, xoff, dev)
            yb, yp, ldy, col = _y_at(M, width, place, dev)
            rc, tc, _ = _run(lambda: lib.magat_gat_forward_dense_f32(
                X.data_ptr(), Sd.data_ptr(), 1 if s64 else 0, t["weight"].data_ptr(), t["weight_bias"].data_ptr(),
                t["mixer"].data_ptr(), t["filterWeight"].data_ptr(), bias.data_ptr(), yp, ldy, None, wsd.data_ptr(), wsd.numel(),
                B, N, G, G, K, P, md, 1 if concat else 0, stream), tag_counts)
            assert _poison_intact(yb, M, width, col), (xoff, place, rc)
            if xoff:
                assert rc == UNSUPPORTED and tc.get(ONE, 0) + tc.get(MAPS, 0) + tc.get(GRAPH, 0) == 0, (rc, tc)
            else:
                assert rc == OK, rc
                assert float((_block(yb, M, width, col).double() - ref).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("N,G", [(10, 128), (110, 128)])
def test_tail_entry_with_the_action_head(gpu_device, tag_counts, N, G):
    """magat_gat_forward_tail_f32 with the five-output action head: the layer's rows AND the head's logits (whether the head rode
    in the layer's last launch or is left to the caller, *tail_done says which) against float64 references."""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    dev = gpu_device
    B, K, P, concat = 1, 3, 4, True
    width, M = P * G, B * N
    x, S = _inputs(B, N, G, False, seed=N)
    p = _layer(G, K, P, "KeyQuery", concat, seed=3)
    ref = _oracle(x, S, p, "KeyQuery", concat)
    packed, bias, _ = _pack(p, G, K, P, 0, dev)
    Sd = S.to(dev).contiguous()
    ws = torch.zeros(lib.magat_gat_workspace_bytes(B, N, G, G, K, P, 0, 1), dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(11)
    Wa, ba = torch.randn(5, width, generator=g) * 0.05, torch.randn(5, generator=g) * 0.1
    logits_ref = ref @ Wa.double().t() + ba.double()
    Wd, bd = Wa.to(dev), ba.to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    xb, X = _x_at(x.permute(0, 2, 1).reshape(M, G), 0, dev)
    Y = torch.empty(M, width, device=dev)
    out = torch.full((M, 5), float("nan"), device=dev)
    d = nat.ConvGemmDesc()
    d.inp, d.Cin, d.lda = Y.data_ptr(), width, width
    d.wt, d.bias, d.out = Wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    d.M, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad, d.Hout, d.Wout = M, 1, 1, 1, 1, 1, 0, 1, 1
    d.Cout, d.ldc, d.relu, d.tag = 5, 5, 0, nat.TAG_ACTIONS
    done = ctypes.c_int(7)
    rc, tc, _ = _run(lambda: lib.magat_gat_forward_tail_f32(X.data_ptr(), Sd.data_ptr(), 0, packed.data_ptr(), bias.data_ptr(),
                                                            Y.data_ptr(), width, ws.data_ptr(), ws.numel(), B, N, G, G, K, P, 0,
                                                            1, ctypes.byref(d), ctypes.byref(done), stream), tag_counts)
    assert rc == OK and done.value in (0, 1), (rc, done.value)
    if not done.value:
        assert lib.magat_conv_gemm_f32(ctypes.byref(d), stream) == OK
    torch.cuda.synchronize()
    scale = max(1.0, float(ref.abs().max()))
    assert float((Y.cpu().double() - ref).abs().max()) <= 1e-5 * scale
    assert float((out.cpu().double() - logits_ref).abs().max()) <= 1e-4 * max(1.0, float(logits_ref.abs().max()))


def _host_csr(S, rule):
    """rowptr (absolute) / colidx / vals in the header's order; rule 0: |S| > 1e-9, 2: float(S) != 0"""
    Sn = S.double().numpy()
    edge = (np.abs(Sn) > 1e-9) if rule == 0 else (Sn.astype(np.float32) != 0)
    B, N = Sn.shape[0], Sn.shape[1]
    rowptr = np.zeros(B * (N + 1), dtype=np.int32)
    cols, vals, off = [], [], 0
    for b in range(B):
        for i in range(N):
            rowptr[b * (N + 1) + i] = off
            j = np.nonzero(edge[b, i])[0]
            cols.append(j.astype(np.int32))
            vals.append(Sn[b, i, j].astype(np.float32))
            off += len(j)
        rowptr[b * (N + 1) + N] = off
    return rowptr, np.concatenate(cols), np.concatenate(vals), off


CSR = [(10, 128, "KeyQuery", 2, 4, True), (129, 32, "GAT_modified", 3, 1, False), (1000, 64, "KeyQuery", 1, 2, True),
       (129, 128, "GAT_modified", 2, 1, True), (100, 32, "GAT_origin", 3, 4, False)]


@pytest.mark.parametrize("N,G,mode,K,P,concat", CSR, ids=["N%d_G%d_%s_K%d" % (c[0], c[1], c[2], c[3]) for c in CSR])
def test_csr_and_csc_entries_under_every_placement(gpu_device, tag_counts, N, G, mode, K, P, concat):
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.graphml import CsrStructure
    lib = nat.lib()
    dev = gpu_device
    md = MODES[mode]
    B = 2
    width = P * G if concat else G
    M = B * N
    x, S = _inputs(B, N, G, False, seed=N + G)
    p = _layer(G, K, P, mode, concat, seed=N)
    ref = _oracle(x, S, p, mode, concat)
    scale = max(1.0, float(ref.abs().max()))
    packed, bias, _ = _pack(p, G, K, P, md, dev)
    Sd = S.to(dev).contiguous()
    csr = CsrStructure().build(Sd, 1 if mode == "GAT_origin" else 0)
    nnz = csr.ready(dev)
    rows = x.permute(0, 2, 1).reshape(M, G)
    stream = torch.cuda.current_stream().cuda_stream
    c = 1 if concat else 0
    for entry in ("csr", "csc"):
        if entry == "csr":
            ws = torch.zeros(lib.magat_gat_csr_workspace_bytes(B, N, nnz, G, G, K, P, md, c), dtype=torch.uint8, device=dev)
        else:
            ws = torch.zeros(lib.magat_gat_csc_workspace_bytes(B, N, nnz, G, G, K, P, md, c, 0), dtype=torch.uint8, device=dev)
        base = None
        for place in PLACES:
            for xoff in (0, 1, 2, 3):
                xb, X = _x_at(rows, xoff, dev)
                yb, yp, ldy, col = _y_at(M, width, place, dev)
                tail = (nnz, packed.data_ptr(), bias.data_ptr(), yp, ldy, None, ws.data_ptr(), ws.numel(), B, N, G, G, K, P, md,
                        c, stream)
                if entry == "csr":
                    fn = lambda: lib.magat_gat_forward_csr_f32(X.data_ptr(), csr.rowptr.data_ptr(), csr.colidx.data_ptr(), *tail)
                else:
                    fn = lambda: lib.magat_gat_forward_csc_f32(X.data_ptr(), csr.rowptr.data_ptr(), csr.colidx.data_ptr(),
                                                               csr.cscptr.data_ptr(), csr.csc[0].data_ptr(),
                                                               csr.csc[1].data_ptr(), *tail)
                rc, tc, _ = _run(fn, tag_counts)
                what = (entry, place, xoff, rc, tc)
                assert _poison_intact(yb, M, width, col), what
                if xoff:
                    assert rc == UNSUPPORTED and sum(tc.values()) == 0, what
                    continue
                assert rc == OK, what
                y = _block(yb, M, width, col)
                assert float((y.double() - ref).abs().max()) <= 1e-5 * scale, what
                if base is None:
                    base = y
                else:
                    assert torch.equal(y, base), what          # one kernel sequence for every placement: the same bits


def _bf16_expect(entry, fused, xoff, y_aligned, ldy, bias_off):
    """the rule magat_hip.h "Alignment" states for the bf16-storage entries: X on a 16-byte boundary; the fused form of the CSC
    entries (exception (2)) also needs Y and bias on a 16-byte boundary and ldy a multiple of 8 (bf16 rows) / 4 (float32 rows)"""
    if xoff:
        return UNSUPPORTED
    if fused and entry != "csr":
        if not y_aligned or bias_off or ldy % (4 if entry == "csc_f32out" else 8):
            return UNSUPPORTED
    return OK


@pytest.mark.parametrize("N", [10, 129, 1000])
def test_bf16_csr_and_csc_entries_under_every_placement(gpu_device, tag_counts, N):
    """magat_gat_forward_csr_bf16, _csc_bf16 and _csc_bf16_f32out at every placement of X, Y (own rows, column 0 of wider rows,
    an odd column offset, a row stride of 4 mod 8 elements) and the bias.  N = 10 and 1000 are the fused form's shape
    (gat_csr_fused.hip: KeyQuery, K = 2, G = F = 128, concat), N = 129 at 64 features is not."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.graphml import CsrStructure
    from oracle import magat_oracle as orc
    lib = nat.lib()
    dev = gpu_device
    B, G, K, P, concat = 2, 128 if N != 129 else 64, 2, 2, True
    width, M = P * G, B * N
    fused = G == 128 and nat.get_option("CSR_FUSED") != 0
    x, S = _inputs(B, N, G, N == 10, seed=N + 1)
    p = _layer(G, K, P, "KeyQuery", concat, seed=N + 2)
    y_emul, _ = orc.gat_layer_forward_bf16_storage(x, S.unsqueeze(1), p, "KeyQuery", concat)
    y_emul = y_emul.permute(0, 2, 1).reshape(M, width)
    scale = max(1.0, float(y_emul.abs().max()))
    packed, bias, _ = _pack(p, G, K, P, 0, dev)
    bias_buf = torch.zeros(bias.numel() + 4, device=dev)
    bias_buf[1:1 + bias.numel()] = bias
    Sd = S.to(dev).contiguous()
    csr = CsrStructure().build(Sd, 0)
    nnz = csr.ready(dev)
    rows = x.permute(0, 2, 1).reshape(M, G)
    stream = torch.cuda.current_stream().cuda_stream
    csc_bits = None
    for entry in ("csr", "csc", "csc_f32out"):
        ydt = torch.float32 if entry == "csc_f32out" else torch.bfloat16
        if entry == "csr":
            ws = torch.zeros(lib.magat_gat_csr_bf16_workspace_bytes(B, N, nnz, G, G, K, P, 0, 1), dtype=torch.uint8, device=dev)
        else:
            ws = torch.zeros(lib.magat_gat_csc_workspace_bytes(B, N, nnz, G, G, K, P, 0, 1, 1), dtype=torch.uint8, device=dev)
        base = None
        cases = [(place, xoff, 0) for place in ("own", "col0", "odd", "ld4") for xoff in (0, 1, 2, 7)] + [("own", 0, 1)]
        for place, xoff, bias_off in cases:
            xb, X = _x_at(rows, xoff, dev, torch.bfloat16)
            yb, yp, ldy, col = _y_at(M, width, "own" if place == "ld4" else place, dev, ydt)
            if place == "ld4":                      # (a row stride of 4 mod 8 elements, the block at column 0)
                yb = torch.full((M + 1, width + 4), POISON if ydt == torch.float32 else 0x7FCD,
                                dtype=torch.int32 if ydt == torch.float32 else torch.int16, device=dev)
                yp, ldy, col = yb.data_ptr(), width + 4, 0
            bptr = bias_buf.data_ptr() + 4 if bias_off else bias.data_ptr()
            tail = (nnz, packed.data_ptr(), bptr, yp, ldy, None, ws.data_ptr(), ws.numel(), B, N, G, G, K, P, 0, 1, stream)
            if entry == "csr":
                fn = lambda: lib.magat_gat_forward_csr_bf16(X.data_ptr(), csr.rowptr.data_ptr(), csr.colidx.data_ptr(), *tail)
            else:
                f = lib.magat_gat_forward_csc_bf16 if entry == "csc" else lib.magat_gat_forward_csc_bf16_f32out
                fn = lambda: f(X.data_ptr(), csr.rowptr.data_ptr(), csr.colidx.data_ptr(), csr.cscptr.data_ptr(),
                               csr.csc[0].data_ptr(), csr.csc[1].data_ptr(), *tail)
            rc, tc, _ = _run(fn, tag_counts)
            n_fused = int(lib.magat_form_count(nat.FORMS["csr_fused"]))
            want = _bf16_expect(entry, fused, xoff, yp % 16 == 0, ldy, bias_off)
            what = (entry, place, xoff, bias_off, ldy, rc, tc)
            assert rc == want, what
            assert _poison_intact(yb, M, width, col, ydt), what
            if rc != OK:
                assert sum(tc.values()) == 0 and n_fused == 0, what        # refused before anything was launched
                continue
            assert n_fused == (1 if fused and entry != "csr" else 0), what
            y = _block(yb, M, width, col, ydt)
            assert float((y - y_emul).abs().max()) <= 2.0 ** -7 * scale, what
            if base is None:
                base = y
            else:
                assert torch.equal(y, base), what       # one kernel sequence for every placement: the same bits
        if entry == "csc":
            csc_bits = base
        elif entry == "csc_f32out":
            assert torch.equal(base, csc_bits)           # the widened rows are the bf16 result's values


@pytest.mark.parametrize("N,G,K", [(10, 32, 3), (129, 128, 2), (1000, 16, 1)])
def test_gnn_csr_entry_under_every_placement(gpu_device, tag_counts, N, G, K):
    from magat_pathplanning_amd import _native as nat
    from oracle import magat_oracle as orc
    lib = nat.lib()
    dev = gpu_device
    B, F = 2, G
    M = B * N
    x, S = _inputs(B, N, G, False, seed=N + K)
    g = torch.Generator().manual_seed(N)
    w = torch.randn(F, 1, K, G, generator=g) * (1.0 / G) ** 0.5
    b = torch.randn(F, 1, generator=g) * 0.1
    # (the oracle keeps the reference's float(S) products - graphML.py:5562 - so this one reference is float32)
    ref = orc.graph_filter_batch_forward(x, S.unsqueeze(1), w, b).double()
    ref = ref.permute(0, 2, 1).reshape(M, F)
    scale = max(1.0, float(ref.abs().max()))
    rowptr, colidx, vals, nnz = _host_csr(S, 2)
    rp, ci, vv = (torch.from_numpy(a).to(dev) for a in (rowptr, colidx, vals))
    wd = w.to(dev).contiguous()
    bias = b.reshape(-1).to(dev).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(lib.magat_gat_packed_floats(G, F, K, 1, 3), dtype=torch.float32, device=dev)
    assert lib.magat_gat_pack_weights(None, None, None, wd.data_ptr(), packed.data_ptr(), G, F, K, 1, 3, stream) == OK
    ws = torch.zeros(lib.magat_gat_csr_workspace_bytes(B, N, nnz, G, F, K, 1, 3, 1), dtype=torch.uint8, device=dev)
    rows = x.permute(0, 2, 1).reshape(M, G)
    base = None
    for place in PLACES:
        for xoff in (0, 1, 2, 3):
            xb, X = _x_at(rows, xoff, dev)
            yb, yp, ldy, col = _y_at(M, F, place, dev)
            rc, tc, _ = _run(lambda: lib.magat_gnn_forward_csr_f32(X.data_ptr(), rp.data_ptr(), ci.data_ptr(), vv.data_ptr(), nnz,
                                                                   packed.data_ptr(), bias.data_ptr(), yp, ldy, ws.data_ptr(),
                                                                   ws.numel(), B, N, G, F, K, stream), tag_counts)
            what = (place, xoff, rc, tc)
            assert _poison_intact(yb, M, F, col), what
            if xoff:
                assert rc == UNSUPPORTED and sum(tc.values()) == 0, what
                continue
            assert rc == OK, what
            y = _block(yb, M, F, col)
            assert float((y.double() - ref).abs().max()) <= 1e-5 * scale, what
            if base is None:
                base = y
            else:
                assert torch.equal(y, base), what


def test_module_path_takes_an_unaligned_x(gpu_device):
    """graphml.gat_forward_rows with X a contiguous view at a non-16-byte offset, at a shape (G = 128, N = 110) that only the
    one-launch gat_mid form covers among the dense kernels.  Every entry point refuses such an X (the tests above), so the module
    path hands the kernels an aligned copy: the oracle's numbers."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.graphml import gat_forward_rows
    B, N, G, K, P = 2, 110, 128, 3, 4
    x, S = _inputs(B, N, G, False, seed=5)
    p = _layer(G, K, P, "KeyQuery", True, seed=6)
    ref = _oracle(x, S, p, "KeyQuery", True)
    layer = GraphFilterBatchAttentional(G, G, K, P, attentionMode="KeyQuery", concatenate=True)
    layer.load_state_dict(p)
    layer = layer.to(gpu_device).eval()
    base = torch.zeros(B * N * G + 4, device=gpu_device)
    X = base[1:1 + B * N * G].view(B, N, G)
    X.copy_(x.permute(0, 2, 1).to(gpu_device))
    assert X.is_contiguous() and X.data_ptr() % 16 == 4
    with torch.no_grad():
        out, _ = gat_forward_rows(X, S.to(gpu_device), layer)
    torch.cuda.synchronize()
    assert float((out.cpu().double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
