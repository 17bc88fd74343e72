"""The float32 segmented-K MFMA kernel (csrc/conv_gemm_f32.hip, magat_conv_gemm_f32 with in_fmt = 0) in every form its dispatcher
picks, against float64 on the CPU - and the two encoder passes that run on it alone: the calibration pass, whose `absmax[16]`
decides every activation scale of the fast path, and the range guard's predicated re-run (conv_gemm_chain_kernel).  Behind them
magat_cast_rows, which makes the bf16 rows of the re-run.

Cases, layouts, references and gates: tests/conv_f32_cases.py (tests/test_host_conv_f32_cases.py checks on the CPU that the table
reaches all twelve tile template x loader pairs, agent-tile counts 1 / 8 / 9 / 17 and the edges listed there).

What is asserted
  every form        max|got - float64| <= 3e-5 max(1, max|float64|), and every padding row and column of the output still holds
                    its poison (inputs and weights carry NaN in theirs)
  tile-major        [agent tile][pixel][128][ld] as the encoder lays its maps out: bit-identical to the pixel-major run of the
                    same case, and rows 0..255 of the 257-agent run bit-identical to the 256-agent (FULL loader) run - the order
                    of the sums of one output element depends on neither the loader nor the batch
  run_if            flag 0: the output keeps its poison everywhere; flag 1: bit-identical to the unpredicated launch, also when
                    512 workgroups walk 968 tiles
  absmax            the float32 maximum of |out| over the valid region of the kernel's own output, bit for bit; a larger value
                    already there survives, an all-zero launch leaves it alone, the 1e30 in the padding is not picked up
  calibration       absmax[0..8] within 2e-5 max(1, v) of the float64 per-layer maxima v, the same scale exponent
                    (encoder.scale_exponent), slots the variant does not have and slots 9..15 exactly 0; the input's last agent
                    - in the ragged tile - holds every maximum
  re-run            status says so; feat and comp within 2e-5 max(1, max|float64|); the bf16 rows are comp.to(bfloat16) bit for bit
  magat_cast_rows   bit-exact against torch for finite values and infinities in both directions, NaN stays NaN with its sign

Measured on an MI355X: tile template (p: pooled), loader, agent tiles, max|got - float64| / gate (max(1, max|float64|) included)
  test_forms_vs_float64
    stepA-M128             128x32   FULL    1  2.73e-06 / 1.52e-04     stepA-M129             128x32   ragged  2  2.78e-06 / 1.69e-04
    stepA-M256             128x32   FULL    2  2.59e-06 / 1.57e-04     stepA-M257             128x32   ragged  3  2.46e-06 / 1.63e-04
    stepB-M128             128x64   FULL    1  2.87e-06 / 1.72e-04     stepB-M129             128x64   ragged  2  3.18e-06 / 1.56e-04
    stepB-M256             128x64   FULL    2  2.99e-06 / 2.18e-04     stepB-M257             128x64   ragged  3  2.72e-06 / 1.90e-04
    stepC-M64              64x128   FULL    1  4.20e-06 / 1.67e-04     stepC-M65              64x128   ragged  2  3.98e-06 / 1.85e-04
    stepC-M128             64x128   FULL    2  4.99e-06 / 1.99e-04     stepC-M129             64x128   ragged  3  5.01e-06 / 1.78e-04
    grid128-M1664          128x128  FULL   13  1.51e-06 / 2.27e-04     grid128-M1665          128x128  ragged 14  1.67e-06 / 2.37e-04
    ragged-Cout5           128x32   ragged  1  2.05e-06 / 1.97e-04     ragged-Cout33          128x64   ragged  1  2.50e-06 / 2.17e-04
    ragged-Cout65          64x128   ragged  2  3.10e-06 / 2.14e-04     ragged-Cout130         64x128   ragged  2  3.02e-06 / 2.42e-04
    ldw-full               128x64   FULL    1  3.20e-06 / 2.08e-04     ldw-ragged             128x64   ragged  1  2.87e-06 / 2.27e-04
    ld-full                128x64   FULL    1  3.20e-06 / 2.08e-04     ld-full-odd-ldc        128x64   FULL    1  3.20e-06 / 2.08e-04
    ld-ragged              64x128   ragged  3  2.90e-06 / 2.49e-04
    tiles128-M1024         128x32   FULL    8  1.01e-06 / 1.65e-04     tiles128-M1030         128x32   ragged  9  1.15e-06 / 1.72e-04
    tiles128-M2176         128x32   FULL   17  1.08e-06 / 1.94e-04     tiles64-M512           64x128   FULL    8  1.80e-06 / 1.57e-04
    tiles64-M513           64x128   ragged  9  1.92e-06 / 1.37e-04     tiles64-M1088          64x128   FULL   17  1.55e-06 / 1.37e-04
    rect-7x11              128x32   ragged  2  3.48e-06 / 2.05e-04     rect-7x11-s2           128x64   FULL    1  2.54e-06 / 1.74e-04
    even-12-s2             128x32   ragged  2  3.92e-06 / 1.79e-04
    valid-6x6-M64          64x128   FULL    1  4.82e-06 / 1.43e-04     valid-6x6-M65          64x128   ragged  2  4.75e-06 / 1.74e-04
    pool1-M64              64x128p  FULL    1  4.29e-06 / 2.19e-04     pool1-M65              64x128p  ragged  2  5.20e-06 / 2.50e-04
    pool2-M64              64x128p  FULL    1  2.22e-06 / 1.77e-04     pool2-M65              64x128p  ragged  2  2.41e-06 / 1.62e-04
    pool2-Cout32           64x128p  ragged  2  2.60e-06 / 1.43e-04
    poolgrid-sum-M2048     128x128p FULL   16  2.95e-06 / 3.69e-04     poolgrid-max-M2049     128x128p ragged 17  1.85e-06 / 2.51e-04
    res-l1conv2-M128       128x32   FULL    1  3.13e-06 / 2.13e-04     res-l1conv2-M129       128x32   ragged  2  2.57e-06 / 2.26e-04
    res-l1conv2-C2x4-M128  128x32   ragged  1  2.84e-06 / 2.33e-04     res-l1conv2-C2x4-M129  128x32   ragged  2  2.69e-06 / 2.19e-04
  test_tile_major_layout_is_bit_identical: the largest of the six runs (129 / 256 / 257 agents, both layouts) of each shape
    stepA 128x32  2.46e-06 / 1.63e-04     stepB 128x64  2.72e-06 / 1.88e-04     stepC 64x128  4.71e-06 / 1.80e-04
    resA  128x32  3.31e-06 / 2.50e-04     resB  128x64  4.71e-06 / 2.25e-04     resC  64x128  6.69e-06 / 2.24e-04
  test_run_if_predicate, test_absmax_is_the_maximum_of_the_valid_output (absmax and max|valid out| agree in all nine digits printed)
    runif-6x6 2.71e-06 / 1.63e-04 (grid 288)     runif-11x11 2.85e-06 / 1.55e-04 (968 tiles, 512 workgroups)
    absmax-relu 2.33e-06 / 1.74e-04, 5.78865814     absmax-negative 3.01e-06 / 2.88e-04, 9.60776901
    absmax-full 3.15e-06 / 2.97e-04, 9.90542984     absmax-tile-major 2.57e-06 / 2.26e-04, 7.52177906
  test_calibration_absmax_vs_float64: the largest |absmax[s] - float64| over the slots / the smallest gate; feat; comp
    ResNetLarge_withMLP M=1    7.43e-07 / 2.00e-05   feat 7.15e-07 / 2.03e-05   comp 7.43e-07 / 2.00e-05
    ResNetLarge_withMLP M=128  5.65e-07 / 2.00e-05   feat 1.40e-06 / 2.00e-05   comp 8.42e-07 / 2.00e-05
    ResNetLarge_withMLP M=129  3.38e-07 / 2.00e-05   feat 1.16e-06 / 2.14e-05   comp 7.51e-07 / 2.00e-05
    ResNetLarge_withMLP M=257  1.14e-06 / 2.00e-05   feat 1.26e-06 / 2.13e-05   comp 9.48e-07 / 2.00e-05
    ResNetSlim_withMLP  M=129  4.91e-07 / 2.57e-05   feat 8.44e-07 / 2.57e-05   comp 5.83e-07 / 2.67e-05
    ResNetLarge         M=129  3.38e-07 / 2.37e-05   feat 6.44e-07 / 2.38e-05
  test_guard_rerun_vs_float64 (status: flag 1, one re-run; max|feat| is ~4e4)
    M=129   feat 3.54e-02 / 7.82e-01   comp 2.40e-02 / 6.60e-01
    M=257   feat 3.75e-02 / 9.52e-01   comp 2.49e-02 / 6.29e-01
    M=4100  feat 3.75e-02 / 9.52e-01   comp 2.49e-02 / 6.29e-01
Every test of this module takes 0.4 s or less.
"""
import ctypes
import types

import pytest
import torch

import conv_f32_cases as cc

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _nat():
    from magat_pathplanning_amd import _native as nat
    return nat, nat.lib()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(dev, c, t, run_if=None, absmax=None):
    """One launch of the case: the output buffer in the case's layout, on the CPU, poison where the kernel must not write."""
    nat, lib = _nat()
    xin = cc.pack_map(t.x, c.layout, c.lda, NAN).to(dev)
    wt, b = cc.weight_rows(c, t).to(dev), t.b.to(dev)
    T = -(-c.M // cc.TILE_ROWS)
    shape = (c.npix, c.M, c.ldc) if c.layout == cc.PIX else (T, c.npix, cc.TILE_ROWS, c.ldc)
    out = torch.full(shape, cc.POISON, device=dev)
    d = nat.ConvGemmDesc()
    d.inp, d.wt, d.bias, d.out = xin.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr()
    (d.in_pix_stride, d.in_tile_stride), (d.out_pix_stride, d.out_tile_stride) = cc.strides(c, "in"), cc.strides(c, "out")
    d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = c.M, c.cin, c.lda, c.hin, c.win, c.k, c.k, c.stride, c.pad
    d.Hout, d.Wout, d.Cout, d.ldc, d.relu = c.hout, c.wout, c.cout, c.ldc, c.relu
    if c.ldw != c.ktot:
        d.ldw = c.ldw
    if c.pool:
        d.pool, d.pool_w = c.pool, c.wphys
    if c.c2:
        x2 = cc.pack_map(t.x2, c.layout, c.lda2, NAN).to(dev)
        d.in2, d.C2, d.lda2, d.W2, d.stride2 = x2.data_ptr(), c.c2, c.lda2, c.w2, c.stride2
        d.in2_pix_stride, d.in2_tile_stride = cc.strides(c, "in2")
    if run_if is not None:
        d.run_if = run_if
    if absmax is not None:
        d.absmax = absmax
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(dev)), "conv_gemm " + c.id)
    torch.cuda.synchronize()
    return out.cpu()


def _check(c, buf, ref, what=""):
    """The gate and the padding; returns the map (M, Cout, Hout, Wout)."""
    mask = cc.valid_mask(buf, c.layout, c.M, c.cout)
    got = cc.unpack_map(buf, c.layout, c.M, c.cout, c.hout, c.wout)
    assert bool(torch.isfinite(got).all()), c.id
    err, lim = float((got.double() - ref).abs().max()), cc.GATE * max(1.0, float(ref.abs().max()))
    bm, bn, pooled = cc.tile_choice(c)
    print("conv_f32: %-34s %3dx%-3d%s %-6s tiles %2d  %.2e / %.2e %s" % (
        c.id, bm, bn, "p" if pooled else " ", "FULL" if cc.is_full(c) else "ragged", cc.agent_tiles(c), err, lim, what))
    assert err <= lim, (c.id, err, lim)
    assert bool((buf[~mask] == cc.POISON).all()), c.id
    return got


@pytest.mark.parametrize("c", cc.FORMS, ids=[c.id for c in cc.FORMS])
def test_forms_vs_float64(gpu_device, c):
    t = cc.make_inputs(c)
    _check(c, _run(gpu_device, c, t), cc.reference(c, t))


@pytest.mark.parametrize("c", cc.TILE_MAJOR, ids=[c.id for c in cc.TILE_MAJOR])
def test_tile_major_layout_is_bit_identical(gpu_device, c):
    ref = cc.reference(c, cc.make_inputs(c))          # 257 agents; the smaller batches are its first rows
    got = {}
    for m in cc.TILE_MAJOR_M:
        for lay in (cc.PIX, cc.TILE):
            cm = cc.with_layout(c, lay, m)
            got[m, lay] = _check(cm, _run(gpu_device, cm, cc.make_inputs(cm)), ref[:m])
        assert torch.equal(_bits(got[m, cc.PIX]), _bits(got[m, cc.TILE])), (c.id, m)
    for lay in (cc.PIX, cc.TILE):
        assert torch.equal(_bits(got[257, lay][:256]), _bits(got[256, lay])), (c.id, lay)
        assert torch.equal(_bits(got[257, lay][:129]), _bits(got[129, lay])), (c.id, lay)


@pytest.mark.parametrize("c", cc.RUN_IF, ids=[c.id for c in cc.RUN_IF])
def test_run_if_predicate(gpu_device, c):
    t = cc.make_inputs(c)
    flags = torch.tensor([0, 1, 0, -5], dtype=torch.int32, device=gpu_device)
    base = _run(gpu_device, c, t)
    _check(c, base, cc.reference(c, t), "grid %d" % cc.launch_grid(c))
    off = _run(gpu_device, c, t, run_if=flags.data_ptr())
    assert bool((off == cc.POISON).all())
    for word in (1, 3):          # any non-zero word runs the launch
        on = _run(gpu_device, c, t, run_if=flags.data_ptr() + 4 * word)
        assert torch.equal(_bits(on), _bits(base)), (c.id, word)


@pytest.mark.parametrize("c", cc.ABSMAX, ids=[c.id for c in cc.ABSMAX])
def test_absmax_is_the_maximum_of_the_valid_output(gpu_device, c):
    t = cc.make_inputs(c)
    if not c.relu:
        t.b = -(t.b.abs() + 4.0)          # negative outputs dominate: the maximum of |out| is not the maximum of out
    am = torch.zeros(4, device=gpu_device)

    def launch(preset, tt=t):
        am.zero_()
        am[1] = preset
        buf = _run(gpu_device, c, tt, absmax=am.data_ptr() + 4)
        res = am.cpu()
        assert float(res[0]) == 0.0 and float(res[2]) == 0.0 and float(res[3]) == 0.0      # one float, nothing beside it
        return buf, res[1:2]

    buf, got = launch(0.0)
    _check(c, buf, cc.reference(c, t))
    valid = buf[cc.valid_mask(buf, c.layout, c.M, c.cout)]
    want = valid.abs().max().reshape(1)
    print("conv_f32: %-34s absmax %.9g, max|valid out| %.9g" % (c.id, float(got), float(want)))
    assert torch.equal(_bits(got), _bits(want)), (float(got), float(want))
    assert 1.0 < float(want) < 1.0e3                      # (not the 1e30 of the padding rows and columns)
    if not c.relu:
        assert float(valid.max()) < 0.5 * float(want) and float(valid.min()) == -float(want)
    # a larger value already there survives, a smaller one is raised
    assert torch.equal(_bits(launch(2.0 * float(want))[1]), _bits(2.0 * want))
    assert torch.equal(_bits(launch(0.5 * float(want))[1]), _bits(want))
    # a launch whose outputs are all zero leaves it untouched
    zero = cc.make_inputs(c)
    zero.w, zero.b = torch.zeros_like(zero.w), torch.zeros_like(zero.b)
    if c.c2:
        zero.w2 = torch.zeros_like(zero.w2)
    for preset in (0.0, 0.25):
        buf0, got0 = launch(preset, zero)
        assert bool((buf0[cc.valid_mask(buf0, c.layout, c.M, c.cout)] == 0.0).all())
        assert torch.equal(_bits(got0), _bits(torch.tensor([preset])))


# ---- the encoder passes -------------------------------------------------------------------------------------------------------
def _encoder(dev, cnn, scaled=False):
    """The C entry's descriptor as tests/test_gpu_model.py::test_encoder_other_map_sizes builds it, 11 x 11 maps."""
    from magat_pathplanning_amd import encoder as enc
    nat, lib = _nat()
    cfg, sd = cc.encoder_model(cnn, scaled)
    mlp = cnn.endswith("_withMLP")
    lin = (sd["ConvLayers.3.weight"], sd["ConvLayers.3.bias"]) if mlp else None
    comp = (sd["compressMLP.0.weight"], sd["compressMLP.0.bias"]) if mlp else None
    pack, offs, meta = enc.fold_resnet(sd, cc.HW, cc.HW, "ConvLayers.0", lin, comp)
    packd = pack.to(dev)
    d = nat.EncoderDesc()
    d.variant, d.H, d.W, d.n_feat, d.n_comp, d.pack = meta["variant"], cc.HW, cc.HW, meta["n_feat"], meta["n_comp"], packd.data_ptr()
    for i, o in enumerate(offs):
        d.off[i] = o
    return types.SimpleNamespace(d=d, pack=packd, n_feat=meta["n_feat"], n_comp=meta["n_comp"])


def _workspace(dev, e, M):
    nat, lib = _nat()
    return torch.zeros(lib.magat_encoder_workspace_bytes(ctypes.byref(e.d), M), dtype=torch.uint8, device=dev)      # status block zeroed


def _status(dev, ws):
    nat, lib = _nat()
    st = (ctypes.c_int32 * 2)()
    nat.check(lib.magat_encoder_read_status(nat.ptr(ws), st, nat.current_stream(dev)), "magat_encoder_read_status")
    return int(st[0]), int(st[1])


def _within(name, got, ref):
    err, lim = float((got.double().cpu() - ref).abs().max()), cc.ENC_GATE * max(1.0, float(ref.abs().max()))
    print("conv_f32:   %-6s %.2e / %.2e" % (name, err, lim))
    assert err <= lim, (name, err, lim)


@pytest.mark.parametrize("cnn,M", cc.CALIBRATE, ids=["%s-M%d" % cm for cm in cc.CALIBRATE])
def test_calibration_absmax_vs_float64(gpu_device, cnn, M):
    from magat_pathplanning_amd import encoder as enc
    nat, lib = _nat()
    e = _encoder(gpu_device, cnn)
    ref = cc.encoder_reference(cnn, M)
    x = cc.encoder_states(M).to(gpu_device)
    ws = _workspace(gpu_device, e, M)
    feat = torch.full((M, e.n_feat), NAN, device=gpu_device)
    comp = torch.full((M, e.n_comp), NAN, device=gpu_device) if e.n_comp else None
    am = torch.full((cc.SLOTS + 8,), 7.0, device=gpu_device)          # the entry clears its 16 floats itself, and only those
    nat.check(lib.magat_encoder_calibrate_f32(ctypes.byref(e.d), nat.ptr(x), nat.ptr(feat), e.n_feat, nat.ptr(comp), e.n_comp,
                                              nat.ptr(ws), ws.numel(), M, nat.ptr(am), nat.current_stream(gpu_device)),
              "magat_encoder_calibrate_f32")
    torch.cuda.synchronize()
    got = am.cpu()
    assert bool((got[cc.SLOTS:] == 7.0).all())
    print("conv_f32: calibrate %s M=%d" % (cnn, M))
    for s in range(cc.SLOTS):
        v = ref.maxima[s] if s < cc.SLOTS_USED else None
        if v is None:
            assert float(got[s]) == 0.0, (s, float(got[s]))
            continue
        err, lim = abs(float(got[s]) - v), cc.ENC_GATE * max(1.0, v)
        print("conv_f32:   slot %d  float64 %.9g  device %.9g  %.2e / %.2e" % (s, v, float(got[s]), err, lim))
        assert err <= lim, (s, v, float(got[s]))
        assert enc.scale_exponent(float(got[s])) == enc.scale_exponent(v), (s, v, float(got[s]))
    _within("feat", feat, ref.feat)
    if comp is not None:
        _within("comp", comp, ref.comp)


@pytest.mark.parametrize("M", [m for _, m in cc.RERUN] + [cc.RERUN_WALK])
def test_guard_rerun_vs_float64(gpu_device, M):
    """layer2.0.bn1 x 1e5: the f16 planes clamp, the guard's predicated float32 pass rewrites feat and comp, and the bf16 rows
    follow it (at 4100 agents the predicated cast's 512 workgroups walk 513 blocks).  The unscaled pack: no re-run."""
    nat, lib = _nat()
    cnn = cc.LARGE_MLP
    distinct = min(M, 257)
    rows = cc.rerun_walk_rows(M, distinct)
    x = cc.encoder_states(distinct)[rows].contiguous().to(gpu_device)
    for scaled in (True, False):
        e = _encoder(gpu_device, cnn, scaled)
        ws = _workspace(gpu_device, e, M)
        feat = torch.full((M, e.n_feat), NAN, device=gpu_device)
        comp = torch.full((M, e.n_comp), NAN, device=gpu_device)
        comp16 = torch.full((M, e.n_comp), cc.BF16_POISON, dtype=torch.int16, device=gpu_device)
        e.d.comp_bf16 = comp16.data_ptr()
        nat.check(lib.magat_encoder_forward_f32(ctypes.byref(e.d), nat.ptr(x), nat.ptr(feat), e.n_feat, nat.ptr(comp), e.n_comp,
                                                nat.ptr(ws), ws.numel(), M, nat.current_stream(gpu_device)), "encoder")
        torch.cuda.synchronize()
        st = _status(gpu_device, ws)
        if not scaled:
            assert st == (0, 0), st
            continue
        assert st[0] != 0 and st[1] == 1, st
        ref = cc.encoder_reference(cnn, distinct, True)
        print("conv_f32: re-run M=%d status %s" % (M, st))
        _within("feat", feat, ref.feat[rows])
        _within("comp", comp, ref.comp[rows])
        assert torch.equal(comp16.cpu(), comp.cpu().to(torch.bfloat16).view(torch.int16))


# ---- magat_cast_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,width,ld_src,ld_dst", cc.CAST)
def test_cast_rows_to_bf16(gpu_device, M, width, ld_src, ld_dst):
    """Round to nearest even, bit-exact against torch for everything finite or infinite; a NaN stays a NaN of its sign (payloads
    differ between implementations and are not compared).  The rounding add used to carry NaNs of a large payload over:
    0x7fffffff -> 0x8000 (-0), 0xffffffff -> 0x0000 (+0), 0x7f800001 -> 0x7f80 (+inf)."""
    nat, lib = _nat()
    x = cc.cast_source(M, width)
    src = torch.full((M, ld_src), cc.POISON)
    src[:, :width] = x
    dst = torch.full((M, ld_dst), cc.BF16_POISON, dtype=torch.int16, device=gpu_device)
    srcd = src.to(gpu_device)
    nat.check(lib.magat_cast_rows(nat.ptr(srcd), nat.ptr(dst), 1, M, width, ld_src, ld_dst, nat.current_stream(gpu_device)),
              "magat_cast_rows")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert bool((got[:, width:] == cc.BF16_POISON).all())
    got = got[:, :width].to(torch.int32) & 0xffff
    want = x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xffff
    nan = torch.isnan(x)
    assert torch.equal(got[~nan], want[~nan])
    assert int(nan.sum()) == 2 * len(cc.NAN_BITS)
    g = got[nan]
    sign = (x.view(torch.int32)[nan] >> 31) & 1
    assert bool(((g & 0x7f80) == 0x7f80).all()) and bool(((g & 0x007f) != 0).all()), [hex(int(v)) for v in g]
    assert torch.equal(g >> 15, sign), [hex(int(v)) for v in g]


@pytest.mark.parametrize("M,width,ld_dst,ld_src", cc.CAST)
def test_cast_rows_from_bf16(gpu_device, M, width, ld_dst, ld_src):
    """bf16 -> float32 is a shift: every bit pattern, NaNs with their payloads included, exactly."""
    nat, lib = _nat()
    g = torch.Generator().manual_seed(M)
    src = torch.randint(-32768, 32768, (M, ld_src), generator=g, dtype=torch.int32).to(torch.int16)
    sp = cc.cast_source(M, width)[0, :len(cc.SPECIAL_BITS)]
    src[0, :len(cc.SPECIAL_BITS)] = (sp.view(torch.int32) >> 16).to(torch.int16)
    dst = torch.full((M, ld_dst), cc.POISON, device=gpu_device)
    srcd = src.to(gpu_device)
    nat.check(lib.magat_cast_rows(nat.ptr(srcd), nat.ptr(dst), 0, M, width, ld_src, ld_dst, nat.current_stream(gpu_device)),
              "magat_cast_rows")
    torch.cuda.synchronize()
    got = dst.cpu()
    assert bool((got[:, width:] == cc.POISON).all())
    want = src[:, :width].to(torch.int32) << 16
    assert torch.equal(_bits(got[:, :width]), want)
    viat = src[:, :width].contiguous().view(torch.bfloat16).float()
    ok = ~torch.isnan(viat)
    assert torch.equal(_bits(viat)[ok], want[ok])
