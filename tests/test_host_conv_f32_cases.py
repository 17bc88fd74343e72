"""CPU checks of tests/conv_f32_cases.py: the table of tests/test_gpu_conv_f32_forms.py reaches every form of the float32 MFMA
kernel it claims to, the layout helpers round-trip, and the encoder inputs have the properties the calibration test relies on."""
import os
import re

import pytest
import torch

import conv_f32_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_reaches_every_tile_template_with_both_loaders():
    """magat_conv_gemm_f32 picks among (BM, BN) = (128, 32), (128, 64), (64, 128), (128, 128) and the pooled (64, 128), (128, 128),
    each with the FULL or the bounds-checked loader: twelve kernels."""
    seen = {(cc.tile_choice(c), cc.is_full(c)) for c in cc.all_cases()}
    want = {((bm, bn, pooled), full) for bm, bn, pooled in ((128, 32, False), (128, 64, False), (64, 128, False),
                                                            (128, 128, False), (64, 128, True), (128, 128, True))
            for full in (True, False)}
    assert seen == want, sorted(want - seen)
    assert not any(cc.takes_skinny_route(c) for c in cc.all_cases())


def test_restatement_reads_the_dispatcher_it_restates():
    """The numbers tile_choice and is_full are built on stand in csrc/conv_gemm_f32.hip as they stand here."""
    src = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "conv_gemm_f32.hip")).read()
    assert "small_grid = blocks128 < 1536" in src
    assert re.search(r"if \(d->pool\) return small_grid \? launch<64, 128, 2, 2, true>\(p, st\) : launch<128, 128, 2, 2, true>", src)
    assert re.search(r"if \(p\.Cout > 64\) return small_grid \? launch<64, 128, 2, 2>\(p, st\) : launch<128, 128, 2, 2>", src)
    assert "if (p.Cout > 32) return launch<128, 64, 2, 2>(p, st);" in src and "return launch<128, 32, 4, 1>(p, st);" in src
    assert "p.M % BM == 0 && p.Cout % BN == 0 && p.Cin % BK == 0 && p.C2 % BK == 0" in src
    assert "(p.run_if && grid > 512) ? 512 : grid" in src
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "#define MAGAT_TILE_ROWS 128" in common and "#define MAGAT_NUM_XCD 8" in common


def test_table_has_the_agent_tile_counts_and_the_edges():
    tiles = {cc.agent_tiles(c) for c in cc.all_cases()}
    assert {1, 8, 9, 17} <= tiles, tiles
    # ... for both tile heights
    for bm in (64, 128):
        assert {8, 9, 17} <= {cc.agent_tiles(c) for c in cc.FORMS if cc.tile_choice(c)[0] == bm}, bm
    by_id = {c.id: c for c in cc.all_cases()}
    assert len(by_id) == len(cc.all_cases())
    # the predicated launches: one grid launched whole, one walked by 512 workgroups
    assert cc.launch_grid(by_id["runif-6x6"]) == 288 and cc.launch_grid(by_id["runif-11x11"]) == 968
    # ragged channels, row strides wider than the rows, the residual segment as layer1.conv2 has it
    assert {c.cout for c in cc.FORMS if c.cin == 36 and c.c2 == 4} >= {5, 33, 65, 130}
    assert any(c.ldw > c.ktot and cc.is_full(c) for c in cc.FORMS) and any(c.ldw > c.ktot and not cc.is_full(c) for c in cc.FORMS)
    for full in (True, False):
        assert any(c.lda > c.cin and c.lda2 > c.c2 > 0 and c.ldc > c.cout and cc.is_full(c) == full for c in cc.FORMS), full
    assert any(cc.is_full(c) and c.ldc % 4 for c in cc.FORMS)                  # FULL loader without the vector stores
    for m in (128, 129):
        for c2 in (32, 4):
            assert any(c.M == m and c.c2 == c2 and c.stride2 == 2 and (c.h2, c.w2) == (11, 11) and c.hin == 6 for c in cc.FORMS)
    # geometry and pools: rectangular, even input at stride 2, the valid 6 x 6 kernel, both pools FULL and ragged on odd widths
    assert any(c.hin != c.win for c in cc.FORMS) and any(c.hin == 12 and c.stride == 2 and c.hout == 6 for c in cc.FORMS)
    assert any(c.k == 6 and c.pad == 0 and c.npix == 1 for c in cc.FORMS)
    for pool in (1, 2):
        for full in (True, False):
            assert any(c.pool == pool and cc.is_full(c) == full and c.wphys % 2 == 1 for c in cc.FORMS), (pool, full)
    # both layouts of the three encoder steps and their residual forms at 129 / 256 / 257 agents; 256 is the FULL one of stepA / stepB
    for name in ("stepA", "stepB", "stepC", "resA", "resB", "resC"):
        for m in cc.TILE_MAJOR_M:
            for lay in (cc.PIX, cc.TILE):
                c = by_id["%s-%s-M%d" % (name, lay, m)]
                assert cc.is_full(c) == (m == 256), c.id
                assert cc.tile_choice(c) == cc.tile_choice(by_id["%s-%s-M257" % (name, cc.PIX)])      # one template: one order of sums


@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_layouts_round_trip(M):
    g = torch.Generator().manual_seed(M)
    C, H, W, ld = 12, 3, 5, 16
    t = torch.randn(M, C, H, W, generator=g)
    pm, tm = cc.to_pixel_major(t, ld), cc.to_tile_major(t, ld)
    assert pm.shape == (H * W, M, ld) and tm.shape == (-(-M // 128), H * W, 128, ld)
    assert torch.equal(cc.from_pixel_major(pm, C, H, W), t) and torch.equal(cc.from_tile_major(tm, M, C, H, W), t)
    # every element is either a value of the map or poison, and the mask says which
    for buf, lay in ((pm, cc.PIX), (tm, cc.TILE)):
        mask = cc.valid_mask(buf, lay, M, C)
        assert int(mask.sum()) == t.numel() and bool((buf[~mask] == cc.POISON).all()) and not bool((buf[mask] == cc.POISON).any())
        assert torch.equal(cc.unpack_map(cc.pack_map(t, lay, ld), lay, M, C, H, W), t)
    # the strides the descriptor takes address the same element in both
    c = cc.case("x", M, C, C, H, W, lda_x=ld - C)
    for lay, buf in ((cc.PIX, pm), (cc.TILE, tm)):
        c.layout = lay
        pix_stride, tile_stride = cc.strides(c, "in")
        flat = buf.reshape(-1)
        for m, pix, ch in ((0, 0, 0), (M - 1, H * W - 1, C - 1), (M // 2, 7, 3)):
            assert flat[pix * pix_stride + cc.row_off(m, ld, tile_stride) + ch] == t[m, ch, pix // W, pix % W]


def test_reference_is_the_plain_convolution():
    """The residual segment and the pools of `reference`, spelled out per element for one output value."""
    c = cc.case("x", 3, 8, 4, 6, c2=4, stride2=2, pool=1)
    t = cc.make_inputs(c)
    ref = cc.reference(c, t)
    m, n, oy, ox = 2, 3, 4, 1
    acc = t.b[n].double()
    for ty in range(3):
        for tx in range(3):
            iy, ix = oy - 1 + ty, ox - 1 + tx
            if 0 <= iy < c.hin and 0 <= ix < c.win:
                win = t.x[m, :, 2 * iy:2 * iy + 2, 2 * ix:2 * ix + 2].double().sum(dim=(1, 2))
                acc = acc + (win * t.w[n, :, ty, tx].double()).sum()
    acc = acc + (t.x2[m, :, 2 * oy, 2 * ox].double() * t.w2[n, :, 0, 0].double()).sum()
    assert abs(float(ref[m, n, oy, ox]) - max(float(acc), 0.0)) <= 1e-12
    rows = cc.weight_rows(c, t)
    assert rows.shape == (4, 9 * 8 + 4) and rows[n, (1 * 3 + 2) * 8 + 5] == t.w[n, 5, 1, 2] and rows[n, 72 + 1] == t.w2[n, 1, 0, 0]


@pytest.mark.parametrize("cnn,M", cc.CALIBRATE, ids=["%s-M%d" % cm for cm in cc.CALIBRATE])
def test_last_agent_holds_every_layer_maximum(cnn, M):
    """The calibration test's input: row M - 1 - in the ragged last agent tile when M is 129 or 257 - attains the maximum of every
    absmax slot, so a pass that drops that tile cannot pass; and no maximum sits within 1e-4 of a power of two, so the device's
    float32 maximum and the float64 one must give the same scale exponent."""
    from magat_pathplanning_amd import encoder as enc
    ref = cc.encoder_reference(cnn, M)
    have = [s for s in range(cc.SLOTS_USED) if ref.per_agent[s] is not None]
    want = [0, 1, 2, 3, 4, 7] + ([5, 6] if cnn != cc.SLIM_MLP else []) + ([8] if cnn.endswith("_withMLP") else [])
    assert sorted(have) == sorted(want)
    for s in have:
        assert int(ref.per_agent[s].argmax()) == M - 1, (s, int(ref.per_agent[s].argmax()))
        v = ref.maxima[s]
        assert v > 0 and cc.distance_to_power_of_two(v) > 1e-4, (s, v)
        if M > 1:      # ... by a margin no rounding closes
            assert float(ref.per_agent[s][:M - 1].max()) < 0.99 * v, (s, v)
        assert enc.scale_exponent(v * (1 + 1e-4)) == enc.scale_exponent(v * (1 - 1e-4)) == enc.scale_exponent(v)


def test_scaled_pack_leaves_the_f16_range():
    """The re-run test's checkpoint: layer2.0.bn1 x 1e5 drives layer2's maps past 65504 (the f16 planes clamp, the guard re-runs)."""
    ref = cc.encoder_reference(cc.LARGE_MLP, 129, True)
    assert ref.maxima[cc.slot_conv1(1)] > 65504.0 and ref.maxima[cc.SLOT_STEM] < 100.0
    plain = cc.encoder_reference(cc.LARGE_MLP, 129, False)
    assert max(v for v in plain.maxima if v is not None) < 4094.0
    rows = cc.rerun_walk_rows()
    assert rows.numel() == cc.RERUN_WALK and rows.numel() * (128 // 4) > 512 * 256 and int(rows.max()) == 256


def test_cast_source_has_the_specials():
    for M, width, ld_src, ld_dst in cc.CAST:
        x = cc.cast_source(M, width)
        bits = x.view(torch.int32)
        n = len(cc.SPECIAL_BITS)
        assert [int(b) & 0xffffffff for b in bits[0, :n]] == list(cc.SPECIAL_BITS)
        assert [int(b) & 0xffffffff for b in bits[M - 1, width - n:]] == list(cc.SPECIAL_BITS)
        assert int(torch.isnan(x).sum()) == 2 * len(cc.NAN_BITS) and width % 4 == 0 and ld_src > width and ld_dst > width
    assert cc.CAST[1][0] * (cc.CAST[1][1] // 4) > 8192 * 256
