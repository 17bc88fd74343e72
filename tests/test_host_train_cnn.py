"""CPU-only checks around the training kernels of the per-agent CNN (csrc/conv_train.hip): the cases of
tests/test_gpu_train_cnn_shapes.py (tests/train_cnn_cases.py) keep the regime of the host-side work splits each was made for,
the Python restatement of those splits agrees with what the library itself reports, the shapes of tests/test_gpu_train.py
never leave one output pixel per wave - the reason the training-size cases exist - and the argument checks of
magat_conv_wgrad_f32 and magat_bn_train_{forward,backward}_f32 answer before anything touches a device."""
import ctypes

import pytest

import train_cnn_cases as tc

ERR_NULL, BAD_SHAPE, UNSUPPORTED = -5, -1, -2
ONE = ctypes.c_void_p(16)          # a non-null pointer no refused call may dereference


def _lib():
    from magat_pathplanning_amd import _native as nat
    return nat.lib()


def _wgrad_floats(M, geom, lib=None):
    cin, cout, k, s, p, H = geom
    return (lib or _lib()).magat_conv_wgrad_workspace_floats(M, tc._ceil4(cin), cin, cout, k, k, tc.hout(geom) ** 2)


# ---- the cases keep their regimes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(tc.CONV_CASES))
def test_convolution_case_keeps_the_regime_it_was_made_for(cid):
    k = tc.CONV_CASES[cid]
    s = k.split
    cin, cout, ks, st, p, H = k.geom
    for name, want in k.expect.items():
        assert getattr(s, name) == want, (name, getattr(s, name), want)
    # the restated split is the library's: its workspace is one weight tensor per chunk
    assert _wgrad_floats(k.M, k.geom) == s.cm * s.cpix * cout * ks * ks * cin
    assert (s.cm - 1) * s.mc < k.M <= s.cm * s.mc and s.mc % 2 == 0
    assert (s.cpix - 1) * s.pc < tc.hout(k.geom) ** 2 <= s.cpix * s.pc


def test_function_cases_take_more_than_one_pixel_per_wave_and_skip_taps_inside_a_group():
    for M, geoms in ((333, (tc.STEM, tc.L3)), (701, (tc.STEM, tc.L3)), (2051, tc.GEOMS)):
        for g in geoms:
            k = tc.CONV_CASES["function-M%d-c%d_%d_k%d_s%d_p%d_h%d" % ((M,) + tuple(g))]
            s = k.split
            if g[2] == 3:
                assert s.pc > 1, (M, g)
                assert s.pc in (3, 9) or M != 2051, (M, g, s.pc)
                # stride-2 and pad-1 taps fall outside the map for part of a group while the rest of it accumulates
                assert tc.mixed_groups(g, s) > 0, (M, g)
    stem = {M: tc.CONV_CASES["function-M%d-c3_32_k3_s1_p1_h11" % M].split for M in (333, 701, 2051)}
    assert all(0 < s.last_pix < s.pc for s in stem.values())          # a short last pixel group: 1 of 2, 1 of 3, 4 of 9
    assert (stem[2051].cm, stem[2051].cpix, stem[2051].pc, stem[2051].last_pix) == (33, 14, 9, 4)
    for cid in tc.FUNCTION_CASES:
        k = tc.CONV_CASES[cid]
        if k.M == 2051:           # an odd last agent range, shorter than one unrolled step of 8 agents
            assert k.split.last_agents < 8 and k.split.last_agents % 2 == 1, cid
    from magat_pathplanning_amd.train_cnn import TRAIN_HIP_MIN_AGENTS
    assert TRAIN_HIP_MIN_AGENTS + 3 == 2051


def test_direct_cases_reach_the_cap_and_the_strides_the_header_allows():
    cap = tc.CONV_CASES["direct-M1901-c256_256_k3_s1_p1_h3"]
    s = cap.split
    assert s.capped and s.mc > 64 and s.want == 29 < (cap.M + 63) // 64
    assert (s.cm, s.mc, s.cpix, s.pc) == (29, 66, 1, 9)
    st = tc.CONV_CASES["direct-M333-c32_64_k3_s1_p1_h6-strided"]
    assert st.lda == 40 > st.geom[0] and st.ldc == 72 > st.geom[1] and st.pix_pad > 0


def test_shapes_of_the_older_tests_never_leave_one_pixel_per_wave():
    """tests/test_gpu_train.py runs M = 37, 45, 77, 150: at every geometry a wave handles ONE output pixel (the pixel loop
    of wgrad_kernel runs once, no group is short, no tap is skipped inside a group), there are at most three agent ranges and
    the cap on their number is never reached; its largest BatchNorm input stays under both grid caps."""
    for M in tc.OLD_M:
        for g in tc.GEOMS:
            s = tc.conv_chunks(M, g)
            assert s.pc == 1 and s.last_pix == 1 and s.cm <= 3 and not s.capped, (M, g)
            assert tc.mixed_groups(g, s) == 0
            assert _wgrad_floats(M, g) == s.cm * s.cpix * g[1] * g[2] * g[2] * g[0]
    for rows, C in ((77 * 36, 32), (1001, 64), (23040, 128), (5, 128), (23040, 64)):
        b = tc.bn_blocks(rows, C)
        assert not b.reduce_capped and not b.apply_capped, (rows, C)


@pytest.mark.parametrize("cid", list(tc.BN_CASES))
def test_batchnorm_case_keeps_the_regime_it_was_made_for(cid):
    k = tc.BN_CASES[cid]
    b = k.split
    for name, want in k.expect.items():
        assert getattr(b, name) == want, (name, getattr(b, name), want)
    assert _lib().magat_bn_train_workspace_floats(k.rows, k.C) == b.blocks * 2 * k.C
    assert (b.blocks - 1) * b.rows_per_block < k.rows <= b.blocks * b.rows_per_block
    if k.expect.get("reduce_capped"):
        # more than 8 rows per thread in the reduction, and a second trip of the apply kernels' grid-stride loop
        assert b.blocks <= tc.BN_REDUCE_CAP and b.rows_per_block > 8 * b.lanes
        assert k.rows * k.C / 4 > tc.BN_APPLY_CAP * tc.BN_THREADS and b.apply_grid == tc.BN_APPLY_CAP
    else:
        assert b.rows_per_block <= 8 * b.lanes and k.rows * k.C / 4 <= tc.BN_APPLY_CAP * tc.BN_THREADS


@pytest.mark.parametrize("cid", list(tc.BN_CASES))
def test_batchnorm_relu_inputs_stay_clear_of_the_kink(cid):
    """No pre-activation of a fused-ReLU case lies within RELU_MARGIN of zero (float32 resolves 1e-7 there): every correct
    float32 evaluation has the mask of the float64 reference; the inputs are float32 values and both signs stay present."""
    import torch
    r = tc.bn_inputs(cid, True)
    assert r.x.dtype == torch.float32 and torch.isfinite(r.x).all()
    v = tc.bn_preactivation(r.x, r.gamma, r.beta)
    assert float(v.abs().min()) >= tc.RELU_MARGIN
    assert bool((v > 0).any()) and (bool((v < 0).any()) or r.case.rows < 8)


def test_batchnorm_cases_cover_the_channel_counts_the_kernel_claims():
    assert {k.C for k in tc.BN_CASES.values()} >= {4, 8, 32, 64, 128, 256}
    assert {(k.rows, k.C) for k in tc.BN_CASES.values()} >= {(248171, 32), (73836, 64), (73836, 128)}
    k = tc.BN_CASES["r40001_c128"].split
    assert (k.rows_per_block, k.last_rows) == (79, 27)
    # for every width both caps start at the same row count: rows > 2^22 / C
    for C in (32, 64, 128, 256):
        edge = (1 << 22) // C
        under, over = tc.bn_blocks(edge, C), tc.bn_blocks(edge + 1, C)
        assert not under.reduce_capped and not under.apply_capped and over.reduce_capped and over.apply_capped, C


def test_trunk_relu_inputs_stay_clear_of_the_kink():
    """The end-to-end case (TRAIN_HIP_MIN_AGENTS + 3 agents through the ResNet trunk): in the float64 reference no ReLU input
    lies within TRUNK_RELU_MARGIN of zero, some are negative (masks are exercised), and the trunk has the eleven convolutions
    whose weight-gradient launches the GPU test counts."""
    import torch
    from magat_pathplanning_amd.train_cnn import TRAIN_HIP_MIN_AGENTS
    seq, x, wgt = tc.trunk_inputs(TRAIN_HIP_MIN_AGENTS + 3)
    assert x.dtype == torch.float32 and x.shape == (2051, 3, 11, 11)
    rec = tc.trunk_relu_inputs(seq, x)
    assert len(rec) == 7                                       # stem + two per BasicBlock
    assert min(r[0] for r in rec) >= tc.TRUNK_RELU_MARGIN
    assert sum(r[1] for r in rec) >= 100 and sum(r[2] for r in rec) > 40_000_000
    assert sum(isinstance(m, torch.nn.Conv2d) for m in seq.modules()) == 11


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _wgrad(x=ONE, dy=ONE, part=ONE, chunks=True, M=64, Cin=32, cin_w=32, Cout=32, lda=None, ldc=None, H=6, Ho=6, k=3, stride=1,
           pad=1):
    n = ctypes.c_int(-7)
    lda, ldc = Cin if lda is None else lda, Cout if ldc is None else ldc
    rc = _lib().magat_conv_wgrad_f32(x, M * lda, lda, dy, M * ldc, ldc, part, ctypes.byref(n) if chunks else None, M, Cin,
                                     cin_w, Cout, H, H, Ho, Ho, k, k, stride, pad, None)
    assert n.value == -7            # a refused call leaves *chunks_out alone
    return rc


def test_wgrad_argument_checks_answer_before_anything_touches_a_device():
    f = _wgrad
    for name in ("x", "dy", "part"):
        assert f(**{name: None}) == ERR_NULL, name
    assert f(chunks=False) == ERR_NULL
    for name in ("M", "Cin", "cin_w", "Cout", "H", "Ho", "k", "stride"):
        assert f(**{name: 0}) == BAD_SHAPE and f(**{name: -3}) == BAD_SHAPE, name
    assert f(pad=-1) == BAD_SHAPE
    assert f(Cout=16) == BAD_SHAPE and f(Cout=48) == BAD_SHAPE and f(Cout=33) == BAD_SHAPE          # Cout % 32
    assert f(Cin=32, lda=31) == BAD_SHAPE and f(Cin=4, lda=3) == BAD_SHAPE                          # lda < Cin
    assert f(Cout=64, ldc=63) == BAD_SHAPE
    assert f(Cin=4, cin_w=5) == BAD_SHAPE and f(Cin=32, cin_w=33) == BAD_SHAPE                      # cin_w > Cin
    # null, then sizes
    assert f(x=None, Cout=16) == ERR_NULL and f(part=None, M=0) == ERR_NULL
    # the workspace of a refused shape is 0 floats (lda is no argument of it)
    w = _lib().magat_conv_wgrad_workspace_floats
    s = tc.wgrad_chunks(64, 32, 32, 3, 3, 36)
    assert w(64, 32, 32, 32, 3, 3, 36) == s.cm * s.cpix * 32 * 9 * 32 > 0
    for args in ((0, 32, 32, 32, 3, 3, 36), (-3, 32, 32, 32, 3, 3, 36), (64, 0, 32, 32, 3, 3, 36), (64, 32, 0, 32, 3, 3, 36),
                 (64, 32, 32, 0, 3, 3, 36), (64, 32, 32, 32, 0, 3, 36), (64, 32, 32, 32, 3, 0, 36), (64, 32, 32, 32, 3, 3, 0),
                 (64, 32, 32, 16, 3, 3, 36), (64, 32, 32, 48, 3, 3, 36), (64, 32, 32, 33, 3, 3, 36), (64, 4, 5, 32, 3, 3, 36),
                 (64, 32, 33, 32, 3, 3, 36)):
        assert w(*args) == 0, args


def _bn_forward(x=ONE, y=ONE, rows=64, C=32, gamma=ONE, beta=ONE, rm=ONE, rv=ONE, mean=ONE, invstd=ONE, ws=ONE, relu=0):
    return _lib().magat_bn_train_forward_f32(x, y, rows, C, gamma, beta, rm, rv, 0.1, 1e-5, relu, mean, invstd, ws, None)


def _bn_backward(x=ONE, y=ONE, dy=ONE, dx=ONE, rows=64, C=32, gamma=ONE, mean=ONE, invstd=ONE, relu=0, dgamma=ONE, dbeta=ONE,
                 ws=ONE):
    return _lib().magat_bn_train_backward_f32(x, y, dy, dx, rows, C, gamma, mean, invstd, relu, dgamma, dbeta, ws, None)


BN_BAD = [(dict(C=0), BAD_SHAPE), (dict(C=-4), BAD_SHAPE), (dict(C=6), BAD_SHAPE), (dict(C=30), BAD_SHAPE), (dict(C=260), BAD_SHAPE),
          (dict(C=512), BAD_SHAPE), (dict(C=12), UNSUPPORTED), (dict(C=24), UNSUPPORTED), (dict(C=96), UNSUPPORTED),
          (dict(rows=0), BAD_SHAPE), (dict(rows=-5), BAD_SHAPE)]


def test_batchnorm_forward_argument_checks_answer_before_anything_touches_a_device():
    f = _bn_forward
    for name in ("x", "y", "gamma", "beta", "mean", "invstd", "ws"):
        assert f(**{name: None}) == ERR_NULL, name
    for kw, want in BN_BAD:
        assert f(**kw) == want, kw
        assert f(rm=None, rv=None, **kw) == want, kw          # (the running statistics may be null: still the shape's answer)
    assert f(x=None, C=12) == ERR_NULL and f(rows=0, C=12) == BAD_SHAPE          # null, then sizes, then what is not covered


def test_batchnorm_backward_argument_checks_answer_before_anything_touches_a_device():
    f = _bn_backward
    for name in ("x", "dy", "dx", "gamma", "mean", "invstd", "dgamma", "dbeta", "ws"):
        assert f(**{name: None}) == ERR_NULL, name
    assert f(y=None, relu=1) == ERR_NULL          # the ReLU mask is read from y
    for kw, want in BN_BAD:
        assert f(**kw) == want, kw
        assert f(y=None, **kw) == want, kw        # (without ReLU y may be null)
    assert f(dx=None, C=12) == ERR_NULL and f(rows=0, C=12) == BAD_SHAPE


def test_batchnorm_workspace_is_zero_for_every_refused_shape():
    w = _lib().magat_bn_train_workspace_floats
    for kw, _ in BN_BAD:
        a = dict(rows=64, C=32)
        a.update(kw)
        assert w(a["rows"], a["C"]) == 0, kw
    for C in (4, 8, 16, 32, 64, 128, 256):
        assert w(64, C) == tc.bn_blocks(64, C).blocks * 2 * C > 0, C


def test_weight_gradient_tag_has_a_name():
    """MAGAT_TAG_CONV_WGRAD of include/magat_hip.h is in _native.TAGS: the tag_counts fixture reads only the tags listed there."""
    import os
    import re
    from magat_pathplanning_amd import _native as nat
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "magat_hip.h")).read()
    tag = int(re.search(r"#define MAGAT_TAG_CONV_WGRAD (\d+)", hdr).group(1))
    assert tag == 24 and nat.TAGS[tag] == "conv_wgrad"
    assert len(set(nat.TAGS.values())) == len(nat.TAGS)
