"""GPU parity of the individual gfx950 kernels, called through the C ABI (ctypes), against fp64
torch references and the reference-made golden vectors."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as tnf

from conftest import golden_paths, load_layer_fixture

pytestmark = pytest.mark.gpu

LAYER = golden_paths("gat_")


def _nat():
    from magat_pathplanning_amd import _native as nat
    return nat, nat.lib()


@pytest.mark.parametrize("M,N,K,relu", [(300, 128, 128, 0), (1000, 2048, 128, 0), (257, 5, 640, 0),
                                        (130, 64, 96, 1), (64, 32, 1152, 1), (5, 128, 36, 1)])
def test_linear_f32(gpu_device, M, N, K, relu):
    nat, lib = _nat()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ref = x.double() @ w.double().t() + b.double()
    if relu:
        ref = ref.clamp_min(0)
    xd, wd, bd = x.to(gpu_device), w.to(gpu_device), b.to(gpu_device)
    y = torch.full((M, N), float("nan"), device=gpu_device)
    nat.check(lib.magat_linear_f32(nat.ptr(xd), K, nat.ptr(wd), nat.ptr(bd), nat.ptr(y), N, M, N, K, relu,
                                   nat.current_stream(gpu_device)), "linear")
    torch.cuda.synchronize()
    np.testing.assert_allclose(y.cpu().numpy(), ref.float().numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("M,K1,K2,N,relu", [(51200, 128, 512, 5, 0), (4099, 128, 0, 5, 1), (8192, 64, 36, 8, 0),
                                            (5000, 132, 128, 1, 0), (100, 128, 512, 5, 0)])
def test_skinny_layer_is_the_same_product(gpu_device, libopt, M, K1, K2, N, relu):
    """The action head's form (a 1x1 float32 layer with at most 8 outputs over [in | in2]) as streamed dot products (option
    SKINNY): against float64, bit-identical from run to run, the padding of wider row buffers untouched,
    and within float32 rounding of the MFMA-tile kernel it replaces (SKINNY=0)."""
    nat, lib = _nat()
    g = torch.Generator().manual_seed(M + K1 + K2 + N)
    ld1, ld2, ldc = K1 + 4, K2 + 8, N + 3
    x1 = torch.randn(M, ld1, generator=g).to(gpu_device)
    x2 = torch.randn(M, max(ld2, 4), generator=g).to(gpu_device)
    w = (torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5).to(gpu_device)
    b = torch.randn(N, generator=g).to(gpu_device)
    ref = torch.cat((x1[:, :K1], x2[:, :K2]), 1).double() @ w.double().t() + b.double()
    if relu:
        ref = ref.clamp_min(0)

    def run():
        y = torch.full((M, ldc), -3.0, device=gpu_device)
        d = nat.ConvGemmDesc()
        d.inp, d.Cin, d.lda = x1.data_ptr(), K1, ld1
        if K2:
            d.in2, d.C2, d.lda2, d.W2, d.stride2 = x2.data_ptr(), K2, ld2, 1, 1
        d.wt, d.bias, d.out = w.data_ptr(), b.data_ptr(), y.data_ptr()
        d.M, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad, d.Hout, d.Wout = M, 1, 1, 1, 1, 1, 0, 1, 1
        d.Cout, d.ldc, d.relu = N, ldc, relu
        nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "conv_gemm")
        torch.cuda.synchronize()
        return y

    libopt.set("SKINNY", 1)
    y1, y2 = run(), run()
    libopt.set("SKINNY", 0)
    y0 = run()
    assert torch.equal(y1, y2)
    assert bool((y1[:, N:] == -3.0).all())
    np.testing.assert_allclose(y1[:, :N].cpu().numpy(), ref.float().cpu().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(y1[:, :N].cpu().numpy(), y0[:, :N].cpu().numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("M,K1,K2,N,rows16", [(20000, 128, 512, 5, 2), (4099, 512, 0, 5, 1), (777, 64, 40, 3, 3),
                                              (100, 128, 512, 5, 2)])
def test_skinny_layer_reads_bf16_rows(gpu_device, M, K1, K2, N, rows16):
    """magat_conv_gemm_desc.bf16_rows: the action head's inputs as bf16 rows (the bf16-storage graph layer's result, read as
    it is) - against float64 over the same bf16 values, next to a float32 `in` where only `in2` is bf16; row strides wider
    than the rows; bit-identical from run to run.  Any other kernel refuses the flag."""
    nat, lib = _nat()
    g = torch.Generator().manual_seed(M + K1 + K2 + N)
    ld1, ld2, ldc = K1 + 8, K2 + 16, N + 1
    x1 = torch.randn(M, ld1, generator=g)
    x2 = torch.randn(M, max(ld2, 8), generator=g)
    if rows16 & 1:
        x1 = x1.to(torch.bfloat16)
    if rows16 & 2:
        x2 = x2.to(torch.bfloat16)
    x1, x2 = x1.to(gpu_device), x2.to(gpu_device)
    w = (torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5).to(gpu_device)
    b = torch.randn(N, generator=g).to(gpu_device)
    ref = torch.cat((x1[:, :K1].double(), x2[:, :K2].double()), 1) @ w.double().t() + b.double()

    def desc(y, cout=N):
        d = nat.ConvGemmDesc()
        d.inp, d.Cin, d.lda = x1.data_ptr(), K1, ld1
        if K2:
            d.in2, d.C2, d.lda2, d.W2, d.stride2 = x2.data_ptr(), K2, ld2, 1, 1
        d.wt, d.bias, d.out = w.data_ptr(), b.data_ptr(), y.data_ptr()
        d.M, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad, d.Hout, d.Wout = M, 1, 1, 1, 1, 1, 0, 1, 1
        d.Cout, d.ldc, d.relu, d.bf16_rows = cout, ldc, 0, rows16
        return d

    outs = []
    for _ in range(2):
        y = torch.full((M, ldc), -3.0, device=gpu_device)
        nat.check(lib.magat_conv_gemm_f32(ctypes.byref(desc(y)), nat.current_stream(gpu_device)), "conv_gemm")
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1]) and bool((outs[0][:, N:] == -3.0).all())
    np.testing.assert_allclose(outs[0][:, :N].cpu().numpy(), ref.float().cpu().numpy(), rtol=0, atol=2e-5)
    # a layer the streamed form does not take (32 outputs): the MFMA-tile kernels have no bf16 loader and say so
    wide = torch.empty(M, 32, device=gpu_device)
    d = desc(wide, 32)
    d.ldc = 32
    assert lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)) == -2      # MAGAT_ERR_UNSUPPORTED


def _to_pixel_major(t):           # (M,C,H,W) -> [H*W][M][C]
    M, C, H, W = t.shape
    return t.permute(2, 3, 0, 1).reshape(H * W, M, C).contiguous()


def _from_pixel_major(t, H, W):   # [H*W][M][C] -> (M,C,H,W)
    return t.reshape(H, W, t.shape[1], t.shape[2]).permute(2, 3, 0, 1).contiguous()


@pytest.mark.parametrize("cin,cout,hin,stride,c2", [(32, 32, 11, 2, 0), (32, 32, 6, 1, 32), (32, 64, 6, 1, 0),
                                                     (64, 64, 6, 1, 32), (64, 128, 6, 1, 0), (128, 128, 6, 1, 64)])
def test_conv_gemm_vs_conv2d(gpu_device, cin, cout, hin, stride, c2):
    """3x3 pad-1 conv (+ optional strided 1x1 residual branch as second K segment) + bias + ReLU."""
    nat, lib = _nat()
    M = 150
    g = torch.Generator().manual_seed(cin * cout + hin)
    hout = (hin + 2 - 3) // stride + 1
    x = torch.randn(M, cin, hin, hin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = tnf.conv2d(x.double(), w.double(), b.double(), stride, 1)
    wt = w.permute(0, 2, 3, 1).reshape(cout, -1)
    x2 = None
    if c2:
        # residual source has the resolution of the block input: use stride2 = 1 at the same map size
        x2 = torch.randn(M, c2, hout, hout, generator=g)
        w2 = torch.randn(cout, c2, 1, 1, generator=g) / c2 ** 0.5
        ref = ref + tnf.conv2d(x2.double(), w2.double())
        wt = torch.cat((wt, w2.reshape(cout, c2)), dim=1)
    ref = ref.clamp_min(0)
    xin = _to_pixel_major(x).to(gpu_device)
    wtd, bd = wt.contiguous().to(gpu_device), b.to(gpu_device)
    out = torch.full((hout * hout, M, cout), float("nan"), device=gpu_device)
    d = nat.ConvGemmDesc()
    d.inp, d.wt, d.bias, d.out = xin.data_ptr(), wtd.data_ptr(), bd.data_ptr(), out.data_ptr()
    d.in_pix_stride, d.out_pix_stride = M * cin, M * cout
    d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, hin, hin, 3, 3, stride, 1
    d.Hout, d.Wout, d.Cout, d.ldc, d.relu = hout, hout, cout, cout, 1
    if c2:
        x2d = _to_pixel_major(x2).to(gpu_device)
        d.in2, d.in2_pix_stride, d.C2, d.lda2, d.W2, d.stride2 = x2d.data_ptr(), M * c2, c2, c2, hout, 1
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "conv_gemm")
    torch.cuda.synchronize()
    got = _from_pixel_major(out.cpu(), hout, hout)
    np.testing.assert_allclose(got.numpy(), ref.float().numpy(), rtol=0, atol=3e-5)


@pytest.mark.parametrize("cin,cout,hin,dil,pool", [(32, 32, 11, 3, False), (64, 64, 5, 3, False), (32, 64, 11, 2, False),
                                                    (32, 64, 5, 1, True), (64, 128, 11, 3, True), (32, 32, 4, 3, False)])
def test_conv_gemm_dilated_vs_conv2d(gpu_device, cin, cout, hin, dil, pool):
    """ABI 8: nn.Conv2d(3 x 3, dilation = padding = d) + bias + ReLU on the float32 kernel (the dilated CNNs of
    DecentralPlannerNet: dilation 3 on 11 x 11 and 5 x 5 maps, where most taps of an edge pixel leave the map), also reading the
    2 x 2 max-pool of a physical map on load (`hin` is then the pooled size); the f16x3 kernels decline a dilated window."""
    nat, lib = _nat()
    M = 70
    g = torch.Generator().manual_seed(cin + 7 * cout + hin + dil)
    hphys = 2 * hin + 1 if pool else hin                  # (odd physical size: the last row / column falls out of the pool)
    xp = torch.randn(M, cin, hphys, hphys, generator=g)
    x = tnf.max_pool2d(xp, 2) if pool else xp
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = tnf.conv2d(x.double(), w.double(), b.double(), 1, dil, dil).clamp_min(0)
    wt = w.permute(0, 2, 3, 1).reshape(cout, -1).contiguous().to(gpu_device)
    xin = _to_pixel_major(xp).to(gpu_device)
    out = torch.full((hin * hin, M, cout), float("nan"), device=gpu_device)
    bd = b.to(gpu_device)
    d = nat.ConvGemmDesc()
    d.inp, d.wt, d.bias, d.out = xin.data_ptr(), wt.data_ptr(), bd.data_ptr(), out.data_ptr()
    d.in_pix_stride, d.out_pix_stride = M * cin, M * cout
    d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, hin, hin, 3, 3, 1, dil
    d.Hout, d.Wout, d.Cout, d.ldc, d.relu, d.dilation = hin, hin, cout, cout, 1, dil
    if pool:
        d.pool, d.pool_w = 2, hphys
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "conv_gemm")
    torch.cuda.synchronize()
    got = _from_pixel_major(out.cpu(), hin, hin)
    np.testing.assert_allclose(got.numpy(), ref.float().numpy(), rtol=0, atol=3e-5)
    if dil > 1:
        d.in_fmt = 4
        assert lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)) == -2      # MAGAT_ERR_UNSUPPORTED


@pytest.mark.parametrize("H", [11, 9, 18, 19, 27])
def test_conv_first(gpu_device, H):
    """(19 and 27: the 32 padded images of a workgroup exceed the LDS, the kernel walks row bands)"""
    nat, lib = _nat()
    M = 77
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(M, 3, H, H, generator=g) < 0.3).float()
    w = torch.randn(32, 3, 3, 3, generator=g)
    b = torch.randn(32, generator=g)
    ref = tnf.conv2d(x.double(), w.double(), b.double(), 1, 1).clamp_min(0)
    out = torch.full((H * H, M, 32), float("nan"), device=gpu_device)
    xd, wd, bd = x.to(gpu_device), w.reshape(32, 27).contiguous().to(gpu_device), b.to(gpu_device)
    nat.check(lib.magat_conv_first_f32(nat.ptr(xd), nat.ptr(wd), nat.ptr(bd), nat.ptr(out), M, H, H,
                                       nat.current_stream(gpu_device)), "conv_first")
    torch.cuda.synchronize()
    np.testing.assert_allclose(_from_pixel_major(out.cpu(), H, H).numpy(), ref.float().numpy(), rtol=0, atol=1e-5)


ONE_LAUNCH = "gat_layer (one launch)"


@pytest.mark.parametrize("want_att", [False, True], ids=["default_kernels", "with_attention"])
@pytest.mark.parametrize("path", LAYER, ids=[os.path.basename(p)[:-4] for p in LAYER])
def test_gat_layer_vs_reference_golden(gpu_device, tag_counts, path, want_att):
    """HIP GraphFilterBatchAttentional vs the outputs the real reference produced (tolerance: north star 1e-4;
    observed ~1e-6).  The fixtures' GSOs (oracle/make_golden.py tricky_gso) carry a directed edge pair, 5e-10 / -3e-9
    threshold entries, a NaN, an isolated node and float64 1/lambda_max values.  want_att=False is what inference runs by
    default - for the shapes the one-launch matrix-core kernel covers (magat_gat_one_launch_supported) the test asserts that it
    is the kernel that ran; want_att=True also materialises (and checks) the attention tensor, which takes the two-launch
    form."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    nat, lib = _nat()
    z, p = load_layer_fixture(path)
    mode, N, G, K, P = str(z["mode"]), int(z["N"]), int(z["G"]), int(z["K"]), int(z["P"])
    x = torch.from_numpy(z["x"]).to(gpu_device)
    S = torch.from_numpy(z["S"]).to(gpu_device)
    cls = GraphFilterBatchAttentional_Origin if mode == "GAT_origin" else GraphFilterBatchAttentional
    one_launch = bool(lib.magat_gat_one_launch_supported(N, G, G, K, nat._MODE_IDS[mode], 1))
    for concat, key in ((True, "y_concat"), (False, "y_mean")):
        layer = cls(G, G, K, P, 1, True, concatenate=concat, attentionMode=mode)
        layer.load_state_dict(p)
        layer = layer.to(gpu_device).eval()
        layer.return_attention = want_att
        layer.addGSO(S)
        with tag_counts() as tc, torch.no_grad():
            y = layer(x)
        torch.cuda.synchronize()
        assert tuple(y.shape) == tuple(z[key].shape)
        np.testing.assert_allclose(y.cpu().numpy(), z[key], rtol=0, atol=1e-5)
        if want_att:
            assert tc[ONE_LAUNCH] == 0
            np.testing.assert_allclose(layer.aij.cpu().numpy(), z["aij"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(layer.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)
        else:
            assert (tc[ONE_LAUNCH] > 0) == one_launch, (tc.counts, one_launch)
        if concat:
            nin = int(z["nin"])
            with tag_counts() as tc, torch.no_grad():
                yn = layer(x[:, :, :nin].contiguous())
            np.testing.assert_allclose(yn.cpu().numpy(), z["y_concat_nin"], rtol=0, atol=1e-5)
            if not want_att:
                assert (tc[ONE_LAUNCH] > 0) == one_launch, tc.counts


EDGE = golden_paths("edge_")
EDGE_ACT = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
            "leaky_relu": lambda t: torch.nn.functional.leaky_relu(t, 0.1), "identity": lambda t: t}


@pytest.mark.parametrize("want_att", [False, True], ids=["no_attention", "with_attention"])
@pytest.mark.parametrize("path", EDGE, ids=[os.path.basename(p)[:-4] for p in EDGE])
def test_gat_edge_features_and_nonlinearity_vs_reference_golden(gpu_device, path, want_att):
    """E > 1 edge features and nonlinearities other than ReLU (the layer's general path: one E = 1 pass of the HIP training-path
    kernels per edge feature over the union mask) vs the outputs of the real reference; all three attention modes, concat and
    mean, Nin < N, float32 and float64 directed GSOs per edge feature."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    z, p = load_layer_fixture(path)
    mode, N, G, K, P, E = str(z["mode"]), int(z["N"]), int(z["G"]), int(z["K"]), int(z["P"]), int(z["E"])
    act = EDGE_ACT[str(z["act"])]
    x = torch.from_numpy(z["x"]).to(gpu_device)
    S = torch.from_numpy(z["S"]).to(gpu_device)
    cls = GraphFilterBatchAttentional_Origin if mode == "GAT_origin" else GraphFilterBatchAttentional
    for concat, key in ((True, "y_concat"), (False, "y_mean")):
        layer = cls(G, G, K, P, E, True, nonlinearity=act, concatenate=concat, attentionMode=mode)
        layer.load_state_dict(p)
        layer = layer.to(gpu_device).eval()
        layer.return_attention = want_att
        layer.addGSO(S)
        with torch.no_grad():
            y = layer(x)
        assert tuple(y.shape) == tuple(z[key].shape)
        np.testing.assert_allclose(y.cpu().numpy(), z[key], rtol=0, atol=1e-5)
        if want_att:
            np.testing.assert_allclose(layer.aij.cpu().numpy(), z["aij"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(layer.returnAttentionGSO(), z["aij"].mean(axis=1), rtol=0, atol=2e-6)
        if concat:
            nin = int(z["nin"])
            with torch.no_grad():
                yn = layer(x[:, :, :nin].contiguous())
            np.testing.assert_allclose(yn.cpu().numpy(), z["y_concat_nin"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("path", [p for p in EDGE if "_E2_" in p or "_E3_" in p], ids=lambda p: os.path.basename(p)[:-4])
def test_gat_edge_features_backward_matches_oracle_autograd(gpu_device, path):
    """Gradients through the general path (parameter slices per edge feature + the HIP backward of every pass) against
    float64 autograd through the oracle restatement (pinned to these fixtures' forwards on the CPU)."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    from oracle import magat_oracle as orc
    z, p = load_layer_fixture(path)
    mode, G, K, P, E = str(z["mode"]), int(z["G"]), int(z["K"]), int(z["P"]), int(z["E"])
    act = EDGE_ACT[str(z["act"])]
    cls = GraphFilterBatchAttentional_Origin if mode == "GAT_origin" else GraphFilterBatchAttentional
    layer = cls(G, G, K, P, E, True, nonlinearity=act, concatenate=True, attentionMode=mode)
    layer.load_state_dict(p)
    layer = layer.to(gpu_device).train()
    S = torch.from_numpy(z["S"])
    x = torch.from_numpy(z["x"])
    g = torch.Generator().manual_seed(3)
    wgt = torch.randn(x.shape[0], P * G, x.shape[2], generator=g)
    xd = x.to(gpu_device).requires_grad_(True)
    layer.addGSO(S.to(gpu_device))
    (layer(xd) * wgt.to(gpu_device)).sum().backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    x64 = x.double().requires_grad_(True)
    y64, _ = orc.gat_layer_forward(x64, S.double(), p64, mode, True, nonlinearity=act)
    (y64 * wgt.double()).sum().backward()
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x64.grad.float().numpy(), rtol=0, atol=2e-4)
    for k, v in layer.named_parameters():
        want = p64[k].grad
        want = torch.zeros_like(p64[k]) if want is None else want
        scale = max(1.0, float(want.abs().max()))
        got = torch.zeros_like(v) if v.grad is None else v.grad          # (KeyQuery does not touch mixer / weight_bias)
        np.testing.assert_allclose(got.cpu().numpy(), want.float().numpy(), rtol=0, atol=2e-4 * scale, err_msg=k)


def test_gat_isolated_rows_are_exact_zero_not_nan(gpu_device):
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    layer = GraphFilterBatchAttentional(32, 32, 3, 2, attentionMode="KeyQuery").to(gpu_device).eval()
    layer.return_attention = True
    S = torch.zeros(2, 1, 9, 9, device=gpu_device)
    S[1, 0, 2, 4] = 0.5
    layer.addGSO(S)
    with torch.no_grad():
        y = layer(torch.randn(2, 32, 9, device=gpu_device))
    assert torch.isfinite(y).all()
    a = layer.aij
    assert float(a[0].abs().max()) == 0.0
    assert float(a[1, :, 0, 2, 4].min()) == 1.0 and float(a[1].sum()) == 2.0


def test_errors_are_loud(gpu_device):
    nat, lib = _nat()
    x = torch.zeros(4, 4, device=gpu_device)
    assert lib.magat_linear_f32(nat.ptr(x), 4, None, None, nat.ptr(x), 4, 4, 4, 4, 0, None) == -5
    assert lib.magat_gat_workspace_bytes(0, 4, 16, 16, 2, 1, 0, 1) == 0
    rc = lib.magat_gat_forward_packed_f32(nat.ptr(x), nat.ptr(x), 0, nat.ptr(x), None, nat.ptr(x), 16, None,
                                          nat.ptr(x), 16, 1, 4, 24, 24, 2, 1, 0, 1, None)
    assert rc == -2
    with pytest.raises(nat.MagatNativeError):
        nat.check(rc, "unsupported width")


@pytest.mark.parametrize("mode,concat,N,G,K,P", [("KeyQuery", True, 150, 128, 3, 4), ("KeyQuery", False, 200, 64, 2, 2),
                                                ("GAT_modified", True, 130, 32, 4, 3), ("KeyQuery", True, 40, 128, 3, 4),
                                                ("GAT_modified", False, 300, 128, 2, 4), ("KeyQuery", True, 64, 16, 1, 2),
                                                ("GAT_origin", True, 140, 64, 3, 4), ("GAT_origin", False, 50, 128, 2, 2)])
def test_gat_csr_path_vs_oracle(gpu_device, mode, concat, N, G, K, P):
    """Large-graph (CSR) kernels against the pinned dense oracle; N <= 128 cases force the CSR entry point."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    from magat_pathplanning_amd.graphml import dense_gso_to_csr, gat_forward_rows_csr, _csr_attention_to_dense
    from magat_pathplanning_amd.synthetic import comm_gso
    from oracle import magat_oracle as orc
    B = 3
    g = torch.Generator().manual_seed(N + G)
    origin = mode == "GAT_origin"
    layer = (GraphFilterBatchAttentional_Origin if origin else GraphFilterBatchAttentional)(
        G, G, K, P, concatenate=concat, attentionMode=mode)
    with torch.no_grad():
        if not origin:
            layer.weight_bias.uniform_(-0.3, 0.3, generator=g)
    x = torch.randn(B, G, N, generator=g) * 0.7
    S = comm_gso(B, N, int(8 * N ** 0.5), seed=N, dtype=torch.float64)
    S[0, 5, :] = 0                     # a row without edges
    S[0, :, 7] = 0                     # a node nobody listens to
    S[1, 3, 9], S[1, 9, 3] = 0.5, 0.0  # asymmetric pair
    params = {k: v.detach() for k, v in layer.state_dict().items()}
    y_ref, a_ref = orc.gat_layer_forward(x, S.unsqueeze(1), params, mode, concat)
    layer = layer.to(gpu_device).eval()
    X = x.permute(0, 2, 1).contiguous().to(gpu_device)
    rowptr, colidx, nnz = dense_gso_to_csr(S.to(gpu_device), self_loops=origin)
    S_eff = S.float().double() + torch.eye(N, dtype=torch.float64) if origin else S
    assert nnz == int((S_eff.abs() > 1e-9).sum())
    with torch.no_grad():
        out, att = gat_forward_rows_csr(X, rowptr, colidx, nnz, layer, want_attention=True)
    torch.cuda.synchronize()
    y = out.reshape(B, N, -1).permute(0, 2, 1).cpu()
    np.testing.assert_allclose(y.numpy(), y_ref.numpy(), rtol=0, atol=2e-5)
    if K > 1:
        dense = _csr_attention_to_dense(att, rowptr, colidx, nnz, B, N, P).cpu()
        np.testing.assert_allclose(dense.numpy(), a_ref.numpy(), rtol=0, atol=3e-6)


def test_gat_module_switches_to_csr_for_large_graphs(gpu_device):
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.synthetic import comm_gso
    from oracle import magat_oracle as orc
    B, N, G = 2, 1000, 128
    layer = GraphFilterBatchAttentional(G, G, 2, 4, attentionMode="KeyQuery")
    x = torch.randn(B, G, N, generator=torch.Generator().manual_seed(1)) * 0.5
    S = comm_gso(B, N, 160, seed=2)
    y_ref, _ = orc.gat_layer_forward(x, S.unsqueeze(1), {k: v.detach() for k, v in layer.state_dict().items()},
                                     "KeyQuery", True)
    layer = layer.to(gpu_device).eval()
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        y = layer(x.to(gpu_device))
    np.testing.assert_allclose(y.cpu().numpy(), y_ref.numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("mode,concat", [("KeyQuery", True), ("GAT_modified", False)])
def test_gat_mixed_density_batch_list_and_dense_kernels(gpu_device, mode, concat):
    """One batch holding sparse instances (list kernel), fully connected ones (over the LDS list capacity ->
    dense-tile kernel) and an empty graph: every instance must match the oracle, attention included."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.synthetic import comm_gso, random_gso
    from oracle import magat_oracle as orc
    N, G, K, P = 100, 128, 3, 4
    g = torch.Generator().manual_seed(11)
    S = torch.cat((comm_gso(3, N, 50, seed=5), random_gso(2, N, 1.0, seed=6), torch.zeros(1, N, N),
                   random_gso(2, N, 0.5, seed=7), comm_gso(1, N, 30, seed=8)), dim=0)
    B = S.shape[0]
    layer = GraphFilterBatchAttentional(G, G, K, P, concatenate=concat, attentionMode=mode)
    with torch.no_grad():
        layer.weight_bias.uniform_(-0.3, 0.3, generator=g)
    x = torch.randn(B, G, N, generator=g) * 0.5
    y_ref, a_ref = orc.gat_layer_forward(x, S.unsqueeze(1), {k: v.detach() for k, v in layer.state_dict().items()},
                                         mode, concat)
    layer = layer.to(gpu_device).eval()
    layer.return_attention = True
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        y = layer(x.to(gpu_device))
    np.testing.assert_allclose(y.cpu().numpy(), y_ref.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(layer.aij.cpu().numpy(), a_ref.numpy(), rtol=0, atol=3e-6)


@pytest.mark.parametrize("mode,concat,N,G,K,P", [("KeyQuery", True, 12, 64, 3, 2), ("KeyQuery", False, 20, 128, 2, 4),
                                                ("GAT_modified", True, 9, 32, 4, 3), ("KeyQuery", True, 30, 16, 1, 2),
                                                ("GAT_modified", False, 40, 128, 3, 2), ("GAT_origin", True, 14, 32, 3, 4),
                                                ("GAT_origin", False, 25, 64, 2, 2)])
def test_gat_training_backward_matches_autograd(gpu_device, mode, concat, N, G, K, P):
    """HIP training forward/backward of the layer vs float64 autograd of the composite (same algebra as the pinned
    oracle) on CPU: output, dx and every parameter gradient."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    from magat_pathplanning_amd.graphml import _composite
    from magat_pathplanning_amd.synthetic import comm_gso
    B = 3
    g = torch.Generator().manual_seed(N * 7 + G)
    origin = mode == "GAT_origin"
    cls = GraphFilterBatchAttentional_Origin if origin else GraphFilterBatchAttentional
    ref = cls(G, G, K, P, concatenate=concat, attentionMode=mode).double()
    with torch.no_grad():
        if not origin:
            ref.weight_bias.uniform_(-0.3, 0.3, generator=g)
    x = (torch.randn(B, G, N, generator=g) * 0.6).double().requires_grad_(True)
    S = comm_gso(B, N, max(6, int(4 * N ** 0.5)), seed=N, dtype=torch.float64)
    S[0, 2, :] = 0
    S[1, 3, 5], S[1, 5, 3] = 0.7, 0.0
    wgt = torch.randn(B, P * G if concat else G, N, generator=g).double()
    y_ref, _ = _composite(ref, x, S.unsqueeze(1))
    (y_ref * wgt).sum().backward()
    layer = cls(G, G, K, P, concatenate=concat, attentionMode=mode)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer = layer.to(gpu_device).train()
    xg = x.detach().float().to(gpu_device).requires_grad_(True)
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    y = layer(xg)
    (y * wgt.float().to(gpu_device)).sum().backward()
    torch.cuda.synchronize()

    def close(a, b, what):
        a, b = a.detach().cpu().double(), b.detach().double()
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-4 * scale, (what, float((a - b).abs().max()), scale)

    close(y, y_ref, "y")
    close(xg.grad, x.grad, "dx")
    names = ["filterWeight", "bias"] + (["weight"] if K > 1 or origin else [])
    if mode == "GAT_modified" and K > 1:
        names += ["mixer", "weight_bias"]
    if origin and K > 1:
        names += ["mixer"]
    for n_ in names:
        close(getattr(layer, n_).grad, getattr(ref, n_).grad, n_)


GRAD = golden_paths("grad_")


def _grad_fixture_layer(z, device, dtype):
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    mode, concat = str(z["mode"]), bool(int(z["concat"]))
    G, K, P = int(z["G"]), int(z["K"]), int(z["P"])
    cls = GraphFilterBatchAttentional_Origin if mode == "GAT_origin" else GraphFilterBatchAttentional
    layer = cls(G, G, K, P, concatenate=concat, attentionMode=mode)
    layer.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p_")})
    return layer.to(device=device, dtype=dtype)


@pytest.mark.parametrize("path", GRAD, ids=[os.path.basename(p)[5:-4] for p in GRAD])
def test_gat_training_backward_vs_reference_made_gradients(gpu_device, path):
    """the HIP training forward / backward of the layer against gradients produced by the REAL
    reference's autograd (oracle/make_golden.py --grad: GraphFilterBatchAttentional(_Origin) of utils/graphUtils/graphML.py
    in float64, loss.backward() as in agents/decentralplannerlocal_OnlineExpert_GAT.py:560-567) over directed GSOs: y,
    dL/dx and every parameter gradient within 2e-4 of the gradient's scale.  (The float64-composite check above stays as
    the second gate; tests/test_host.py pins that composite to these same vectors on the CPU.)"""
    z = np.load(path, allow_pickle=False)
    layer = _grad_fixture_layer(z, gpu_device, torch.float32).train()
    xg = torch.from_numpy(z["x"]).to(gpu_device).requires_grad_(True)
    layer.addGSO(torch.from_numpy(z["S"]).to(gpu_device))
    y = layer(xg)
    (y * torch.from_numpy(z["wgt"]).to(gpu_device)).sum().backward()
    torch.cuda.synchronize()

    def close(a, b, what):
        a, b = a.detach().cpu().double(), torch.from_numpy(b).double()
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-4 * scale, (what, float((a - b).abs().max()), scale)

    close(y, z["y"], "y")
    close(xg.grad, z["dx"], "dx")
    for k in z.files:
        if k.startswith("g_"):
            got = getattr(layer, k[2:]).grad
            if got is None:                      # a parameter the mode does not use: the reference's gradient is zero too
                assert not np.any(z[k]), k
            else:
                close(got, z[k], k)


def test_gat_training_backward_stress_poisoned_buffers(gpu_device):
    """`test_gat_training_backward_matches_autograd[GAT_modified-False-40-128-3-2]` once failed (dx off by
    2e-2 on a few rows) in about forty suite runs.  500 forward + backward passes of that parametrisation, every one checked
    against the float64 autograd reference AND bit-for-bit against the first, with the allocator churned through NaN- and
    1e30-filled blocks before each pass (an uninitialised read cannot hide behind zeros) and a fresh module every other pass
    (first-call paths: weight packing, workspaces).  Since round 3 both dense products of the backward run on the library's
    own float32 GEMM (deterministic tile order) instead of the BLAS library."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.graphml import _composite
    from magat_pathplanning_amd.synthetic import comm_gso
    mode, concat, N, G, K, P, B = "GAT_modified", False, 40, 128, 3, 2, 3
    g = torch.Generator().manual_seed(N * 7 + G)
    ref = GraphFilterBatchAttentional(G, G, K, P, concatenate=concat, attentionMode=mode).double()
    with torch.no_grad():
        ref.weight_bias.uniform_(-0.3, 0.3, generator=g)
    x = (torch.randn(B, G, N, generator=g) * 0.6).double().requires_grad_(True)
    S = comm_gso(B, N, max(6, int(4 * N ** 0.5)), seed=N, dtype=torch.float64)
    S[0, 2, :] = 0
    S[1, 3, 5], S[1, 5, 3] = 0.7, 0.0
    wgt = torch.randn(B, G, N, generator=g).double()
    y_ref, _ = _composite(ref, x, S.unsqueeze(1))
    (y_ref * wgt).sum().backward()
    want = {"y": y_ref.detach(), "dx": x.grad}
    want.update({n: p.grad for n, p in ref.named_parameters()})
    sd = {k: v.float() for k, v in ref.state_dict().items()}
    Sd, wd, x0 = S.unsqueeze(1).to(gpu_device), wgt.float().to(gpu_device), x.detach().float().to(gpu_device)
    layer, first = None, None
    for r in range(500):
        junk = [torch.full((1 << 18,), float("nan"), device=gpu_device) for _ in range(3)]
        junk += [torch.full((64 << (i % 11),), float("nan") if (i + r) % 3 else 1e30, device=gpu_device) for i in range(44)]
        del junk
        if r % 2 == 0:
            layer = GraphFilterBatchAttentional(G, G, K, P, concatenate=concat, attentionMode=mode)
            layer.load_state_dict(sd)
            layer = layer.to(gpu_device).train()
            layer.addGSO(Sd)
        layer.zero_grad()
        xg = x0.clone().requires_grad_(True)
        y = layer(xg)
        (y * wd).sum().backward()
        got = {"y": y.detach(), "dx": xg.grad}
        got.update({n: p.grad for n, p in layer.named_parameters()})
        got = {k: v.clone() for k, v in got.items()}
        if first is None:
            first = got
            for k, v in got.items():
                scale = max(1.0, float(want[k].abs().max()))
                err = float((v.cpu().double() - want[k]).abs().max())
                assert err <= 2e-4 * scale, (k, err, scale)
        else:
            for k, v in got.items():
                assert torch.equal(v, first[k]), (r, k, float((v - first[k]).abs().max()))


@pytest.mark.parametrize("N,G,F,K", [(12, 64, 32, 3), (20, 128, 128, 2), (9, 32, 16, 4), (30, 16, 64, 1), (100, 128, 128, 3)])
def test_graph_filter_batch_backward_matches_autograd(gpu_device, N, G, F, K):
    """HIP training forward/backward of GraphFilterBatch (magat_gnn_backward_csr_f32 + two GEMMs) vs float64 autograd
    of the reference algebra (x @ S per hop, graphML.py:5485-5579) on CPU: y, dx, dweight, dbias.  The GSO has directed
    (asymmetric) entries, an isolated node and negative values, so the direction of the gradient hop is exercised."""
    from magat_pathplanning_amd import GraphFilterBatch
    from magat_pathplanning_amd.synthetic import comm_gso
    from oracle import magat_oracle as orc
    B = 3
    g = torch.Generator().manual_seed(N * 5 + F)
    ref = GraphFilterBatch(G, F, K).double()
    x = (torch.randn(B, G, N, generator=g) * 0.6).double().requires_grad_(True)
    S = comm_gso(B, N, max(6, int(4 * N ** 0.5)), seed=N, dtype=torch.float64)
    S[0, 2, :] = 0
    S[0, :, 2] = 0
    S[1, 3, 5], S[1, 5, 3] = 0.7, 0.0
    S[2, 1, 4], S[2, 4, 1] = -0.4, 0.2
    wgt = torch.randn(B, F, N, generator=g).double()
    Sd = S.float().double()                      # the layer multiplies by S.float() (:5562)
    z, y_ref = x, torch.einsum("bgn,fg->bfn", x, ref.weight[:, 0, 0])
    for k in range(1, K):
        z = torch.matmul(z, Sd)
        y_ref = y_ref + torch.einsum("bgn,fg->bfn", z, ref.weight[:, 0, k])
    y_ref = y_ref + ref.bias
    if K <= 3 and N <= 30:                       # the same algebra as the pinned oracle
        with torch.no_grad():
            want = orc.graph_filter_batch_forward(x.float(), S.unsqueeze(1), ref.weight.float(), ref.bias.float())
        assert float((want.double() - y_ref).abs().max()) < 1e-4
    (y_ref * wgt).sum().backward()
    layer = GraphFilterBatch(G, F, K)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer = layer.to(gpu_device).train()
    xg = x.detach().float().to(gpu_device).requires_grad_(True)
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    y = layer(xg)
    assert type(y.grad_fn).__name__ == "_GnnTrainFunctionBackward"          # the HIP function, not the composite
    (y * wgt.float().to(gpu_device)).sum().backward()
    torch.cuda.synchronize()
    for a, b, what in ((y, y_ref, "y"), (xg.grad, x.grad, "dx"), (layer.weight.grad, ref.weight.grad, "dweight"),
                       (layer.bias.grad, ref.bias.grad, "dbias")):
        a, b = a.detach().cpu().double(), b.detach().double()
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-4 * scale, (what, float((a - b).abs().max()), scale)
    # parameters only (input without grad), Nin < N padding
    layer.zero_grad()
    y2 = layer(x.detach().float().to(gpu_device)[:, :, :N - 2].contiguous())
    assert y2.shape == (B, F, N - 2)
    y2.sum().backward()
    assert layer.weight.grad is not None and float(layer.weight.grad.abs().sum()) > 0


def test_model_training_step_runs_on_gpu(gpu_device):
    """loss.backward() + optimizer step through DecentralPlannerGATNet in train() mode on the GPU: the GAT layer's
    forward/backward are the HIP kernels, CNN/MLPs are torch autograd; the loss must drop."""
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    torch.manual_seed(0)
    cfg = make_config(num_agents=12, nGraphFilterTaps=3, nAttentionHeads=2, bottleneckFeature=32,
                      bottleneckMode="BottomNeck_skipConcatGNN", device=str(gpu_device))
    net = DecentralPlannerGATNet(cfg).to(gpu_device).train()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    x, S = fov_states(6, 12, seed=1).to(gpu_device), comm_gso(6, 12, 14, seed=2).to(gpu_device)
    tgt = torch.randint(0, 5, (72,), device=gpu_device)
    losses = []
    for _ in range(12):
        net.addGSO(S)
        loss = torch.nn.functional.cross_entropy(net(x), tgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert net.GFL[0].filterWeight.grad is not None and float(net.GFL[0].filterWeight.grad.abs().sum()) > 0


BF16_LAYER = [p_ for p_ in LAYER if int(np.load(p_)["G"]) % 32 == 0]


@pytest.mark.parametrize("path", BF16_LAYER, ids=[os.path.basename(p)[:-4] for p in BF16_LAYER])
def test_gat_csr_bf16_storage(gpu_device, path):
    """bf16-STORAGE CSR kernels (BASELINE config 5, magat_gat_forward_csr_bf16) on the reference-made fixtures:
    (a) against the oracle's bf16-storage emulation (same rounding points) to ~1 bf16 ulp of the output scale,
    (b) against the reference's fp32 output within the bf16 error budget (2 % of the output scale),
    (c) attention (fp32 softmax of bf16-stored scores) against the reference's aij."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    from magat_pathplanning_amd.graphml import dense_gso_to_csr, gat_forward_rows_csr, _csr_attention_to_dense
    from oracle import magat_oracle as orc
    z, p = load_layer_fixture(path)
    mode, N, G, K, P = str(z["mode"]), int(z["N"]), int(z["G"]), int(z["K"]), int(z["P"])
    origin = mode == "GAT_origin"
    x = torch.from_numpy(z["x"])
    S = torch.nan_to_num(torch.from_numpy(z["S"]), nan=0.0)
    B = x.shape[0]
    cls = GraphFilterBatchAttentional_Origin if origin else GraphFilterBatchAttentional
    for concat, key in ((True, "y_concat"), (False, "y_mean")):
        layer = cls(G, G, K, P, 1, True, concatenate=concat, attentionMode=mode)
        layer.load_state_dict(p)
        layer = layer.to(gpu_device).eval()
        y_emul, a_emul = orc.gat_layer_forward_bf16_storage(x, S, p, mode, concat)
        X = x.permute(0, 2, 1).contiguous().to(gpu_device).to(torch.bfloat16)
        rowptr, colidx, nnz = dense_gso_to_csr(S.reshape(B, N, N).to(gpu_device), self_loops=origin)
        with torch.no_grad():
            out, att = gat_forward_rows_csr(X, rowptr, colidx, nnz, layer, want_attention=True)
        torch.cuda.synchronize()
        assert out.dtype == torch.bfloat16
        y = out.float().reshape(B, N, -1).permute(0, 2, 1).cpu()
        y_ref = torch.from_numpy(z[key])
        scale = float(y_ref.abs().max())
        assert float((y - y_emul).abs().max()) <= 2.0 ** -7 * scale, (float((y - y_emul).abs().max()), scale)
        assert float((y - y_ref).abs().max()) <= 2e-2 * scale, (float((y - y_ref).abs().max()), scale)
        if K > 1:
            dense = _csr_attention_to_dense(att, rowptr, colidx, nnz, B, N, P).cpu()
            np.testing.assert_allclose(dense.numpy(), a_emul.numpy(), rtol=0, atol=4e-3)
            np.testing.assert_allclose(dense.numpy(), np.nan_to_num(z["aij"]), rtol=0, atol=2e-2)


def test_gat_module_bf16_storage_switch(gpu_device):
    """layer.storage_dtype = torch.bfloat16 routes the module through the bf16 CSR kernels; output stays float32."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional
    from magat_pathplanning_amd.synthetic import comm_gso
    from oracle import magat_oracle as orc
    B, N, G, K, P = 2, 300, 128, 2, 4
    g = torch.Generator().manual_seed(5)
    layer = GraphFilterBatchAttentional(G, G, K, P, attentionMode="KeyQuery")
    x = torch.randn(B, G, N, generator=g) * 0.5
    S = comm_gso(B, N, 90, seed=8)
    params = {k: v.detach() for k, v in layer.state_dict().items()}
    y_ref, _ = orc.gat_layer_forward(x, S.unsqueeze(1), params, "KeyQuery", True)
    y_emul, _ = orc.gat_layer_forward_bf16_storage(x, S.unsqueeze(1), params, "KeyQuery", True)
    layer = layer.to(gpu_device).eval()
    layer.storage_dtype = torch.bfloat16
    layer.addGSO(S.unsqueeze(1).to(gpu_device))
    with torch.no_grad():
        y = layer(x.to(gpu_device))
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, P * G, N)
    scale = float(y_ref.abs().max())
    assert float((y.cpu() - y_emul).abs().max()) <= 2.0 ** -7 * scale
    assert float((y.cpu() - y_ref).abs().max()) <= 2e-2 * scale


GNN_FIX = golden_paths("gnn_")


@pytest.mark.parametrize("path", GNN_FIX, ids=[os.path.basename(p)[:-4] for p in GNN_FIX])
def test_graph_filter_batch_vs_reference_golden(gpu_device, path):
    """GraphFilterBatch (non-attentional GNN baseline) on the HIP CSR kernels against outputs of the
    reference class: GSO VALUES as edge weights (incl. f64 GSOs, |S| < 1e-9 entries, asymmetric pairs, isolated nodes),
    G != F, Nin < N zero padding."""
    from magat_pathplanning_amd import GraphFilterBatch
    z = np.load(path)
    layer = GraphFilterBatch(int(z["G"]), int(z["F"]), int(z["K"]))
    layer.load_state_dict({"weight": torch.from_numpy(z["p_weight"]), "bias": torch.from_numpy(z["p_bias"])})
    layer = layer.to(gpu_device).eval()
    x = torch.from_numpy(z["x"]).to(gpu_device)
    layer.addGSO(torch.from_numpy(z["S"]).to(gpu_device))
    with torch.no_grad():
        y = layer(x)
        torch.cuda.synchronize()
        np.testing.assert_allclose(y.cpu().numpy(), z["y"], rtol=0, atol=1e-5)
        nin = int(z["N"]) - 3
        from oracle import magat_oracle as orc
        xp = torch.cat((torch.from_numpy(z["x"])[:, :, :nin], torch.zeros(2, int(z["G"]), 3)), dim=2)
        want = orc.graph_filter_batch_forward(xp, torch.from_numpy(z["S"]), torch.from_numpy(z["p_weight"]),
                                              torch.from_numpy(z["p_bias"]))[:, :, :nin]
        got = layer(x[:, :, :nin].contiguous())
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("seed", [11, 12])
def test_persistent_dense_kernel_vs_csr_randomised(gpu_device, seed):
    """The persistent dense kernel (workgroups walking instances and heads with LDS-direct prefetch) against the
    independent CSR kernels on random shapes / densities / modes, plus run-to-run bit determinism: a race or a
    prefetch-ordering bug would show up here (tools/gat_stress.py is the long version)."""
    from magat_pathplanning_amd import GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin
    from magat_pathplanning_amd.graphml import dense_gso_to_csr, gat_forward_rows, gat_forward_rows_csr
    from magat_pathplanning_amd.synthetic import comm_gso, random_gso
    rng = np.random.default_rng(seed)
    for it in range(6):
        mode = ["KeyQuery", "GAT_modified", "GAT_origin"][int(rng.integers(0, 3))]
        G, N = int(rng.choice([64, 128])), int(rng.integers(40, 129))
        K, P, B = int(rng.integers(1, 5)), int(rng.choice([1, 2, 4])), int(rng.choice([8, 260, 300]))
        concat = bool(rng.integers(0, 2))
        cls = GraphFilterBatchAttentional_Origin if mode == "GAT_origin" else GraphFilterBatchAttentional
        layer = cls(G, G, K, P, concatenate=concat, attentionMode=mode).to(gpu_device).eval()
        X = torch.randn(B, N, G, device=gpu_device) * 0.6
        S = (comm_gso(B, N, int(6 * N ** 0.5), seed=int(rng.integers(1 << 30))) if it % 2 else
             random_gso(B, N, float(rng.choice([0.03, 0.3, 1.0])), seed=int(rng.integers(1 << 30)))).to(gpu_device)
        with torch.no_grad():
            ya = gat_forward_rows(X, S, layer)[0].clone()
            yb = gat_forward_rows(X, S, layer)[0].clone()
            rowptr, colidx, nnz = dense_gso_to_csr(S.contiguous(), self_loops=mode == "GAT_origin")
            yc = gat_forward_rows_csr(X, rowptr, colidx, nnz, layer)[0]
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), (mode, B, N, G, K, P)
        assert float((ya - yc).abs().max()) <= 5e-5 * max(1.0, float(yc.abs().max())), (mode, B, N, G, K, P, concat)


@pytest.mark.parametrize("cin,cout,c2,M,scale", [(64, 128, 0, 200, 1.0), (128, 128, 64, 131, 1.0), (32, 128, 32, 64, 1.0),
                                                 (32, 64, 0, 130, 1.0), (64, 64, 32, 77, 30.0), (32, 32, 32, 129, 1e-3),
                                                 (32, 32, 0, 40, 1.0), (64, 128, 0, 70, 3000.0)])
def test_conv_gemm_f16x3_split_mfma_matches_fp64(gpu_device, cin, cout, c2, M, scale):
    """f16x3 split-MFMA conv (in_fmt 4: two f16 planes per operand, three products, power-of-two weight scale) against an
    fp64 conv2d of the same fp32 inputs - same error bound as the fp32 MFMA / bf16x6 kernels; `scale` moves the
    activations to large (x30) and tiny (x1e-3: second plane partly subnormal) magnitudes."""
    from magat_pathplanning_amd.encoder import split_f16x2
    nat, lib = _nat()
    g = torch.Generator().manual_seed(cin + cout + c2 + 7)
    x = torch.randn(M, cin, 6, 6, generator=g) * scale
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    b = torch.randn(cout, generator=g) * scale
    ref = tnf.conv2d(x.double(), w.double(), b.double(), 1, 1)
    wt = w.permute(0, 2, 3, 1).reshape(cout, -1)
    d = nat.ConvGemmDesc()
    keep = [_to_pixel_major(x).to(gpu_device)]
    if c2:
        x2 = torch.randn(M, c2, 6, 6, generator=g) * scale
        w2 = torch.randn(cout, c2, 1, 1, generator=g) / c2 ** 0.5
        ref = ref + tnf.conv2d(x2.double(), w2.double())
        wt = torch.cat((wt, w2.reshape(cout, c2)), dim=1)
        keep.append(_to_pixel_major(x2).to(gpu_device))
        d.in2, d.in2_pix_stride, d.C2, d.lda2, d.W2, d.stride2 = keep[1].data_ptr(), M * c2, c2, c2, 6, 1
    ref = ref.clamp_min(0)
    blk, e = split_f16x2(wt.contiguous())
    ws, bd = blk.to(gpu_device), b.to(gpu_device)
    out = torch.full((36, M, cout), float("nan"), device=gpu_device)
    d.inp, d.wt, d.bias, d.out = keep[0].data_ptr(), ws.data_ptr(), bd.data_ptr(), out.data_ptr()
    d.in_pix_stride, d.out_pix_stride = M * cin, M * cout
    d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, 6, 6, 3, 3, 1, 1
    d.Hout, d.Wout, d.Cout, d.ldc, d.relu, d.in_fmt = 6, 6, cout, cout, 1, 4
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "conv_gemm f16x3")
    torch.cuda.synchronize()
    got = _from_pixel_major(out.cpu(), 6, 6)
    err = (got.double() - ref).abs().max().item()
    assert err <= 8e-6 * max(1.0, scale), (err, e)



@pytest.mark.gpu
def test_conv_gemm_f16x3_granule_layouts(gpu_device, monkeypatch, libopt):
    """Direct f16x3 kernel: float32 granule-major tiles (in_gl/out_gl = 1) are bit-identical to row-major tiles; f16
    plane granules (in_gl/out_gl = 2, K-permuted weights) agree to the rounding of the two output planes and of the
    MFMA's internal sum order.  Residual 1x1 segment (in2), ragged M (partial last agent tile)."""
    from magat_pathplanning_amd.encoder import split_f16x2
    nat, lib = _nat()
    M, cin, cout, c2, npix = 300, 64, 128, 32, 36
    Mp = (M + 127) // 128 * 128
    g = torch.Generator().manual_seed(11)
    x = torch.zeros(npix, Mp, cin); x[:, :M] = torch.relu(torch.randn(npix, M, cin, generator=g))
    x2 = torch.zeros(npix, Mp, c2); x2[:, :M] = torch.relu(torch.randn(npix, M, c2, generator=g))
    wt = (torch.randn(cout, 9 * cin + c2, generator=g) / (9 * cin) ** 0.5).contiguous()
    b = torch.randn(cout, generator=g)
    perm = torch.tensor([16 * (q >> 4) + 8 * ((q & 7) >> 2) + 4 * ((q >> 3) & 1) + (q & 3) for q in range(32)])

    def kidx(c):
        return (torch.arange(c) // 32) * 32 + perm.repeat(c // 32)

    def to_gl(t):
        return t.view(npix, Mp // 128, 128, t.shape[-1] // 4, 4).permute(0, 1, 3, 2, 4).contiguous()

    def from_gl(t, c):
        return t.view(npix, Mp // 128, c // 4, 128, 4).permute(0, 1, 3, 2, 4).reshape(npix, Mp, c)

    def to_pl(t):
        c = t.shape[-1]
        tp = t.clamp(-65504.0, 65504.0)[..., kidx(c)]
        h1 = tp.half()
        pl = torch.stack((h1, (tp - h1.float()).half()), dim=1)
        return pl.view(npix, 2, Mp // 128, 128, c // 8, 8).permute(0, 2, 1, 4, 3, 5).contiguous()

    def from_pl(buf, c):
        pl = buf.view(torch.float16).view(npix, Mp // 128, 2, c // 8, 128, 8).permute(0, 2, 1, 4, 3, 5)
        pl = pl.reshape(npix, 2, Mp, c)
        v = pl[:, 0].float() + pl[:, 1].float()
        out = torch.empty_like(v)
        out[..., kidx(c)] = v
        return out

    ws = split_f16x2(wt)[0].to(gpu_device)
    wsp = split_f16x2(wt[:, kidx(wt.shape[1])])[0].to(gpu_device)
    bd = b.to(gpu_device)
    res = {}
    for lay in (0, 1, 2):
        xi, x2i = ((x, x2), (to_gl(x), to_gl(x2)), (to_pl(x), to_pl(x2)))[lay]
        xi, x2i = xi.to(gpu_device), x2i.to(gpu_device)
        out = torch.full((npix, Mp, cout), float("nan"), device=gpu_device)
        d = nat.ConvGemmDesc()
        d.inp, d.in2, d.bias, d.out = xi.data_ptr(), x2i.data_ptr(), bd.data_ptr(), out.data_ptr()
        d.wt = (wsp if lay == 2 else ws).data_ptr()
        d.in_pix_stride, d.in2_pix_stride, d.out_pix_stride = Mp * cin, Mp * c2, Mp * cout
        d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, 6, 6, 3, 3, 1, 1
        d.C2, d.lda2, d.W2, d.stride2 = c2, c2, 6, 1
        d.Hout, d.Wout, d.Cout, d.ldc, d.relu, d.in_fmt, d.in_gl, d.out_gl = 6, 6, cout, cout, 1, 4, lay, lay
        nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)),
                  "conv_gemm granule layout %d" % lay)
        torch.cuda.synchronize()
        got = out.cpu()
        res[lay] = (got if lay == 0 else (from_gl(got, cout) if lay == 1 else from_pl(got, cout)))[:, :M]
    # float64 reference
    ref = torch.zeros(npix, M, cout, dtype=torch.float64)
    w64 = wt.double()
    for oy in range(6):
        for ox in range(6):
            acc = x2[oy * 6 + ox, :M].double() @ w64[:, 9 * cin:].T
            for ty in range(3):
                for tx in range(3):
                    iy, ix = oy - 1 + ty, ox - 1 + tx
                    if 0 <= iy < 6 and 0 <= ix < 6:
                        acc += x[iy * 6 + ix, :M].double() @ w64[:, (ty * 3 + tx) * cin:(ty * 3 + tx + 1) * cin].T
            ref[oy * 6 + ox] = torch.relu(acc + b.double())
    scale = float(ref.abs().max())
    assert not torch.isnan(res[0]).any()
    assert torch.equal(res[0], res[1])
    assert float((res[0].double() - ref).abs().max()) <= 3e-6 * scale
    assert float((res[2].double() - ref).abs().max()) <= 3e-6 * scale
    assert float((res[2] - res[0]).abs().max()) <= 3e-6 * scale


@pytest.mark.gpu
def test_conv_gemm_f16x3_direct_256_agent_tiles_ragged(gpu_device, monkeypatch, libopt):
    """The 256-agent-tile form of the direct kernel (TM = 2, taken when the grid is large) on a ragged agent count
    (14700 = 57 full tiles + 108 agents) is bit-identical to the 128-agent form, for float32 granules and f16 plane
    granules, row-major and granule outputs."""
    from magat_pathplanning_amd.encoder import split_f16x2
    nat, lib = _nat()
    M, cin, cout, c2, npix = 14700, 32, 128, 32, 36
    Mp = (M + 127) // 128 * 128
    g = torch.Generator().manual_seed(21)
    perm = torch.tensor([16 * (q >> 4) + 8 * ((q & 7) >> 2) + 4 * ((q >> 3) & 1) + (q & 3) for q in range(32)])

    def kidx(c):
        return (torch.arange(c) // 32) * 32 + perm.repeat(c // 32)

    def to_pl(t):
        c = t.shape[-1]
        tp = t.clamp(-65504.0, 65504.0)[..., kidx(c).to(t.device)]
        h1 = tp.half()
        pl = torch.stack((h1, (tp - h1.float()).half()), dim=1)
        return pl.view(npix, 2, Mp // 128, 128, c // 8, 8).permute(0, 2, 1, 4, 3, 5).contiguous()

    x = torch.zeros(npix, Mp, cin, device=gpu_device)
    x[:, :M] = torch.relu(torch.randn(npix, M, cin, generator=g)).to(gpu_device)
    x2 = torch.zeros(npix, Mp, c2, device=gpu_device)
    x2[:, :M] = torch.relu(torch.randn(npix, M, c2, generator=g)).to(gpu_device)
    wt = (torch.randn(cout, 9 * cin + c2, generator=g) / (9 * cin) ** 0.5).contiguous()
    wsp = split_f16x2(wt[:, kidx(wt.shape[1])])[0].to(gpu_device)
    bd = torch.randn(cout, generator=g).to(gpu_device)
    xi, x2i = to_pl(x), to_pl(x2)
    outs = {}
    for out_gl in (0, 2):
        for env in ({"MAGAT_CONV_TM": "1"}, {}):
            for k, v in env.items():
                libopt.set(k, v)
            out = torch.full((npix, Mp, cout), 7.0, device=gpu_device)
            d = nat.ConvGemmDesc()
            d.inp, d.in2, d.wt, d.bias, d.out = xi.data_ptr(), x2i.data_ptr(), wsp.data_ptr(), bd.data_ptr(), out.data_ptr()
            d.in_pix_stride, d.in2_pix_stride, d.out_pix_stride = Mp * cin, Mp * c2, Mp * cout
            d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, 6, 6, 3, 3, 1, 1
            d.C2, d.lda2, d.W2, d.stride2 = c2, c2, 6, 1
            d.Hout, d.Wout, d.Cout, d.ldc, d.relu, d.in_fmt, d.in_gl, d.out_gl = 6, 6, cout, cout, 1, 4, 2, out_gl
            nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "direct kernel %s" % env)
            torch.cuda.synchronize()
            for k in env:
                libopt.reset(k)
            outs[(out_gl, tuple(env))] = out
        ref = outs[(out_gl, ("MAGAT_CONV_TM",))]
        assert not torch.isnan(ref[:, :M]).any()
        if out_gl == 0:          # rows past M are never written
            assert bool((ref[:, M:] == 7.0).all())
        for key, got in outs.items():
            if key[0] == out_gl:
                assert torch.equal(got, ref), key


@pytest.mark.gpu
@pytest.mark.parametrize("M,cin,cout,hp", [(150, 128, 128, 3), (37, 64, 128, 2), (300, 128, 1152, 3)])
def test_conv_gemm_f32_per_pixel_weights_over_pooled_map(gpu_device, M, cin, cout, hp):
    """wt_pix_stride / ldw of magat_conv_gemm_desc: output pixel q of a 1x1 conv over the 2x2 sum-pooled map multiplies
    with its own slice [q*cin, (q+1)*cin) of rows that are hp*hp*cin floats long - the split-K form of the encoder head.
    The hp*hp partial products, summed, equal the one long-K GEMM of the same call without the split (and fp64)."""
    nat, lib = _nat()
    g = torch.Generator().manual_seed(M + cin + cout)
    hin = 2 * hp + (M & 1)                       # odd physical maps drop their last row / column (AvgPool2d floor)
    x = torch.relu(torch.randn(M, cin, hin, hin, generator=g))
    w = torch.randn(cout, hp * hp * cin, generator=g) / (hp * hp * cin) ** 0.5
    pooled = x[:, :, :2 * hp, :2 * hp].double().reshape(M, cin, hp, 2, hp, 2).sum(dim=(3, 5))       # (M, cin, hp, hp)
    flat = pooled.permute(0, 2, 3, 1).reshape(M, hp * hp, cin)
    ref_parts = torch.einsum("mqc,nqc->qmn", flat, w.double().view(cout, hp * hp, cin))
    xin = _to_pixel_major(x).to(gpu_device)
    wd = w.contiguous().to(gpu_device)
    part = torch.full((hp * hp, M, cout), float("nan"), device=gpu_device)
    d = nat.ConvGemmDesc()
    d.inp, d.wt, d.out = xin.data_ptr(), wd.data_ptr(), part.data_ptr()
    d.in_pix_stride, d.out_pix_stride = M * cin, M * cout
    d.M, d.Cin, d.lda, d.Hin, d.Win, d.kH, d.kW, d.stride, d.pad = M, cin, cin, hp, hp, 1, 1, 1, 0
    d.Hout, d.Wout, d.Cout, d.ldc, d.relu, d.pool, d.pool_w = hp, hp, cout, cout, 0, 1, hin
    d.wt_pix_stride, d.ldw = cin, hp * hp * cin
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)), "conv_gemm per-pixel weights")
    torch.cuda.synchronize()
    np.testing.assert_allclose(part.cpu().numpy(), ref_parts.float().numpy(), rtol=0, atol=3e-5)
    # the unsplit call: one output pixel, K = hp*hp*cin
    whole = torch.full((M, cout), float("nan"), device=gpu_device)
    d2 = nat.ConvGemmDesc()
    d2.inp, d2.wt, d2.out = xin.data_ptr(), wd.data_ptr(), whole.data_ptr()
    d2.in_pix_stride = M * cin
    d2.M, d2.Cin, d2.lda, d2.Hin, d2.Win, d2.kH, d2.kW, d2.stride, d2.pad = M, cin, cin, hp, hp, hp, hp, 1, 0
    d2.Hout, d2.Wout, d2.Cout, d2.ldc, d2.relu, d2.pool, d2.pool_w = 1, 1, cout, cout, 0, 1, hin
    nat.check(lib.magat_conv_gemm_f32(ctypes.byref(d2), nat.current_stream(gpu_device)), "conv_gemm pooled head")
    torch.cuda.synchronize()
    np.testing.assert_allclose(part.sum(0).cpu().numpy(), whole.cpu().numpy(), rtol=0, atol=3e-5)
    # misuse is refused: row stride shorter than the row, unaligned offsets, the split-MFMA formats
    d.ldw = cin - 4
    assert lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)) == -1      # MAGAT_ERR_BAD_SHAPE
    d.ldw, d.wt_pix_stride = hp * hp * cin, 6
    assert lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)) == -1      # MAGAT_ERR_BAD_SHAPE
    d.wt_pix_stride, d.in_fmt, d.pool = cin, 4, 0
    assert lib.magat_conv_gemm_f32(ctypes.byref(d), nat.current_stream(gpu_device)) == -2      # MAGAT_ERR_UNSUPPORTED


