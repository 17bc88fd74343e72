"""Cases, inputs and float64 references of the training-size tests of the CNN kernels (csrc/conv_train.hip through
train_cnn.py): tests/test_gpu_train_cnn_shapes.py runs them on the HIP kernels, tests/test_host_train_cnn.py checks on the
CPU that every case still enters the regime it is named for.

The host side of conv_train.hip cuts the weight gradient's contraction into agent ranges x groups of output pixels
(wgrad_chunks) and caps the BatchNorm grids (bn_blocks, the apply launches).  `wgrad_chunks` and `bn_blocks` below restate
that arithmetic in plain Python.  They LABEL cases - nothing is compared with a number they produce except the chunk and
workspace counts the library itself reports, which ties them to the code they mirror.

Every value handed to the device is a float32 value drawn on the CPU from a seeded generator; the references are torch's own
operators in float64 on the CPU over those values (conv2d and its autograd, torch.nn.functional.batch_norm)."""
import copy
import functools
import types

import torch
import torch.nn.functional as tnf

from test_gpu_train import GEOMS

STEM, L3 = GEOMS[0], GEOMS[6]          # (3, 32, 3, 1, 1, 11) and (128, 128, 3, 1, 1, 6)
OLD_M = (37, 45, 77, 150)              # the agent counts of tests/test_gpu_train.py
BN_THREADS, BN_REDUCE_CAP, BN_APPLY_CAP = 256, 512, 4096


# ---- the host-side work splits of csrc/conv_train.hip, restated ----------------------------------------------------------------
def wgrad_chunks(M, Cin, Cout, kH, kW, npix):
    """wgrad_chunks of conv_train.hip (Cin = the row width the kernel sees, a multiple of 4): cm agent ranges of mc agents x
    cpix groups of pc output pixels; last_pix / last_agents = the sizes of the last group / range; capped = `a > want` cut the
    number of ranges, so that a range is longer than 64 agents."""
    nco, nci = (2 if Cout % 64 == 0 else 1), (2 if Cin % 64 == 0 else 1)
    waves = (Cout // (32 * nco)) * ((Cin + 32 * nci - 1) // (32 * nci)) * kH * kW
    want = max(1, (4096 + waves - 1) // waves)
    a = (M + 63) // 64
    capped = a > want
    a = min(a, want)
    mc = ((M + a - 1) // a + 1) & ~1
    a = (M + mc - 1) // mc
    g = max(1, min((want + a - 1) // a, npix))
    pc = (npix + g - 1) // g
    g = (npix + pc - 1) // pc
    return types.SimpleNamespace(cm=a, mc=mc, cpix=g, pc=pc, last_pix=npix - (g - 1) * pc, last_agents=M - (a - 1) * mc,
                                 capped=capped, want=want)


def bn_blocks(rows, C):
    """bn_blocks of conv_train.hip and the grid of the apply launches: blocks of rows_per_block rows (the last one: last_rows),
    reduce_capped = the 512-block cap cut the grid (more than 8 rows per thread), apply_grid workgroups of 256 threads over
    rows * C / 4 channel quads, apply_capped = the 4096 cap cut it (the grid-stride loop takes a second trip)."""
    lanes = BN_THREADS // (C >> 2)
    b = (rows + lanes * 8 - 1) // (lanes * 8)
    reduce_capped = b > BN_REDUCE_CAP
    b = max(1, min(b, BN_REDUCE_CAP))
    rpb = (rows + b - 1) // b
    blocks = (rows + rpb - 1) // rpb
    grid = (rows * (C >> 2) + BN_THREADS - 1) // BN_THREADS
    return types.SimpleNamespace(blocks=blocks, rows_per_block=rpb, last_rows=rows - (blocks - 1) * rpb, lanes=lanes,
                                 reduce_capped=reduce_capped, apply_grid=min(grid, BN_APPLY_CAP), apply_capped=grid > BN_APPLY_CAP)


def _ceil4(c):
    return (c + 3) // 4 * 4


def hout(geom):
    cin, cout, k, s, p, H = geom
    return (H + 2 * p - k) // s + 1


def conv_chunks(M, geom):
    """The split of a GEOMS-style geometry as train_cnn._ConvPixelMajor hands it over (channels rounded up to 4)."""
    cin, cout, k, s, p, H = geom
    return wgrad_chunks(M, _ceil4(cin), cout, k, k, hout(geom) ** 2)


def mixed_groups(geom, split):
    """How many (pixel group, tap) pairs have the tap inside the map for some pixels of the group and outside for others: the
    waves in which the kernel's two `continue`s skip part of a group while the rest accumulates."""
    cin, cout, k, s, p, H = geom
    ho = hout(geom)
    n = 0
    for g in range(split.cpix):
        pix = range(g * split.pc, min((g + 1) * split.pc, ho * ho))
        for ty in range(k):
            for tx in range(k):
                inside = [0 <= (o // ho) * s - p + ty < H and 0 <= (o % ho) * s - p + tx < H for o in pix]
                n += any(inside) and not all(inside)
    return n


# ---- convolution cases ----------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _conv_case(route, M, geom, lda=None, ldc=None, pix_pad=0, **expect):
    cin, cout, k, s, p, H = geom
    return types.SimpleNamespace(route=route, M=M, geom=geom, lda=lda or _ceil4(cin), ldc=ldc or cout, pix_pad=pix_pad, expect=expect)


def _conv_cases():
    c = []
    # through _ConvPixelMajor (forward, dgrad, wgrad).  M = 333: a wave takes two pixels, the stem's last group has one
    c.append(_conv_case("function", 333, STEM, pc=2, last_pix=1))
    c.append(_conv_case("function", 333, L3, pc=2, last_pix=2))
    # M = 701: a short last group behind groups of three, groups of four, eleven agent ranges with a last one of 61 agents
    c.append(_conv_case("function", 701, STEM, pc=3, last_pix=1, cm=11, last_agents=61))
    c.append(_conv_case("function", 701, L3, pc=4, last_pix=4, cm=11, last_agents=61))
    # M = TRAIN_HIP_MIN_AGENTS + 3: what a training step runs; a last range of 3 agents (odd, shorter than an unrolled step of 8)
    for g in GEOMS:
        cin, cout, k, s, p, H = g
        e = dict(last_agents=3)
        if g == STEM:
            e.update(pc=9, last_pix=4)
        c.append(_conv_case("function", 2051, g, **e))
    # magat_conv_wgrad_f32 called directly.  Capped ranges: want = 29 < ceil(1901 / 64) = 30 -> 29 ranges of 66 agents
    c.append(_conv_case("direct", 1901, (256, 256, 3, 1, 1, 3), capped=True, mc=66, cm=29, cpix=1, pc=9))
    # row strides wider than the channel counts and pixel strides wider than M rows, NaN in everything the kernel must not read
    c.append(_conv_case("direct", 333, GEOMS[3], lda=40, ldc=72, pix_pad=1))
    out = {}
    for k in c:
        k.id = "%s-M%d-c%d_%d_k%d_s%d_p%d_h%d" % ((k.route, k.M) + tuple(k.geom)) + ("-strided" if k.pix_pad else "")
        assert k.id not in out
        k.seed = 3000 + len(out)
        k.split = conv_chunks(k.M, k.geom)
        out[k.id] = k
    return out


CONV_CASES = _conv_cases()
FUNCTION_CASES = [i for i, k in CONV_CASES.items() if k.route == "function"]
DIRECT_CASES = [i for i, k in CONV_CASES.items() if k.route == "direct"]
DETERMINISM_CASE = "function-M2051-c128_128_k3_s1_p1_h6"


def conv_inputs(cid):
    """x (M, Cin, H, H), w (Cout, Cin, k, k), dy-like weights wgt (M, Cout, Ho, Ho): float32 values, the same at every call."""
    k = CONV_CASES[cid]
    cin, cout, ks, s, p, H = k.geom
    g = _gen(k.seed)
    ho = hout(k.geom)
    return types.SimpleNamespace(case=k, x=torch.randn(k.M, cin, H, H, generator=g), w=torch.randn(cout, cin, ks, ks, generator=g) * 0.2,
                                 wgt=torch.randn(k.M, cout, ho, ho, generator=g))


def conv_result(r, dtype, device="cpu"):
    """torch's conv2d and its autograd on the inputs of a case in `dtype` on `device`: y, dX, dW for dY = wgt (a direct case:
    dW alone).  float64 on the CPU is the reference; float32 on the GPU is the error the gates are measured against."""
    cin, cout, ks, s, p, H = r.case.geom
    direct = r.case.route == "direct"
    x = r.x.to(device=device, dtype=dtype).requires_grad_(not direct)
    w = r.w.to(device=device, dtype=dtype).requires_grad_(True)
    y = tnf.conv2d(x, w, None, s, p)
    grads = torch.autograd.grad(y, (w,) if direct else (w, x), r.wgt.to(device=device, dtype=dtype))
    return types.SimpleNamespace(y=y.detach().cpu().double(), dw=grads[0].cpu().double(), dx=None if direct else grads[1].cpu().double())


@functools.lru_cache(maxsize=1)
def conv_reference(cid):
    """Inputs and float64 reference of a case; the latest one is kept (a 2051-agent case holds a few hundred MB)."""
    r = conv_inputs(cid)
    r.want = conv_result(r, torch.float64)
    return r


def pixel_major(t, ld=None, pix_pad=0, fill=0.0):
    """(M, C, H, W) -> [H*W][M + pix_pad][ld >= C] float32 with `fill` in every column and row that is padding; returns the
    buffer (hand its pointer on, pixel stride = (M + pix_pad) * ld floats)."""
    M, C, H, W = t.shape
    ld = ld or C
    out = torch.full((H * W, M + pix_pad, ld), fill, dtype=torch.float32)
    out[:, :M, :C] = t.permute(2, 3, 0, 1).reshape(H * W, M, C)
    return out


# ---- BatchNorm cases ------------------------------------------------------------------------------------------------------------
def _bn_case(rows, C, **expect):
    return types.SimpleNamespace(rows=rows, C=C, expect=expect, split=bn_blocks(rows, C), id="r%d_c%d" % (rows, C))


BN_CASES = {k.id: k for k in (
    # the row counts of a 2051-agent step: 121 pixels behind the stem, 36 from layer1 on - all past both caps
    _bn_case(2051 * 121, 32, reduce_capped=True, apply_capped=True),
    _bn_case(2051 * 36, 64, reduce_capped=True, apply_capped=True),
    _bn_case(2051 * 36, 128, reduce_capped=True, apply_capped=True),
    _bn_case(20000, 256, reduce_capped=True, apply_capped=True),
    _bn_case(40001, 128, reduce_capped=True, apply_capped=True, rows_per_block=79, last_rows=27),
    # small edges: fewer rows than row lanes, the narrowest and the widest channel counts
    _bn_case(2, 4, blocks=1), _bn_case(5, 8, blocks=1), _bn_case(1001, 256, reduce_capped=False, apply_capped=False))}


RELU_MARGIN = 1e-4


def bn_preactivation(x, gamma, beta, eps=1e-5):
    """(x - mean) * invstd * gamma + beta in float64 with the batch statistics of x: what the fused ReLU sees."""
    x = x.double()
    mean, var = x.mean(dim=0), x.var(dim=0, unbiased=False)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def bn_inputs(cid, relu):
    """Inputs of a case (float32 values).  With the ReLU fused, the few elements whose pre-activation lies within 2 x
    RELU_MARGIN of zero are moved away from it: at 8 million elements some would otherwise sit closer to the kink than float32 resolves,
    and the mask (so dx at that element) of a correct float32 evaluation would be a coin toss - not what these cases test."""
    k = BN_CASES[cid]
    g = _gen(4000 + k.rows + k.C + int(relu))
    x = torch.randn(k.rows, k.C, generator=g) * 1.7 + 0.4
    gamma, beta = torch.rand(k.C, generator=g) + 0.5, torch.randn(k.C, generator=g) * 0.3
    if relu:
        v = bn_preactivation(x, gamma, beta)
        near = v.abs() < 2 * RELU_MARGIN
        x[near] += (torch.where(v >= 0, 1.0, -1.0) * (16 * RELU_MARGIN)).float()[near]         # (dv/dx = gamma * invstd >= 0.25)
    return types.SimpleNamespace(case=k, relu=relu, x=x, gamma=gamma, beta=beta,
                                 rm=torch.randn(k.C, generator=g) * 0.1, rv=torch.rand(k.C, generator=g) + 0.5,
                                 wgt=torch.randn(k.rows, k.C, generator=g))


def bn_result(r, dtype, device="cpu"):
    """torch.nn.functional.batch_norm (+ relu) in training mode, momentum 0.1, eps 1e-5, and its autograd in `dtype` on
    `device`: y, dx, dgamma, dbeta and the running statistics after the step."""
    x, gamma, beta = (t.to(device=device, dtype=dtype).requires_grad_(True) for t in (r.x, r.gamma, r.beta))
    rm, rv = r.rm.to(device=device, dtype=dtype).clone(), r.rv.to(device=device, dtype=dtype).clone()
    y = tnf.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)
    y = torch.relu(y) if r.relu else y
    dx, dgamma, dbeta = torch.autograd.grad(y, (x, gamma, beta), r.wgt.to(device=device, dtype=dtype))
    return {n: t.detach().cpu().double() for n, t in (("y", y), ("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta),
                                                      ("running_mean", rm), ("running_var", rv))}


@functools.lru_cache(maxsize=1)
def bn_reference(cid, relu):
    r = bn_inputs(cid, relu)
    r.want = bn_result(r, torch.float64)
    return r


# ---- the ResNet trunk at training size --------------------------------------------------------------------------------------
TRUNK_RELU_MARGIN = 1e-4


def trunk_input(M, g):
    """(M, 3, 11, 11) field-of-view-like planes: obstacles / goals as 0-1 cells plus noise (tests/test_gpu_train.py)."""
    return (torch.rand(M, 3, 11, 11, generator=g) < 0.3).float() + 0.1 * torch.randn(M, 3, 11, 11, generator=g)


def trunk_inputs(M, seed=3):
    """nn.Sequential(ResNet()) with seeded weights, its input x and the weights wgt of loss = sum(y * wgt).

    BatchNorm: gamma in (0.5, 1), beta ~ N(3.5, 0.15).  A ReLU input is then negative for a couple of hundred of the 41 million
    elements of a 2051-agent batch (the masks are still exercised) and none lies within TRUNK_RELU_MARGIN of zero, so every
    correct float32 evaluation has the masks of the float64 reference.  With beta ~ N(0, 0.2) half of them are negative and the
    closest sits 5e-8 from zero: which masks flip then decides the gradient error, whatever computes the convolutions."""
    from magat_pathplanning_amd.resnet import ResNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        body = ResNet()
    g = _gen(seed + 1)
    with torch.no_grad():
        for m in body.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.0, generator=g)
                m.bias.normal_(3.5, 0.15, generator=g)
    x = trunk_input(M, g)
    return torch.nn.Sequential(body), x, torch.randn(M, 128, 3, 3, generator=g)          # (11 x 11 -> 6 x 6 -> pooled 3 x 3)


def trunk_relu_inputs(seq, x):
    """(smallest |v|, number of v < 0, number of v) over the inputs v of every ReLU call of the training-mode float64 forward."""
    net = copy.deepcopy(seq).double().train()
    rec = []
    for m in net.modules():
        if isinstance(m, torch.nn.ReLU):
            m.register_forward_pre_hook(lambda mod, inp: rec.append((float(inp[0].abs().min()), int((inp[0] < 0).sum()), inp[0].numel())))
    with torch.no_grad():
        net(x.double())
    return rec


def trunk_pass(seq, x, wgt, device, dtype, forward):
    """One training step's forward + backward of a copy of `seq`: y, dx, the gradient of every parameter, the buffers."""
    net = copy.deepcopy(seq).to(device=device, dtype=dtype).train()
    xg = x.to(device=device, dtype=dtype).requires_grad_(True)
    y = forward(net, xg)
    (y * wgt.to(device=device, dtype=dtype)).sum().backward()
    out = {"y": y.detach().cpu().double(), "dx": xg.grad.cpu().double()}
    out["params"] = {n: None if p.grad is None else p.grad.cpu().double() for n, p in net.named_parameters()}
    out["buffers"] = {n: b.detach().cpu().double() if b.dtype.is_floating_point else int(b) for n, b in net.named_buffers()}
    return out


# ---- gates ----------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """max|a - b| / max|b|: the error measure of tests/test_gpu_train.py"""
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def gate(existing, torch_f32_err):
    """The larger of the gate tests/test_gpu_train.py uses for the quantity and four times the error of torch's own float32
    operator on the same inputs against the same float64 reference: both are float32 sums in another order."""
    return max(existing, 4.0 * torch_f32_err)
