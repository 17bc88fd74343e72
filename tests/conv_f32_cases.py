"""Cases, layouts and float64 references of the tests of the float32 segmented-K MFMA kernel (csrc/conv_gemm_f32.hip) and of the
two encoder passes that run on it alone: magat_encoder_calibrate_f32 and the range guard's predicated re-run.
tests/test_gpu_conv_f32_forms.py runs them on the device; tests/test_host_conv_f32_cases.py checks on the CPU that the table
still reaches every kernel form it was made for.

Activations are channel-last rows per (pixel, agent) in one of two layouts:
  pixel-major  [pix][M][ld]                       pix_stride = M ld,    tile_stride = 0 (the kernel's default: 128 ld)
  tile-major   [ceil(M / 128)][pix][128][ld]      pix_stride = 128 ld,  tile_stride = npix 128 ld   (csrc/encoder_f32.hip)
Every padding column (ld > C) and every padding row of the last agent tile holds a poison value: NaN in what the kernel
reads - a loader that touched it would spoil the result - and 1e30 in what it writes, so that a stray store shows and an
`absmax` that looked at the padding would return it.

`tile_choice` and `is_full` restate two decisions of magat_conv_gemm_f32 (which tile template a shape gets, and whether the loader
without bounds checks serves it); the restatement is what lets a CPU-only run say that the table covers all twelve forms.

Gate (the one tests/test_gpu_kernels.py::test_conv_gemm_vs_conv2d holds this kernel to): 3e-5 max(1, max|reference|).
Encoder passes: 2e-5 max(1, |float64 value|), the figure of tests/test_gpu_model.py::test_encoder_other_map_sizes."""
import functools
import math
import types

import torch
import torch.nn.functional as tnf

GATE = 3e-5
ENC_GATE = 2e-5
POISON = 1.0e30
TILE_ROWS = 128
NUM_XCD = 8                # the block -> tile map hands whole agent tiles to the eight XCDs in turn
PIX, TILE = "pix", "tile"


# ---- the case table -----------------------------------------------------------------------------------------------------------
def case(id, M, cin, cout, hin, win=None, k=3, stride=1, pad=1, c2=0, stride2=1, pool=0, relu=1, layout=PIX, lda_x=0, lda2_x=0,
         ldc_x=0, ldw_x=0, mdraw=None):
    """hin x win: the map the taps walk (pool: the POOLED map; the physical one is (2 hin + 1) x (2 win + 1), odd on purpose: its
    last row and column fall out of every window).  c2 > 0: a 1 x 1 residual segment read from a second map of width w2 at
    stride2.  *_x: how much wider than its row a row stride is.  mdraw: agents drawn (cases that must share inputs)."""
    win = hin if win is None else win
    c = types.SimpleNamespace(id=id, M=M, cin=cin, cout=cout, hin=hin, win=win, k=k, stride=stride, pad=pad, c2=c2, stride2=stride2,
                              pool=pool, relu=relu, layout=layout, lda=cin + lda_x, lda2=c2 + lda2_x, ldc=cout + ldc_x,
                              mdraw=mdraw or M)
    c.hout, c.wout = (hin + 2 * pad - k) // stride + 1, (win + 2 * pad - k) // stride + 1
    c.hphys, c.wphys = (2 * hin + 1, 2 * win + 1) if pool else (hin, win)
    c.h2, c.w2 = (c.hout - 1) * stride2 + 1, (c.wout - 1) * stride2 + 1
    c.ktot = k * k * cin + c2
    c.ldw = c.ktot + ldw_x
    c.npix = c.hout * c.wout
    return c


def with_layout(c, layout, M=None):
    d = types.SimpleNamespace(**vars(c))
    d.layout, d.M = layout, (c.M if M is None else M)
    d.id = "%s-%s-M%d" % (c.id, layout, d.M)
    return d


STEP_A = dict(cin=32, cout=32, hin=11, stride=2)      # layer1.conv1: 11 x 11 -> 6 x 6
STEP_B = dict(cin=32, cout=64, hin=6)                 # layer2.conv1
STEP_C = dict(cin=64, cout=128, hin=6)                # layer3.conv1
RES_A = dict(cin=32, cout=32, hin=6, c2=32, stride2=2)      # layer1.conv2 as the float32 pass runs it: in2 is the 11 x 11 block input
RES_B = dict(cin=64, cout=64, hin=6, c2=32)                 # layer2.conv2
RES_C = dict(cin=128, cout=128, hin=6, c2=64)               # layer3.conv2

FORMS = (
    # the encoder's three steps at the edges of the BM = 128 tiles ...
    [case("stepA-M%d" % m, m, **STEP_A) for m in (128, 129, 256, 257)] +
    [case("stepB-M%d" % m, m, **STEP_B) for m in (128, 129, 256, 257)] +
    # ... and of the BM = 64 tile (Cout > 64 on a small grid)
    [case("stepC-M%d" % m, m, **STEP_C) for m in (64, 65, 128, 129)] +
    # the 128 x 128 tile of a large grid: 13 (14) agent tiles x 121 pixels >= 1536 workgroups; 1 x 1 keeps the reference cheap
    [case("grid128-M%d" % m, m, 32, 128, 11, k=1, pad=0) for m in (1664, 1665)] +
    # ragged channels: Cin = 36 leaves a 4-wide second slab per tap, C2 = 4, Cout one past each column tile (and 5 columns)
    [case("ragged-Cout%d" % n, 70, 36, n, 6, c2=4) for n in (5, 33, 65, 130)] +
    # weight rows, activation rows and output rows wider than what is read or written
    [case("ldw-full", 128, 32, 64, 6, c2=32, ldw_x=8),
     case("ldw-ragged", 77, 36, 33, 6, c2=4, ldw_x=12),
     case("ld-full", 128, 32, 64, 6, c2=32, lda_x=4, lda2_x=8, ldc_x=4),
     case("ld-full-odd-ldc", 128, 32, 64, 6, c2=32, lda_x=4, lda2_x=8, ldc_x=1),      # FULL loader, scalar stores
     case("ld-ragged", 129, 36, 65, 6, c2=4, lda_x=8, lda2_x=4, ldc_x=3)] +
    # agent tiles: 8 fill the first group of the XCD map, 9 and 17 open the second and the third
    [case("tiles128-M%d" % m, m, 32, 32, 2, k=1, pad=0) for m in (1024, 1030, 2176)] +
    [case("tiles64-M%d" % m, m, 32, 128, 2) for m in (512, 513, 1088)] +
    # geometry
    [case("rect-7x11", 129, 32, 32, 7, 11),
     case("rect-7x11-s2", 128, 32, 64, 7, 11, stride=2),
     case("even-12-s2", 129, 32, 32, 12, stride=2),
     case("valid-6x6-M64", 64, 32, 128, 6, k=6, pad=0, relu=0),      # the folded head: one output pixel, no padding
     case("valid-6x6-M65", 65, 32, 128, 6, k=6, pad=0, relu=0)] +
    # 2 x 2 pool on load: sum (the head's AvgPool2d, 1/4 in the weights) and max (the plain CNNs)
    [case("pool%d-M%d" % (p, m), m, 32, 128, 3, pool=p) for p in (1, 2) for m in (64, 65)] +
    [case("pool2-Cout32", 70, 32, 32, 5, pool=2),
     case("poolgrid-sum-M2048", 2048, 32, 512, 5, k=1, pad=0, pool=1),      # 16 tiles x 25 pixels x 4 column tiles = 1600
     case("poolgrid-max-M2049", 2049, 32, 512, 5, k=1, pad=0, pool=2)] +
    # the residual segment exactly as layer1.conv2 has it (W2 = 11, stride2 = 2), and four channels wide
    [case("res-l1conv2-M%d" % m, m, **RES_A) for m in (128, 129)] +
    [case("res-l1conv2-C2x4-M%d" % m, m, 32, 32, 6, c2=4, stride2=2) for m in (128, 129)]
)

# both layouts, M = 129 / 256 / 257 from one draw: bit-identical between the layouts, rows 0..255 between 256 and 257
TILE_MAJOR = [case(n, 257, mdraw=257, **kw) for n, kw in (("stepA", STEP_A), ("stepB", STEP_B), ("stepC", STEP_C),
                                                          ("resA", RES_A), ("resB", RES_B), ("resC", RES_C))]
TILE_MAJOR_M = (129, 256, 257)

# predicated launches: a grid that is launched whole (288 workgroups) and one that 512 workgroups walk (968 virtual tiles)
RUN_IF = [case("runif-6x6", 150, 32, 32, 6), case("runif-11x11", 150, 32, 32, 11)]

ABSMAX = [case("absmax-relu", 150, 32, 33, 6, ldc_x=3),
          case("absmax-negative", 150, 32, 33, 6, relu=0, ldc_x=3),
          case("absmax-full", 128, 32, 64, 6, relu=0, ldc_x=4),
          case("absmax-tile-major", 129, 32, 32, 6, c2=32, stride2=2, layout=TILE)]


def all_cases():
    out = list(FORMS) + list(RUN_IF) + list(ABSMAX)
    for c in TILE_MAJOR:
        out += [with_layout(c, lay, m) for m in TILE_MAJOR_M for lay in (PIX, TILE)]
    return out


# ---- two decisions of magat_conv_gemm_f32, restated ----------------------------------------------------------------------------
def tile_choice(c):
    """(BM, BN, pooled) of the tile template the dispatcher picks."""
    blocks128 = -(-c.M // 128) * c.npix * -(-c.cout // 128)
    small_grid = blocks128 < 1536
    if c.pool:
        return (64 if small_grid else 128, 128, True)
    if c.cout > 64:
        return (64 if small_grid else 128, 128, False)
    if c.cout > 32:
        return (128, 64, False)
    return (128, 32, False)


def strides(c, which):
    """(pix_stride, tile_stride) of the case's layout for `which` = in / in2 / out, as the descriptor takes them."""
    ld, npix = {"in": (c.lda, c.hphys * c.wphys), "in2": (c.lda2, c.h2 * c.w2), "out": (c.ldc, c.npix)}[which]
    if c.layout == PIX:
        return c.M * ld, 0
    return TILE_ROWS * ld, npix * TILE_ROWS * ld


def row_off(m, ld, tile_stride):
    return (m >> 7) * (tile_stride or TILE_ROWS * ld) + (m & 127) * ld


def is_full(c):
    """The FULL loader: whole tiles in every direction and offsets that fit 32 bits."""
    bm, bn, _ = tile_choice(c)
    fits = row_off(c.M, c.lda, strides(c, "in")[1]) * 4 < 0xffffffff and c.cout * c.ldw * 4 < 0xffffffff and \
        (c.c2 == 0 or row_off(c.M, c.lda2, strides(c, "in2")[1]) * 4 < 0xffffffff)
    return c.M % bm == 0 and c.cout % bn == 0 and c.cin % 32 == 0 and c.c2 % 32 == 0 and fits


def agent_tiles(c):
    return -(-c.M // tile_choice(c)[0])


def launch_grid(c):
    """Virtual tiles of the launch: agent tiles rounded up to whole XCD groups x pixels x column tiles."""
    bm, bn, _ = tile_choice(c)
    return -(-agent_tiles(c) // NUM_XCD) * NUM_XCD * c.npix * -(-c.cout // bn)


def takes_skinny_route(c):
    """The streamed form for <= 8 output columns (a plain row-major 1 x 1 product) would take the case from the MFMA kernel."""
    return c.cout <= 8 and c.k == 1 and c.hin == 1 and c.win == 1 and c.npix == 1


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def to_pixel_major(t, ld=None, poison=POISON):
    """(M, C, H, W) -> [H W][M][ld]"""
    M, C, H, W = t.shape
    buf = torch.full((H * W, M, ld or C), poison, dtype=t.dtype)
    buf[:, :, :C] = t.permute(2, 3, 0, 1).reshape(H * W, M, C)
    return buf


def from_pixel_major(buf, C, H, W):
    """[H W][M][ld] -> (M, C, H, W)"""
    return buf[:, :, :C].reshape(H, W, buf.shape[1], C).permute(2, 3, 0, 1).contiguous()


def to_tile_major(t, ld=None, poison=POISON):
    """(M, C, H, W) -> [ceil(M / 128)][H W][128][ld]"""
    M, C, H, W = t.shape
    T = -(-M // TILE_ROWS)
    rows = torch.full((T * TILE_ROWS, H * W, C), poison, dtype=t.dtype)
    rows[:M] = t.permute(0, 2, 3, 1).reshape(M, H * W, C)
    buf = torch.full((T, H * W, TILE_ROWS, ld or C), poison, dtype=t.dtype)
    buf[..., :C] = rows.reshape(T, TILE_ROWS, H * W, C).permute(0, 2, 1, 3)
    return buf


def from_tile_major(buf, M, C, H, W):
    """[T][H W][128][ld] -> (M, C, H, W)"""
    T, HW = buf.shape[0], buf.shape[1]
    rows = buf[..., :C].permute(0, 2, 1, 3).reshape(T * TILE_ROWS, HW, C)[:M]
    return rows.reshape(M, H, W, C).permute(0, 3, 1, 2).contiguous()


def pack_map(t, layout, ld, poison=POISON):
    return to_pixel_major(t, ld, poison) if layout == PIX else to_tile_major(t, ld, poison)


def unpack_map(buf, layout, M, C, H, W):
    return from_pixel_major(buf, C, H, W) if layout == PIX else from_tile_major(buf, M, C, H, W)


def valid_mask(buf, layout, M, C):
    """True where the buffer holds a value of the map, False on padding rows and columns."""
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    if layout == PIX:
        mask[:, :, :C] = True
    else:
        T = buf.shape[0]
        live = (torch.arange(T * TILE_ROWS) < M).reshape(T, 1, TILE_ROWS, 1)
        mask[..., :C] = live
    return mask


# ---- inputs and the float64 reference -----------------------------------------------------------------------------------------
def _seed(c):
    return 1000003 * c.cin + 10007 * c.cout + 101 * c.hin + 13 * c.win + 7 * c.k + 5 * c.c2 + 3 * c.stride + c.pool + c.mdraw


def make_inputs(c):
    """randn activations, randn / sqrt(K) weights per segment, randn bias - drawn for c.mdraw agents, the first c.M kept."""
    g = torch.Generator().manual_seed(_seed(c))
    t = types.SimpleNamespace()
    t.x = torch.randn(c.mdraw, c.cin, c.hphys, c.wphys, generator=g)[:c.M]
    t.w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / (c.k * c.k * c.cin) ** 0.5
    t.b = torch.randn(c.cout, generator=g)
    t.x2 = t.w2 = None
    if c.c2:
        t.x2 = torch.randn(c.mdraw, c.c2, c.h2, c.w2, generator=g)[:c.M]
        t.w2 = torch.randn(c.cout, c.c2, 1, 1, generator=g) / c.c2 ** 0.5
    return t


def weight_rows(c, t):
    """[Cout][ldw]: the taps in (ty, tx, channel) order, the residual segment behind them, NaN in the padding."""
    rows = torch.full((c.cout, c.ldw), float("nan"))
    rows[:, :c.k * c.k * c.cin] = t.w.permute(0, 2, 3, 1).reshape(c.cout, -1)
    if c.c2:
        rows[:, c.k * c.k * c.cin:c.ktot] = t.w2.reshape(c.cout, c.c2)
    return rows


def reference(c, t):
    """float64, (M, Cout, Hout, Wout)"""
    x = t.x.double()
    if c.pool == 1:
        x = tnf.avg_pool2d(x, 2) * 4.0          # the kernel SUMS the window: AvgPool2d's 1/4 lives in the weights
    elif c.pool == 2:
        x = tnf.max_pool2d(x, 2)
    y = tnf.conv2d(x, t.w.double(), t.b.double(), c.stride, c.pad)
    if c.c2:
        y = y + tnf.conv2d(t.x2.double(), t.w2.double(), None, c.stride2)
    return y.clamp_min(0) if c.relu else y


# ---- the encoder passes -------------------------------------------------------------------------------------------------------
# absmax slots of magat_encoder_calibrate_f32
SLOT_STEM, SLOT_FEAT, SLOT_COMP, SLOTS_USED, SLOTS = 0, 7, 8, 9, 16
def slot_conv1(l): return 1 + 2 * l
def slot_block(l): return 2 + 2 * l


LARGE_MLP, SLIM_MLP, LARGE = "ResNetLarge_withMLP", "ResNetSlim_withMLP", "ResNetLarge"
CALIBRATE = [(LARGE_MLP, 1), (LARGE_MLP, 128), (LARGE_MLP, 129), (LARGE_MLP, 257), (SLIM_MLP, 129), (LARGE, 129)]
RERUN = [(LARGE_MLP, 129), (LARGE_MLP, 257)]
RERUN_WALK = 4100          # x 128 / 4 columns / 256 threads = 513 blocks: the predicated cast's 512 workgroups walk them
LAST_AGENT_FACTOR = 3.0    # the last agent's state is this much larger: row M - 1 then holds every layer's maximum
MODEL_SEED = {LARGE_MLP: 23, SLIM_MLP: 23, LARGE: 23}
HW = 11


@functools.lru_cache(maxsize=None)
def encoder_model(cnn, scaled=False):
    """(cfg, state dict).  scaled: layer2.0.bn1's gamma and beta x 1e5 (tests/test_gpu_range.py _scaled_model): every map behind
    it leaves the f16 planes' range and the guard re-runs the encoder in float32."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd.synthetic import make_config
    cfg = make_config(CNN_mode=cnn)
    sd = orc.init_state_dict(cfg, seed=MODEL_SEED[cnn])
    if scaled:
        for k in ("weight", "bias"):
            sd["ConvLayers.0.layer2.0.bn1." + k] = sd["ConvLayers.0.layer2.0.bn1." + k] * 1.0e5
    return cfg, sd


@functools.lru_cache(maxsize=None)
def encoder_states(M):
    g = torch.Generator().manual_seed(3 + M)
    x = (torch.rand(M, 3, HW, HW, generator=g) < 0.3).float() + 0.25 * torch.rand(M, 3, HW, HW, generator=g)
    x[M - 1] *= LAST_AGENT_FACTOR
    return x


@functools.lru_cache(maxsize=None)
def encoder_reference(cnn, M, scaled=False):
    """float64: feat (M, n_feat), comp (M, n_comp) or None, and per absmax slot the largest |value| of every agent (M,) - None for
    a slot the variant does not have."""
    from oracle import magat_oracle as orc
    cfg, sd = encoder_model(cnn, scaled)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = encoder_states(M).double()
    pre = "ConvLayers.0"
    per_agent = [None] * SLOTS_USED
    y = torch.relu(orc._bn(tnf.conv2d(x, sd[pre + ".conv1.weight"], None, 1, 1), sd, pre + ".bn1"))
    per_agent[SLOT_STEM] = y.abs().amax(dim=(1, 2, 3))
    nblocks = 3 if (pre + ".layer3.0.conv1.weight") in sd else 2
    for l in range(nblocks):
        bp, stride = "%s.layer%d.0" % (pre, l + 1), (2, 1, 1)[l]
        mid = torch.relu(orc._bn(tnf.conv2d(y, sd[bp + ".conv1.weight"], None, stride, 1), sd, bp + ".bn1"))
        per_agent[slot_conv1(l)] = mid.abs().amax(dim=(1, 2, 3))
        y = orc._basic_block(y, sd, bp, stride)
        per_agent[slot_block(l)] = y.abs().amax(dim=(1, 2, 3))
    feat = orc.conv_layers_forward(x, sd, cnn)
    per_agent[SLOT_FEAT] = feat.abs().amax(dim=1)
    comp = None
    if cnn.endswith("_withMLP"):
        comp = torch.relu(tnf.linear(feat, sd["compressMLP.0.weight"], sd["compressMLP.0.bias"]))
        per_agent[SLOT_COMP] = comp.abs().amax(dim=1)
    return types.SimpleNamespace(feat=feat, comp=comp, per_agent=per_agent,
                                 maxima=[None if p is None else float(p.max()) for p in per_agent])


def rerun_walk_rows(M=RERUN_WALK, distinct=257):
    """Agent i of the M-agent batch is agent i % distinct of the 257-agent one: one float64 reference serves every row."""
    return torch.arange(M) % distinct


def distance_to_power_of_two(v):
    """|v / 2^n - 1| for the nearest power of two: a maximum this close to one could round to the other side of it in float32."""
    e = math.log2(v)
    return min(abs(v / 2.0 ** math.floor(e) - 1.0), abs(v / 2.0 ** math.ceil(e) - 1.0))


# ---- magat_cast_rows ----------------------------------------------------------------------------------------------------------
NAN_BITS = (0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7fff8000, 0xffffffff)
SPECIAL_BITS = (0x00000000, 0x80000000,                              # +-0
                0x00000001, 0x807fffff, 0x00008000, 0x00018000,      # subnormals, two of them ties
                0x3f808000, 0x3f818000,                              # ties: to even down (0x3f80) and up (0x3f82)
                0x3f807fff, 0x3f808001,                              # one bit either side of a tie
                0x7f7fffff, 0xff7fffff,                              # +-FLT_MAX: rounds to +-inf
                0x7f800000, 0xff800000) + NAN_BITS                   # +-inf; quiet / signalling NaNs of both signs
CAST = [(5, 24, 28, 32), (70000, 128, 132, 136)]      # (M, width, ld_src, ld_dst): 70000 x 32 quads = 8750 blocks > the 8192 launched
BF16_POISON = 0x7b7b


def bits_to_f32(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def cast_source(M, width, seed=5):
    """(M, width) float32: randn over a wide range of magnitudes, the specials in the first and the last row."""
    g = torch.Generator().manual_seed(seed + M)
    x = torch.randn(M, width, generator=g) * torch.exp2(torch.randint(-20, 20, (M, 1), generator=g).float())
    sp = bits_to_f32(SPECIAL_BITS)
    assert sp.numel() <= width
    x[0, :sp.numel()] = sp
    x[M - 1, width - sp.numel():] = sp
    return x
