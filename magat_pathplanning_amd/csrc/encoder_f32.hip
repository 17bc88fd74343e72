// Per-agent CNN encoder + compressMLP on gfx950 (reference decentralplanner_GAT_bottleneck.py:90-166,
// 291-302; graphs/models/resnet_pytorch.py:40-73, 334-524), inference form: BatchNorm folded into the
// conv weights host-side (fp64 fold, fp32 store), residual 1x1 branch appended as an extra K segment,
// avgpool+fc(+Flatten+Linear) folded into one "valid" conv.  All GEMM-shaped layers run on the fp32
// MFMA kernel of conv_gemm_f32.hip; only the 3-channel first conv is a direct VALU kernel.
#include <cstdlib>

#include "magat_common.h"
#include "encoder_pack.h"
#include "encoder_route.h"

namespace enc = magat_enc;

namespace {

// conv3x3(3->32, pad 1)+BN+ReLU on (M,3,H,W) NCHW -> pixel-major [H*W][M][32], as an MFMA GEMM with the
// 27-wide im2col row padded to K=32.  A workgroup stages 32 agents' zero-padded images in LDS
// ((H+2)x(W+2) per channel, odd agent stride -> conflict-free column reads); each wave then walks
// output pixels: its 32x32 tile is (32 agents) x (32 channels) at one pixel, i.e. 4 KB of contiguous
// output, from 16 v_mfma_f32_32x32x2_f32 whose A operands are plain ds_read_b32 gathers.
// HC/WC: compile-time map size (0 = runtime H, W).  With constants every index split is a multiply-shift and the
// staging loop unrolls into 12 back-to-back 16-byte loads per thread (the 32 agents' inputs are one contiguous
// 46 KB run), instead of 46 dependent load->divide->store rounds.
template <int HC, int WC>
__global__ __launch_bounds__(256) void conv_first_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                         int M, int Hr, int Wr, long long out_pix_stride,
                                                         long long out_tile_stride, long long out_plane, int out_gl,
                                                         int* range_flag, const int* run_if, int BH, float* absmax) {
  extern __shared__ float img[];
  if (run_if && *run_if == 0) return;        // range-guard re-run: nothing to do unless the split path clamped
  const int H = HC ? HC : Hr, W = WC ? WC : Wr;
  // Row bands (maps whose 32 padded images do not fit the LDS, e.g. 19 x 19 at FOV 17): blockIdx.y owns output rows
  // [ybase, ybase + bh) and stages input rows ybase - 1 .. ybase + bh only.  BH = H (one band) for the usual sizes.
  const int BHe = HC ? HC : BH;
  const int ybase = HC ? 0 : (int)blockIdx.y * BHe;
  const int bh = min(BHe, H - ybase);
  const int PW = W + 2, PHW = (BHe + 2) * PW;
  const int PS = (3 * PHW) | 1;            // odd per-agent stride
  const int HW = H * W;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float amax = 0.f;          // calibration launches: largest stem output of this wave
  // (grid-stride over the 32-agent blocks: one block per workgroup in ordinary launches; the range guard's predicated re-run
  //  is launched with a capped grid - a launch that returns at once still pays for every workgroup it dispatches, and these
  //  carry 65 KB of LDS each: 1600 .. 4000 of them were 10 .. 26 us per forward)
  for (int blk = blockIdx.x; blk * 32 < M; blk += gridDim.x) {
  if (blk != (int)blockIdx.x) __syncthreads();
  const int m0 = blk * 32;
  for (int i = t; i < 32 * PS; i += 256) img[i] = 0.f;
  __syncthreads();
  const int per = 3 * HW;
  if constexpr (HC != 0 && (32 * 3 * HC * WC) % 4 == 0) {
    constexpr int NV = 32 * 3 * HC * WC / 4;          // float4s in the block's contiguous input run
    constexpr int IT = (NV + 255) / 256;
    const long long navail = ((long long)(M - m0) * per) / 4;   // run may be cut short by the batch end
    const f32x4* src = reinterpret_cast<const f32x4*>(x + (long long)m0 * per);
    f32x4 v[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int i4 = t + 256 * k;
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i4 < NV && i4 < navail) v[k] = src[i4];
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int i4 = t + 256 * k;
      if (i4 < NV && i4 < navail) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int f = 4 * i4 + e;
          const int a = f / per, r = f - a * per;
          const int c = r / HW, q = r - c * HW;
          const int y = q / W, xx = q - y * W;
          img[a * PS + c * PHW + (y + 1) * PW + xx + 1] = v[k][e];
        }
      }
    }
    // a batch end that is not float4-aligned leaves < 4 trailing floats: scalar tail
    const long long done = navail * 4, want = (long long)(M - m0 < 32 ? M - m0 : 32) * per;
    for (long long f = done + t; f < want; f += 256) {
      const int a = (int)(f / per), r = (int)(f - (long long)a * per);
      const int c = r / HW, q = r - c * HW;
      const int y = q / W, xx = q - y * W;
      img[a * PS + c * PHW + (y + 1) * PW + xx + 1] = x[(long long)m0 * per + f];
    }
  } else {
    const int brows = bh + 2, bper = 3 * brows * W;      // staged rows per channel: global rows ybase - 1 + ry
    for (int i = t; i < 32 * bper; i += 256) {
      const int a = i / bper, r = i - a * bper;
      const int c = r / (brows * W), q = r - c * brows * W;
      const int ry = q / W, xx = q - ry * W;
      const int y = ybase - 1 + ry;
      if (m0 + a < M && y >= 0 && y < H)
        img[a * PS + c * PHW + ry * PW + xx + 1] = x[(long long)(m0 + a) * per + c * HW + y * W + xx];
    }
  }
  // B operand (weights) and per-k LDS tap offsets for this lane half: k = s + 16*(lane>>5)
  float bw[16];
  int koff[16];
  const int co = lane & 31;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int k = s + 16 * (lane >> 5);
    const bool kok = k < 27;
    bw[s] = kok ? wt[co * 27 + k] : 0.f;
    const int kk = kok ? k : 0;
    koff[s] = (kk / 9) * PHW + ((kk % 9) / 3) * PW + (kk % 3);
  }
  f32x4 bch[4];     // bias of the channels this lane stores: 8q + 4*(lane>>5) + 0..3
#pragma unroll
  for (int q = 0; q < 4; ++q) bch[q] = *reinterpret_cast<const f32x4*>(bias + 8 * q + 4 * (lane >> 5));
  __syncthreads();
  const int abase = (lane & 31) * PS;
  for (int lpix = wave; lpix < bh * W; lpix += 4) {
    const int oy = lpix / W, ox = lpix - oy * W;
    const int base = abase + oy * PW + ox;
    const int pix = (ybase + oy) * W + ox;      // the output pixel in the whole map
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      float a = img[base + koff[s]];
      if (s + 16 * (lane >> 5) >= 27) a = 0.f;
      // operands swapped (weights as the row operand): D[channel][agent], so a lane ends up with four runs of
      // 4 consecutive channels of ONE agent -> 16-byte stores instead of 4-byte ones
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bw[s], a, acc, 0, 0, 0);
    }
    const int agent = m0 + (lane & 31);
    if (agent < M) {
      float* o = out + (long long)pix * out_pix_stride + magat_row_off(agent, 32, out_tile_stride) + 4 * (lane >> 5);
      // granule-major tile ([8 channel quads][128 agents][4], magat_hip.h in_gl/out_gl): quad 2q + (lane>>5) of agent
      // a sits next to its neighbour agents' -> 512-byte runs per half wave and store
      float* og = out + (long long)pix * out_pix_stride + (long long)(agent >> 7) * out_tile_stride +
                  ((lane >> 5) * 128 + (agent & 127)) * 4;
      if (out_gl == 2) {
        // f16 plane granules (magat_hip.h out_gl = 2): quads 2 ks, 2 ks + 1 form the next layer's k-step-ks operand
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        char* ob = reinterpret_cast<char*>(out) + ((long long)pix * out_pix_stride + (long long)(agent >> 7) * out_tile_stride) * 4 +
                   (lane >> 5) * 2048 + (agent & 127) * 16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          unsigned w1[4], w2[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {        // pairs (2e, 2e+1) of the 8 values of quads 2 ks, 2 ks + 1
            const int q = 2 * ks + (e >> 1), c = 2 * (e & 1);
            const float a0 = magat_relu(acc[4 * q + c] + bch[q][c]), b0 = magat_relu(acc[4 * q + c + 1] + bch[q][c + 1]);
            if ((!(a0 <= 65504.f) || !(b0 <= 65504.f)) && range_flag) atomicOr(range_flag, 1);      // range guard (rare)
            const float a = __builtin_amdgcn_fmed3f(a0, -65504.f, 65504.f);
            const float b2 = __builtin_amdgcn_fmed3f(b0, -65504.f, 65504.f);
            const h2 h = __builtin_convertvector(f2{a, b2}, h2);
            const h2 r = __builtin_convertvector(f2{a - (float)h[0], b2 - (float)h[1]}, h2);
            w1[e] = __builtin_bit_cast(unsigned, h);
            w2[e] = __builtin_bit_cast(unsigned, r);
          }
          *reinterpret_cast<u4*>(ob + ks * 4096) = u4{w1[0], w1[1], w1[2], w1[3]};
          *reinterpret_cast<u4*>(ob + 256 * 32 + ks * 4096) = u4{w2[0], w2[1], w2[2], w2[3]};
        }
        continue;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = magat_relu(acc[4 * q + c] + bch[q][c]);
        if (absmax) amax = fmaxf(fmaxf(amax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        if (out_gl) {
          *reinterpret_cast<f32x4*>(og + q * 1024) = v;
        } else if (out_plane == 0) {
          *reinterpret_cast<f32x4*>(o + 8 * q) = v;
        } else {      // two f16 planes (operand format of the f16x3 convs, conv_gemm_bf16x6.hip in_fmt 5)
          typedef _Float16 h2 __attribute__((ext_vector_type(2)));
          typedef float f2 __attribute__((ext_vector_type(2)));
          unsigned short* ob = reinterpret_cast<unsigned short*>(out) + (o - out) + 8 * q;
          unsigned w1[2], w2[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const float a = fminf(v[2 * c], 65504.f), b2 = fminf(v[2 * c + 1], 65504.f);
            const h2 h = __builtin_convertvector(f2{a, b2}, h2);
            const h2 r = __builtin_convertvector(f2{a - (float)h[0], b2 - (float)h[1]}, h2);
            w1[c] = __builtin_bit_cast(unsigned, h);
            w2[c] = __builtin_bit_cast(unsigned, r);
          }
          *reinterpret_cast<uint2*>(ob) = uint2{w1[0], w1[1]};
          *reinterpret_cast<uint2*>(ob + out_plane) = uint2{w2[0], w2[1]};
        }
      }
    }
  }
  }      // (32-agent blocks)
  if (absmax) {
    amax = wave_max(amax);
    if (lane == 0 && amax > 0.f) atomicMax(reinterpret_cast<unsigned*>(absmax), __builtin_bit_cast(unsigned, amax));
  }
}

int enc_chunk_agents(int M) {
  long long c = magat_opt(MAGAT_OPT_ENC_CHUNK);
  if (c < 128) c = 128;
  if (c > M) c = M;
  return (int)c;
}

struct BlockShape {
  int cin, cout, stride;
};


// feat[m][n] = bias[n] + sum over the pooled cells (fixed order) of part[c][m][n]: the second half of the split-K head
__global__ __launch_bounds__(256) void head_sum_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                       float* __restrict__ feat, int ldfeat, int M, int nf, int cells,
                                                       const int* __restrict__ run_if) {
  if (run_if && *run_if == 0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int q = nf / 4;
  if (i >= (long long)M * q) return;
  const int m = (int)(i / q), n = (int)(i % q) * 4;
  f32x4 acc = *reinterpret_cast<const f32x4*>(bias + n);
  const float* src = part + (long long)m * nf + n;
  for (int c = 0; c < cells; ++c) acc += *reinterpret_cast<const f32x4*>(src + (long long)c * M * nf);
  *reinterpret_cast<f32x4*>(feat + (long long)m * ldfeat + n) = acc;
}

// range guard bookkeeping at the end of a forward: status[2] = this forward's flag, status[1] += 1 when the float32 re-run
// happened, and the working flag status[0] is cleared for the next forward (no memset launch per forward)
__global__ void guard_count_kernel(int* status) {
  const int f = status[0];
  status[2] = f;
  if (f != 0) status[1] += 1;
  status[0] = 0;
}

}  // namespace

static int conv_first_launch(const float* x, const float* wt, const float* bias, float* out, int M, int H, int W,
                             long long pix_stride, long long tile_stride, void* stream, long long out_plane = 0,
                             int out_gl = 0, int* range_flag = nullptr, const int* run_if = nullptr, int tag = MAGAT_TAG_CONV_FIRST,
                             float* absmax = nullptr) {
  if (!x || !wt || !bias || !out) return MAGAT_ERR_NULL;
  if (M <= 0 || H <= 0 || W <= 0) return MAGAT_ERR_BAD_SHAPE;
  int BH = H;      // rows per band: the whole map when its 32 padded images fit the LDS
  auto lds_for = [&](int bh) { return sizeof(float) * 32 * (size_t)((3 * (bh + 2) * (W + 2)) | 1); };
  while (BH > 1 && lds_for(BH) > 160 * 1024) BH = (BH + 1) / 2;
  const size_t lds = lds_for(BH);
  if (lds > 160 * 1024) return MAGAT_ERR_UNSUPPORTED;
  const int bands = (H + BH - 1) / BH;
  const bool c11 = H == 11 && W == 11 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (lds > 64 * 1024 &&
      magat_ensure_dyn_lds(c11 ? reinterpret_cast<const void*>(&conv_first_kernel<11, 11>)
                               : reinterpret_cast<const void*>(&conv_first_kernel<0, 0>),
                           c11 ? MAGAT_LDS_CONV_FIRST11 : MAGAT_LDS_CONV_FIRST, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  int blocks = (M + 31) / 32;
  if (run_if && blocks > 256) blocks = 256;      // predicated re-run: a capped grid that walks the blocks (see the kernel)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int pid = magat_prof_begin(tag, st);
  if (c11)
    hipLaunchKernelGGL((conv_first_kernel<11, 11>), dim3(blocks), dim3(256), lds, st, x, wt, bias, out, M, H, W,
                       pix_stride, tile_stride, out_plane, out_gl, range_flag, run_if, H, absmax);
  else
    hipLaunchKernelGGL((conv_first_kernel<0, 0>), dim3(blocks, bands), dim3(256), lds, st, x, wt, bias, out, M, H, W,
                       pix_stride, tile_stride, out_plane, out_gl, range_flag, run_if, BH, absmax);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_encoder_stem_block_f32(const magat_encoder_desc* d, const float* x, void* out, void* ctr, int M, int form,
                                            int32_t* range_flag, void* stream) {
  if (!d || !d->pack || !x || !out || !ctr) return MAGAT_ERR_NULL;
  if (M <= 0 || form < 0 || form > 2) return MAGAT_ERR_BAD_SHAPE;
  if (d->variant != 0 && d->variant != 1) return MAGAT_ERR_UNSUPPORTED;
  if (d->off[enc::PERMUTED] == 0) return MAGAT_ERR_UNSUPPORTED;        // (the pack holds no plane-granule weight copies)
  const float* pk = d->pack;
  const int H = d->H, W = d->W;
  const enc::FusedPtrs fp = enc::resolve(pk, d->off, d->scaled_off, true);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool can8 = H == 11 && W == 11 && d->l1frag_off > 0;
  if (form == 0) form = (can8 && magat_opt(MAGAT_OPT_L1_FUSED) >= 2) ? 2 : 1;
  if (form == 2) {
    if (!can8) return MAGAT_ERR_UNSUPPORTED;
    return magat_stem8(x, fp.w0, fp.b0, pk + d->l1frag_off, fp.b1, out, ctr, M, H, W, st, reinterpret_cast<int*>(range_flag));
  }
  if (magat_layer1_fused_lds(W) == 0) return MAGAT_ERR_UNSUPPORTED;
  // (the K-permuted f16 copy of layer1.conv1 sits behind the plain one)
  return magat_layer1_fused(x, fp.w0, fp.b0, pk + d->off[enc::conv1_f16(0)] + enc::permuted_behind(32, 9 * 32), fp.b1, out, ctr, M,
                            H, W, st, reinterpret_cast<int*>(range_flag));
}

extern "C" int magat_conv_first_f32(const float* x, const float* wt, const float* bias, float* out, int M, int H,
                                    int W, void* stream) {
  return conv_first_launch(x, wt, bias, out, M, H, W, (long long)M * 32, (long long)MAGAT_TILE_ROWS * 32, stream);
}

extern "C" int magat_conv_first_tiled_f32(const float* x, const float* wt, const float* bias, float* out, int M, int H,
                                          int W, void* stream) {
  return conv_first_launch(x, wt, bias, out, M, H, W, (long long)MAGAT_TILE_ROWS * 32,
                           (long long)H * W * MAGAT_TILE_ROWS * 32, stream);
}

// floats per agent of one rotating activation buffer
static size_t enc_buf_floats_per_agent(const magat_encoder_desc* d) {
  if (d->variant >= 2) return (size_t)d->H * d->W * 32;    // plain CNNs: the first map is the largest
  const int Ho = (d->H + 2 - 3) / 2 + 1, Wo = (d->W + 2 - 3) / 2 + 1;
  const size_t a0 = (size_t)d->H * d->W * 32;
  const size_t a3 = (size_t)Ho * Wo * (d->variant == 0 ? 128 : 64);
  return a0 > a3 ? a0 : a3;
}

constexpr size_t ENC_STATUS_BYTES = 256;     // status block at the head of the workspace (magat_hip.h)

// bytes of one of the three rotating activation buffers: whole agent tiles of a chunk
static size_t enc_buf_bytes(const magat_encoder_desc* d, int M) {
  const int mc = (enc_chunk_agents(M) + MAGAT_TILE_ROWS - 1) / MAGAT_TILE_ROWS * MAGAT_TILE_ROWS;
  return magat_align_up(enc_buf_floats_per_agent(d) * (size_t)mc * sizeof(float), 256);
}

extern "C" size_t magat_encoder_workspace_bytes(const magat_encoder_desc* d, int M) {
  if (!d || M <= 0) return 0;
  return ENC_STATUS_BYTES + 3 * enc_buf_bytes(d, M);
}

extern "C" int magat_encoder_read_status(const void* workspace, int32_t status_host[2], void* stream) {
  if (!workspace || !status_host) return MAGAT_ERR_NULL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t w[3];
  if (hipMemcpyAsync(w, workspace, sizeof(w), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MAGAT_ERR_LAUNCH;
  status_host[0] = w[2];      // the last forward's flag
  status_host[1] = w[1];      // re-run count
  return MAGAT_OK;
}

// The workspace of one call: status block, agents per chunk, the three rotating activation buffers.
// Activations are TILE-major: [agent tile][pixel][128][C]
struct EncBuffers { int32_t* status; int mc; float* buf[3]; };
static int64_t enc_pixs(int c) { return (int64_t)MAGAT_TILE_ROWS * c; }
static int64_t enc_tiles(int npix, int c) { return (int64_t)npix * MAGAT_TILE_ROWS * c; }

static EncBuffers enc_buffers(const magat_encoder_desc* d, int M, void* workspace) {
  const size_t bstride = enc_buf_bytes(d, M) / sizeof(float);
  float* base = reinterpret_cast<float*>(static_cast<char*>(workspace) + ENC_STATUS_BYTES);
  return {static_cast<int32_t*>(workspace), enc_chunk_agents(M), {base, base + bstride, base + 2 * bstride}};
}

// y = act(x @ w^T + b) as a 1 x 1 convolution (compressMLP in every form it takes)
static magat_conv_gemm_desc enc_linear_desc(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int M,
                                            int N, int K, int relu, int tag) {
  magat_conv_gemm_desc d = {};
  d.tag = tag;
  d.in = x; d.wt = w; d.bias = b; d.out = y;
  d.M = M; d.Cin = K; d.lda = ldx; d.Hin = d.Win = 1; d.kH = d.kW = 1; d.stride = 1; d.pad = 0;
  d.Hout = d.Wout = 1; d.Cout = N; d.ldc = ldy; d.relu = relu;
  return d;
}

// What a pass of the ResNet encoders carries besides the route's inputs
struct EncPass {
  enc::Pass pass;
  int32_t* range_flag = nullptr;       // forward: where the split kernels report a clamp when the route guards the pass
  const int32_t* run_if = nullptr;     // re-run: its predicate (every launch returns immediately unless *run_if != 0)
  float* absmax = nullptr;             // calibration: the 16 floats of magat_encoder_calibrate_f32
  int32_t* book = nullptr;             // re-run: the status block, for the bookkeeping of the last chained launch
  // out
  enc::Guard guard = enc::GUARD_NONE;  // forward: who guards (GUARD_LAT: block_lat.hip did - nothing to re-run, nothing to book)
  bool bf16_after_guard = false;       // forward: desc.comp_bf16 is rewritten behind the guard
  bool booked = false;                 // re-run: the last chained launch did the bookkeeping
};

// One chunk of agents on its way through the three stages
struct EncChunk {
  const magat_encoder_desc* d; EncPass* pass; void* stream;
  enc::Route r; enc::FusedPtrs fp;
  float* const* buf; int mm;           // the three rotating buffers; agents of this chunk
  const float* x; float* feat; float* comp; int ldfeat, ldcomp;      // this chunk's rows
  unsigned short* comp16;              // ... of desc.comp_bf16 (ABI 7), when the route serves them
  int32_t* flag;                       // the pass's range flag, null when nobody guards
  int cur = 0, hin = 0, win = 0;       // buffer holding the next stage's input, and its map size
  magat_conv_gemm_desc chain[10];      // the guard's re-run: every float32 layer behind the stem goes into ONE predicated launch
  int nchain = 0;                      // (magat_conv_gemm_chain_f32)

  bool rerun() const { return pass->pass == enc::PASS_RERUN; }
  int tagof(int t) const { return rerun() ? MAGAT_TAG_UNTAGGED : t; }     // the re-run is timed as ONE span by the caller
  int run_or_chain(const magat_conv_gemm_desc& g) {
    if (rerun() && nchain < 10) { chain[nchain] = g; chain[nchain].run_if = nullptr; ++nchain; return MAGAT_OK; }
    return magat_conv_gemm_f32(&g, stream);
  }
};

// Stem (+ layer1.conv1 in the fused forms: the 121-pixel stem output never reaches HBM; buf[0] receives only its 36 stride-2
// pixels, the input of the block's residual 1x1 branch, buf[1] layer1.conv1's map)
static int enc_stem(EncChunk& c) {
  const magat_encoder_desc* d = c.d;
  const float* pk = d->pack;
  const int H = d->H, W = d->W;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  switch (c.r.stem) {
    case enc::STEM_LAT:      // (block_lat runs it: buf[0] / buf[1] hold nothing)
      return MAGAT_OK;
    case enc::STEM_8:        // block_fused.hip stem8_kernel: every stem pixel once, no im2col instructions
      return magat_stem8(c.x, c.fp.w0, c.fp.b0, pk + d->l1frag_off, c.fp.b1, c.buf[1], c.buf[0], c.mm, H, W, st, c.flag);
    case enc::STEM_BAND:
      return magat_layer1_fused(c.x, c.fp.w0, c.fp.b0, pk + d->off[enc::conv1_f16(0)] + enc::permuted_behind(32, 9 * 32), c.fp.b1,
                                c.buf[1], c.buf[0], c.mm, H, W, st, c.flag);
    default:
      return conv_first_launch(c.x, c.fp.w0, c.fp.b0, c.buf[0], c.mm, H, W, (long long)MAGAT_TILE_ROWS * 32,
                               (long long)H * W * MAGAT_TILE_ROWS * 32, c.stream, 0, c.r.lay, c.flag, c.pass->run_if,
                               c.tagof(MAGAT_TAG_CONV_FIRST), c.pass->absmax);
  }
}

// BasicBlock chain: the chain kernels, then whatever blocks the route leaves to the layer-by-layer loop
static int enc_chain(EncChunk& c) {
  const magat_encoder_desc* d = c.d;
  const enc::Route& r = c.r;
  const enc::FusedPtrs& fp = c.fp;
  const float* pk = d->pack;
  float* const* buf = c.buf;
  const int H = d->H, W = d->W;
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const BlockShape shapes[3] = {{32, 32, 2}, {32, 64, 1}, {64, 128, 1}};
  const int nblocks = d->variant == 0 ? 3 : 2;
  int32_t* range_flag = c.flag;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  int rc;
  c.cur = 0; c.hin = H; c.win = W;
  if (r.chain != enc::CHAIN_LAYERS) { c.cur = 2; c.hin = Ho; c.win = Wo; }      // (every chain kernel leaves Ho x Wo maps in buf[2])
  if (r.chain == enc::CHAIN_LAT) {      // block_lat.hip: the chain and, where the route says so, the head + compressMLP, ...
    magat_lat_head lh = {};
    const bool head_in = r.head == enc::HEAD_LAT;
    if (head_in) {
      lh.hfrag = pk + d->headfrag_off; lh.cfrag = pk + d->compfrag_off;
      lh.hbias = pk + d->off[enc::HEAD_B]; lh.cbias = pk + d->off[enc::COMP_B];
      lh.insc = fp.head_in; lh.insc2 = fp.comp_in;
      lh.feat = c.feat; lh.ldfeat = c.ldfeat;
      lh.comp = c.comp; lh.ldcomp = c.ldcomp; lh.ncomp = d->n_comp;
    }
    magat_lat_stem ls = {};      // ... the stem + layer1.conv1 in front (enc_stem launched nothing then)
    const bool stem_in = r.stem == enc::STEM_LAT;
    if (stem_in) {
      ls.x = c.x; ls.w0 = fp.w0; ls.b0 = fp.b0;
      ls.w1f = pk + d->l1frag_off; ls.b1 = fp.b1;
    }
    magat_lat_guard lg = {};     // ... and the encoder's range guard
    const bool inguard = r.guard == enc::GUARD_LAT;
    if (inguard) {
      lg.x = c.x; lg.pack = pk; lg.off = d->off; lg.book = reinterpret_cast<int*>(range_flag);
    }
    rc = magat_block_lat(buf[1], buf[0], pk + d->chain_off, fp.bA, fp.bB, fp.bC, buf[2], pk + d->chain3_off, fp.b31, fp.b32, c.mm,
                         reinterpret_cast<int*>(range_flag), st, fp.scales, r.head_gl ? 1 : 0, head_in ? &lh : nullptr,
                         inguard ? &lg : nullptr, stem_in ? &ls : nullptr);
    if (rc != MAGAT_OK) return rc;
  } else if (r.chain == enc::CHAIN_ONE) {
    rc = magat_block_full(buf[1], buf[0], pk + d->chain_off, fp.bA, fp.bB, fp.bC, buf[2], pk + d->chain3_off, fp.b31, fp.b32, c.mm,
                          reinterpret_cast<int*>(range_flag), st, fp.scales, r.head_gl ? 1 : 0,
                          d->off[enc::TILE16] > 0 ? pk + d->off[enc::TILE16] : nullptr, r.Mform);
    if (rc != MAGAT_OK) return rc;
  } else if (r.chain == enc::CHAIN_TWO) {
    rc = magat_block_chain(buf[1], buf[0], buf[2], nblocks == 2 ? 0 : 2, enc_pixs(64), enc_tiles(Ho * Wo, 64), pk + d->chain_off,
                           fp.bA, fp.bB, fp.bC, c.mm, reinterpret_cast<int*>(range_flag), st);
    if (rc != MAGAT_OK) return rc;
    // ... and layer3 + ReLU + AvgPool2d(2) as one more launch: the head then reads 9 pooled cells instead of 36 pixels
    if (r.first_loop_block == 3) {
      rc = magat_block3(buf[2], buf[0], pk + d->chain3_off, fp.b31, fp.b32, c.mm, reinterpret_cast<int*>(range_flag), st);
      if (rc != MAGAT_OK) return rc;
      c.cur = 0;
    }
  }
  const bool fused1 = r.stem != enc::STEM_PLAIN;      // layer1.conv1 ran with the stem
  const int lay = r.lay;
  auto permuted = [&](int cout, int ktot) { return lay == 2 ? enc::permuted_behind(cout, ktot) : (int64_t)0; };
  for (int l = r.first_loop_block; l < nblocks; ++l) {
    const BlockShape s = shapes[l];
    const int hin = c.hin, win = c.win, cur = c.cur;
    const int hout = s.stride == 2 ? Ho : hin, wout = s.stride == 2 ? Wo : win;
    const int mid = (cur + 1) % 3, nxt = (cur + 2) % 3;
    magat_conv_gemm_desc g = {};
    // conv1 + bn1 + relu
    g.in = buf[cur]; g.wt = pk + d->off[enc::conv1_w(l)]; g.bias = pk + d->off[enc::conv1_b(l)]; g.out = buf[mid];
    g.in_pix_stride = enc_pixs(s.cin); g.out_pix_stride = enc_pixs(s.cout);
    g.in_tile_stride = enc_tiles(hin * win, s.cin); g.out_tile_stride = enc_tiles(hout * wout, s.cout);
    g.M = c.mm; g.Cin = s.cin; g.lda = s.cin; g.Hin = hin; g.Win = win; g.kH = g.kW = 3; g.stride = s.stride;
    g.pad = 1; g.Hout = hout; g.Wout = wout; g.Cout = s.cout; g.ldc = s.cout; g.relu = 1;
    g.tag = c.tagof(MAGAT_TAG_BLOCK_CONV + 2 * l);
    g.range_flag = range_flag; g.run_if = c.pass->run_if;
    if (c.pass->absmax) g.absmax = c.pass->absmax + 1 + 2 * l;
    if (r.split >> l & 1) {      // split-MFMA kernel: float32 activations split by its loader, pre-split weights
      g.in_fmt = 4; g.wt = pk + d->off[enc::conv1_f16(l)];
    }
    g.in_gl = g.out_gl = lay;
    if (lay == 2) g.wt += permuted(s.cout, 9 * s.cin);
    if (!(fused1 && l == 0)) {
      rc = c.run_or_chain(g);
      if (rc != MAGAT_OK) return rc;
    }
    // conv2 + bn2 + (1x1 strided downsample + bn) + relu
    magat_conv_gemm_desc h = {};
    h.in = buf[mid]; h.in2 = buf[cur]; h.wt = pk + d->off[enc::conv2_w(l)]; h.bias = pk + d->off[enc::conv2_b(l)];
    h.out = buf[nxt];
    h.in_pix_stride = enc_pixs(s.cout); h.in2_pix_stride = enc_pixs(s.cin); h.out_pix_stride = enc_pixs(s.cout);
    h.in_tile_stride = enc_tiles(hout * wout, s.cout); h.in2_tile_stride = enc_tiles(hin * win, s.cin);
    h.out_tile_stride = enc_tiles(hout * wout, s.cout);
    h.M = c.mm; h.Cin = s.cout; h.lda = s.cout; h.Hin = hout; h.Win = wout; h.kH = h.kW = 3; h.stride = 1; h.pad = 1;
    h.Hout = hout; h.Wout = wout; h.C2 = s.cin; h.lda2 = s.cin; h.W2 = win; h.stride2 = s.stride;
    h.Cout = s.cout; h.ldc = s.cout; h.relu = 1;
    h.tag = c.tagof(MAGAT_TAG_BLOCK_CONV + 2 * l + 1);
    h.range_flag = range_flag; h.run_if = c.pass->run_if;
    if (c.pass->absmax) h.absmax = c.pass->absmax + 2 + 2 * l;
    if (r.split >> l & 1) {
      h.in_fmt = 4; h.wt = pk + d->off[enc::conv2_f16(l)];
    }
    h.in_gl = lay; h.out_gl = l + 1 < nblocks ? lay : 0;
    if (lay == 2) h.wt += permuted(s.cout, 9 * s.cout + s.cin);
    if (fused1 && l == 0) {    // the residual branch reads the stem's stride-2 pixels, stored as an Ho x Wo map
      h.in2_tile_stride = enc_tiles(hout * wout, s.cin); h.W2 = wout; h.stride2 = 1;
    }
    rc = c.run_or_chain(h);
    if (rc != MAGAT_OK) return rc;
    c.cur = nxt; c.hin = hout; c.win = wout;
  }
  return MAGAT_OK;
}

// Head, compressMLP and the bf16 rows
static int enc_head(EncChunk& c) {
  const magat_encoder_desc* d = c.d;
  const enc::Route& r = c.r;
  const enc::FusedPtrs& fp = c.fp;
  const float* pk = d->pack;
  float* const* buf = c.buf;
  const int hin = c.hin, win = c.win, cur = c.cur, mm = c.mm;
  const int clast = d->variant == 0 ? 128 : 64;
  int32_t* range_flag = c.flag;
  const int32_t* run_if = c.pass->run_if;
  float* absmax = c.pass->absmax;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  int rc = MAGAT_OK;
  bool compress_done = r.head == enc::HEAD_LAT;      // head + compressMLP ran in the chain kernel's epilogue (latency form)
  bool comp16_done = false;                          // compressMLP rode in the head's epilogue and wrote the bf16 rows too
  if (r.head != enc::HEAD_LAT) {
    // head: AvgPool2d(2) (sum-pool on load, 1/4 in the weights) + fc(+Flatten+Linear) folded into one
    // (hin/2 x win/2) valid conv over the pooled map -> [mm][n_feat]
    magat_conv_gemm_desc g = {};
    g.in = buf[cur]; g.wt = pk + d->off[enc::HEAD_W]; g.bias = pk + d->off[enc::HEAD_B];
    g.out = c.feat; g.relu = 0;
    g.in_pix_stride = enc_pixs(clast); g.in_tile_stride = enc_tiles(r.pooled ? (hin / 2) * (win / 2) : hin * win, clast);
    g.M = mm; g.Cin = clast; g.lda = clast; g.Hin = hin / 2; g.Win = win / 2;
    g.kH = hin / 2; g.kW = win / 2; g.stride = 1; g.pad = 0; g.Hout = g.Wout = 1; g.Cout = d->n_feat; g.ldc = c.ldfeat;
    if (!r.pooled) { g.pool = 1; g.pool_w = win; }
    g.tag = c.tagof(MAGAT_TAG_HEAD);
    g.run_if = run_if;
    if (absmax) g.absmax = absmax + 7;
    if (r.head == enc::HEAD_SPLITK) {
      // Few agents (the closed-loop batch-1 step): one workgroup per 64 agents would walk all (hin/2)(win/2) clast of K alone
      // (83 us at 100 agents).  Split K by pooled cell instead: every cell is its own 1x1 "output pixel" with its slice of the
      // weight rows (wt_pix_stride / ldw), the partial products land in a free map buffer, a small kernel sums them in
      // a fixed order and adds the bias.
      const int cells = (hin / 2) * (win / 2);
      float* part = buf[(cur + 1) % 3];                 // [cells][mm][n_feat]
      if (!c.rerun()) magat_form_note(MAGAT_FORM_HEAD_SPLITK);
      g.out = part; g.bias = nullptr; g.ldc = d->n_feat;
      g.out_pix_stride = (long long)mm * d->n_feat;
      g.kH = g.kW = 1; g.Hout = hin / 2; g.Wout = win / 2;
      g.wt_pix_stride = clast; g.ldw = cells * clast;
      const int pid = magat_prof_begin(c.tagof(MAGAT_TAG_HEAD), st);
      g.tag = MAGAT_TAG_UNTAGGED;
      rc = magat_conv_gemm_f32(&g, c.stream);
      if (rc == MAGAT_OK) {
        const long long total4 = (long long)mm * (d->n_feat / 4);
        hipLaunchKernelGGL(head_sum_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, part,
                           pk + d->off[enc::HEAD_B], c.feat, c.ldfeat, mm, d->n_feat, cells, reinterpret_cast<const int*>(run_if));
        if (hipGetLastError() != hipSuccess) rc = MAGAT_ERR_LAUNCH;
      }
      magat_prof_end(pid, st);
    } else if (r.head == enc::HEAD_LONGK) {
      // many agents, pooled input (no pooling on load): a plain valid convolution - f16x3 split products like the blocks
      g.in_fmt = 4; g.wt = pk + d->head16_off; g.range_flag = range_flag; g.run_if = nullptr;
      g.in_scale = fp.head_in;
      if (r.head_gl) g.in_gl = 1;
      magat_form_note(MAGAT_FORM_HEAD_LONGK);
      // compressMLP in the head's epilogue: declined (MAGAT_ERR_UNSUPPORTED, nothing launched) when the head's column tile was
      // narrowed for a small batch - the two launches follow as before
      if (r.comp_epilogue) {
        magat_conv_gemm_desc f = g;
        f.wt2 = pk + d->comp16_off; f.bias2 = pk + d->off[enc::COMP_B]; f.out2 = c.comp;
        f.Cout2 = d->n_comp; f.ldc2 = c.ldcomp; f.relu2 = 1;
        f.in_scale2 = fp.comp_in;
        // (ABI 7: the bf16 rows of the bf16-storage graph layer from the same epilogue)
        if (r.bf16 == enc::BF16_EPILOGUE) { f.out2_bf16 = c.comp16; f.ldc2_bf16 = d->n_comp; }
        rc = magat_conv_gemm_f32(&f, c.stream);
        if (rc == MAGAT_OK) { compress_done = true; comp16_done = r.bf16 == enc::BF16_EPILOGUE; }
        else if (rc != MAGAT_ERR_UNSUPPORTED) return rc;
      }
      if (!compress_done) rc = magat_conv_gemm_f32(&g, c.stream);
    } else {
      rc = c.run_or_chain(g);
    }
    if (rc != MAGAT_OK) return rc;
  }
  if (!compress_done && r.comp != enc::COMP_NONE) {
    // compressMLP: f16x3 split products on the direct kernel when the head ran that way (large pooled batches), else
    // float32 MFMA (and always in the guard's re-run)
    magat_conv_gemm_desc m = enc_linear_desc(c.feat, c.ldfeat, pk + d->off[enc::COMP_W], pk + d->off[enc::COMP_B], c.comp,
                                             c.ldcomp, mm, d->n_comp, d->n_feat, 1, c.tagof(MAGAT_TAG_COMPRESS));
    if (r.comp == enc::COMP_F16) {
      m.wt = pk + d->comp16_off; m.in_fmt = 4; m.range_flag = range_flag;
      m.in_scale = fp.comp_in;
      rc = magat_conv_gemm_f32(&m, c.stream);
    } else {      // COMP_F32 / COMP_CHAINED: a launch of its own, or one more layer of the re-run's chained launch
      m.run_if = run_if; m.absmax = absmax ? absmax + 8 : nullptr;
      rc = c.run_or_chain(m);
    }
    if (rc != MAGAT_OK) return rc;
  }
  if (r.bf16 != enc::BF16_NONE && !comp16_done) {
    // comp came from a launch of its own (small batches, float32 forms): one cast pass over this chunk's rows
    rc = magat_cast_rows(c.comp, c.comp16, 1, mm, d->n_comp, c.ldcomp, d->n_comp, c.stream);
    if (rc != MAGAT_OK) return rc;
  }
  return MAGAT_OK;
}

static enc::RouteIn enc_route_input(const magat_encoder_desc* d, const float* comp, int M, enc::Pass pass) {
  enc::RouteIn in = {};
  in.variant = d->variant; in.H = d->H; in.W = d->W; in.n_feat = d->n_feat; in.n_comp = d->n_comp; in.form_agents = d->form_agents;
  for (int l = 0; l < 3; ++l) in.f16[l] = d->off[enc::conv1_f16(l)] > 0 && d->off[enc::conv2_f16(l)] > 0;
  in.permuted = d->off[enc::PERMUTED] != 0;
  in.chain = d->chain_off > 0; in.chain3 = d->chain3_off > 0; in.head16 = d->head16_off > 0; in.comp16 = d->comp16_off > 0;
  in.scaled = d->scaled_off > 0; in.l1frag = d->l1frag_off > 0; in.headfrag = d->headfrag_off > 0; in.compfrag = d->compfrag_off > 0;
  in.comp = comp != nullptr; in.comp_bf16 = d->comp_bf16 != nullptr;
  in.M = in.mm = M; in.pass = pass; in.buf_floats = enc_buf_floats_per_agent(d);
  in.opt = {magat_opt(MAGAT_OPT_CONV_SPLIT), magat_opt(MAGAT_OPT_RANGE_GUARD), magat_opt(MAGAT_OPT_CONV_PCHAIN),
            magat_opt(MAGAT_OPT_L1_FUSED), magat_opt(MAGAT_OPT_BLOCK_FUSED), magat_opt(MAGAT_OPT_HEAD_SPLITK),
            magat_opt(MAGAT_OPT_HEAD_F16), magat_opt(MAGAT_OPT_HEAD_COMPRESS), magat_opt(MAGAT_OPT_LAT_AGENTS)};
  in.conv_direct = magat_conv_direct_enabled() != 0; in.full_out_gl = magat_block_full_out_gl() != 0;
  in.l1_lds = magat_layer1_fused_lds(d->W) != 0;
  return in;
}

// One pass of the ResNet encoders (variant 0 / 1) over all agents, chunk by chunk: route, stem, chain, head.
static int enc_run_resnet(const magat_encoder_desc* d, const float* x, float* feat, int ldfeat, float* comp, int ldcomp,
                          const EncBuffers& b, int M, void* stream, EncPass& pass) {
  enc::RouteIn in = enc_route_input(d, comp, M, pass.pass);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int m0 = 0; m0 < M; m0 += b.mc) {
    EncChunk c;
    c.d = d; c.pass = &pass; c.buf = b.buf; c.stream = stream;
    c.mm = in.mm = (M - m0) < b.mc ? (M - m0) : b.mc;
    c.r = enc::route(in);
    c.fp = enc::resolve(d->pack, d->off, d->scaled_off, c.r.scaled_chain);
    c.flag = c.r.guard != enc::GUARD_NONE ? pass.range_flag : nullptr;
    // (every chunk gives the same answers here: only a call of ONE chunk can be guarded inside the latency kernel)
    pass.guard = c.r.guard; pass.bf16_after_guard = c.r.bf16_after_guard;
    c.x = x + (size_t)m0 * 3 * d->H * d->W;
    c.feat = feat + (size_t)m0 * ldfeat; c.ldfeat = ldfeat;
    c.comp = comp ? comp + (size_t)m0 * ldcomp : nullptr; c.ldcomp = ldcomp;
    c.comp16 = c.r.bf16 != enc::BF16_NONE ? static_cast<unsigned short*>(d->comp_bf16) + (size_t)m0 * d->n_comp : nullptr;
    int rc = enc_stem(c);
    if (rc == MAGAT_OK) rc = enc_chain(c);
    if (rc == MAGAT_OK) rc = enc_head(c);
    if (rc != MAGAT_OK) return rc;
    if (c.nchain > 0) {
      // (the last chunk's chained launch is the last reader of the guard's flag: its last workgroup does the bookkeeping)
      const bool last = pass.book && m0 + b.mc >= M;
      rc = magat_conv_gemm_chain_f32(c.chain, c.nchain, pass.run_if, MAGAT_TAG_UNTAGGED, st, last ? pass.book : nullptr);
      if (rc != MAGAT_OK) return rc;
      if (last) pass.booked = true;
    }
  }
  return MAGAT_OK;
}

// Plain CNNs (float32 kernels only): conv-BN-ReLU stacks with MaxPool2d(2) behind some layers, the pool folded into the NEXT
// layer's loader (or, behind the last layer, into a pooled 1x1 GEMM with identity weights).
//   2: CNN_mode Default - 5 layers, pools behind layers 0, 2, 4;
//   3 / 4 (ABI 8): the dilated CNNs of DecentralPlannerNet (use_dilated_version 1 / 2; decentralplanner.py:57-86, 138-162):
//          5 (4) layers with dilation = padding = 1 3 1 3 (1), pools behind layers 1 and 3
static int enc_run_plain_cnn(const magat_encoder_desc* d, const float* x, float* feat, int ldfeat, float* comp, int ldcomp,
                             const EncBuffers& b, int M, void* stream) {
  const int H = d->H, W = d->W;
  const float* pk = d->pack;
  float* const* buf = b.buf;
  const int nl = d->variant == 4 ? 4 : 5;
  const int chans[6] = {3, 32, 32, 64, 64, 128};
  const int dils[5] = {1, d->variant == 2 ? 1 : 3, 1, d->variant == 2 ? 1 : 3, 1};
  const bool pool_after[5] = {d->variant == 2, d->variant != 2, d->variant == 2, d->variant != 2, d->variant == 2};
  const int clast = chans[nl];
  if (d->n_feat <= 0 || d->n_feat % clast) return MAGAT_ERR_BAD_SHAPE;
  for (int m0 = 0; m0 < M; m0 += b.mc) {
    const int mm = (M - m0) < b.mc ? (M - m0) : b.mc;
    int rc = magat_conv_first_tiled_f32(x + (size_t)m0 * 3 * H * W, pk + d->off[enc::STEM_W], pk + d->off[enc::STEM_B], buf[0], mm,
                                        H, W, stream);
    if (rc != MAGAT_OK) return rc;
    int cur = 0, hp = H, wp = W;          // physical size of the map in buf[cur]
    const bool last_pooled = pool_after[nl - 1];
    for (int l = 1; l < nl; ++l) {
      const bool pooled = pool_after[l - 1];                // the previous layer was followed by a pool
      const int hin = pooled ? hp / 2 : hp, win = pooled ? wp / 2 : wp;
      const bool to_feat = l == nl - 1 && !last_pooled;      // the last map IS the feature row: [cell][channel]
      magat_conv_gemm_desc g = {};
      g.in = buf[cur]; g.wt = pk + d->off[enc::plain_w(l - 1)]; g.bias = pk + d->off[enc::plain_b(l - 1)];
      g.out = to_feat ? feat + (size_t)m0 * ldfeat : buf[(cur + 1) % 3];
      g.in_pix_stride = enc_pixs(chans[l]); g.out_pix_stride = to_feat ? chans[l + 1] : enc_pixs(chans[l + 1]);
      g.in_tile_stride = enc_tiles(hp * wp, chans[l]); g.out_tile_stride = to_feat ? 0 : enc_tiles(hin * win, chans[l + 1]);
      g.M = mm; g.Cin = chans[l]; g.lda = chans[l]; g.Hin = hin; g.Win = win; g.kH = g.kW = 3; g.stride = 1;
      g.pad = dils[l]; g.dilation = dils[l];
      g.Hout = hin; g.Wout = win; g.Cout = chans[l + 1]; g.ldc = to_feat ? ldfeat : chans[l + 1]; g.relu = 1;
      g.tag = MAGAT_TAG_BLOCK_CONV + (l - 1);
      if (pooled) { g.pool = 2; g.pool_w = wp; }
      rc = magat_conv_gemm_f32(&g, stream);
      if (rc != MAGAT_OK) return rc;
      cur = (cur + 1) % 3; hp = hin; wp = win;
    }
    const int hf = last_pooled ? hp / 2 : hp, wf = last_pooled ? wp / 2 : wp;
    if (hf < 1 || wf < 1 || d->n_feat != clast * hf * wf) return MAGAT_ERR_BAD_SHAPE;
    if (last_pooled) {
      // final MaxPool2d(2) -> feat [mm][hf wf][clast]: a pooled 1x1 GEMM with identity weights, one output pixel per pooled
      // cell.  At the reference's FOV = 9 (11 x 11 maps) the Default CNN ends on one cell; at other map sizes (and for the
      // dilated variants) the features are (cell, channel)-ordered here where the reference's Flatten is (channel, cell)-
      // ordered - encoder.fold_default_cnn / fold_dilated_cnn permute the columns of every weight that reads them
      magat_conv_gemm_desc g = {};
      g.in = buf[cur]; g.wt = pk + d->off[enc::HEAD_W]; g.out = feat + (size_t)m0 * ldfeat;
      g.in_pix_stride = enc_pixs(clast); g.in_tile_stride = enc_tiles(hp * wp, clast);
      g.M = mm; g.Cin = clast; g.lda = clast; g.Hin = hf; g.Win = wf;
      g.kH = 1; g.kW = 1; g.stride = 1; g.pad = 0; g.Hout = hf; g.Wout = wf; g.Cout = clast; g.ldc = ldfeat;
      g.out_pix_stride = clast;
      g.pool = 2; g.pool_w = wp; g.tag = MAGAT_TAG_HEAD;
      rc = magat_conv_gemm_f32(&g, stream);
      if (rc != MAGAT_OK) return rc;
    }
    if (d->n_comp > 0) {
      rc = magat_linear_tagged_f32(feat + (size_t)m0 * ldfeat, ldfeat, pk + d->off[enc::COMP_W], pk + d->off[enc::COMP_B],
                                   comp + (size_t)m0 * ldcomp, ldcomp, mm, d->n_comp, d->n_feat, 1,
                                   MAGAT_TAG_COMPRESS, stream);
      if (rc != MAGAT_OK) return rc;
    }
  }
  if (enc::bf16_rows_wanted(d->comp_bf16 != nullptr, d->n_comp))
    return magat_cast_rows(comp, d->comp_bf16, 1, M, d->n_comp, ldcomp, d->n_comp, stream);
  return MAGAT_OK;
}

extern "C" int magat_encoder_forward_f32(const magat_encoder_desc* d, const float* x, float* feat, int ldfeat,
                                         float* comp, int ldcomp, void* workspace, size_t workspace_bytes, int M,
                                         void* stream) {
  if (!d || !x || !feat || !d->pack) return MAGAT_ERR_NULL;
  if (M <= 0 || d->H < 3 || d->W < 3 || d->n_feat <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (d->variant < 0 || d->variant > 4) return MAGAT_ERR_UNSUPPORTED;
  if (d->n_comp > 0 && !comp) return MAGAT_ERR_NULL;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) ||
      workspace_bytes < magat_encoder_workspace_bytes(d, M))
    return MAGAT_ERR_WORKSPACE;
  const EncBuffers b = enc_buffers(d, M, workspace);
  if (d->variant >= 2) return enc_run_plain_cnn(d, x, feat, ldfeat, comp, ldcomp, b, M, stream);
  hipStream_t st = static_cast<hipStream_t>(stream);

  // ResNet encoders.  With the range guard on (default) the split-arithmetic pass reports clamps into status[0] and a
  // float32-MFMA pass of the whole encoder follows in the same stream, every launch of it predicated on that flag: when no
  // value left the f16 planes' range (always, for sane checkpoints) those launches return at once; when one did, feat / comp
  // are recomputed in true fp32 before anything downstream reads them.
  int32_t* status = b.status;
  EncPass fwd = {enc::PASS_FORWARD};
  fwd.range_flag = status;
  int rc = enc_run_resnet(d, x, feat, ldfeat, comp, ldcomp, b, M, stream, fwd);
  if (rc != MAGAT_OK || fwd.guard == enc::GUARD_NONE) return rc;
  if (fwd.guard == enc::GUARD_LAT) {
    if (fwd.bf16_after_guard)
      rc = magat_cast_rows_if(comp, d->comp_bf16, 1, M, d->n_comp, ldcomp, d->n_comp, stream, status + 2);
    return rc;
  }
  const int pid = magat_prof_begin(MAGAT_TAG_RANGE_GUARD, st);
  EncPass re = {enc::PASS_RERUN};
  re.run_if = status; re.book = status;
  rc = enc_run_resnet(d, x, feat, ldfeat, comp, ldcomp, b, M, stream, re);
  if (rc == MAGAT_OK && !re.booked) {
    hipLaunchKernelGGL(guard_count_kernel, dim3(1), dim3(1), 0, st, status);
    if (hipGetLastError() != hipSuccess) rc = MAGAT_ERR_LAUNCH;
  }
  // the bf16 rows follow a re-run (status[2] = this forward's flag by now): a launch that returns at once otherwise
  if (rc == MAGAT_OK && fwd.bf16_after_guard)
    rc = magat_cast_rows_if(comp, d->comp_bf16, 1, M, d->n_comp, ldcomp, d->n_comp, stream, status + 2);
  magat_prof_end(pid, st);
  return rc;
}

extern "C" int magat_encoder_calibrate_f32(const magat_encoder_desc* d, const float* x, float* feat, int ldfeat, float* comp,
                                           int ldcomp, void* workspace, size_t workspace_bytes, int M, float* absmax,
                                           void* stream) {
  if (!d || !x || !feat || !d->pack || !absmax) return MAGAT_ERR_NULL;
  if (M <= 0 || d->H < 3 || d->W < 3 || d->n_feat <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (d->variant != 0 && d->variant != 1) return MAGAT_ERR_UNSUPPORTED;      // (the Default CNN runs in float32: nothing to scale)
  if (d->n_comp > 0 && !comp) return MAGAT_ERR_NULL;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) || workspace_bytes < magat_encoder_workspace_bytes(d, M))
    return MAGAT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(absmax, 0, 16 * sizeof(float), st) != hipSuccess) return MAGAT_ERR_LAUNCH;
  EncPass cal = {enc::PASS_CALIBRATE};
  cal.absmax = absmax;
  return enc_run_resnet(d, x, feat, ldfeat, comp, ldcomp, enc_buffers(d, M, workspace), M, stream, cal);
}
