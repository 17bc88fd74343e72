// GraphFilterBatchAttentional.forward (KeyQuery attention) as ONE launch of matrix-core products for the PUBLISHED feature widths
// on graphs of 33 .. 128 agents: G = F in {32, 64}, K = 2 | 3 - the released "MAGAT F-32-P4 / B-32-P4" checkpoints
// (scripts/train_DMap.sh:42-46) evaluated on the README's 30 / 40 / 50 / 60 / 100-robot generalisation sets (README.md:372-390;
// reference utils/graphUtils/graphML.py:4636-4671, 1724-1827, 1180-1286).  gat_small.hip covers N <= 32 (a wave per instance),
// gat_mfma.hip G = 128; before round 6 these shapes took the two-launch form (maps GEMM + gat_dense_kernel, Z through HBM:
// 194 us per 512 x 100 agents at F = 32).  Same algebra and f16x3 arithmetic as gat_small.hip (two f16 planes per operand,
// three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation; per instance and head):
//   G1  Q[j][g]   = sum_f X[j][f] W_p[g][f]
//   G2  E^T[j][i] = sum_g Q[j][g] X[i][g]; masked softmax over j in the accumulator layout (a lane owns column i) -> A planes
//   G3  U_k[i][c] = sum_f X[i][f] H_pk[c][f],  k = 0..K-1
//   hops acc_k[j][c] += sum_i A[j][i] U^T[c][i],  k = K-2 .. 0  (Horner);  Y_p = relu(acc_0 2^-8 + bias) | head mean
// organised by ROW TILES: a workgroup of NT = ceil(N / 32) waves owns a planning instance, wave w the agents 32 w .. 32 w + 31 -
// as rows j of Q (G1), as columns i of the score tile (G2: its rows of the attention matrix, softmax in registers over all NT
// row tiles), as rows i of U_k (G3) and as output rows j of the hops.  X, Q / U^T (one region: Q is dead when U^T is written)
// and A planes are workgroup LDS (140 KB at N = 128, F = 64; 54 KB at N <= 64: two workgroups per CU); four or five workgroup
// barriers per head.  Weights come straight from the row-major f16 planes of the layer's pack (L2 / L1 hits), the edge masks
// from coalesced row reads of S + ballots.  Values beyond the f16 range raise range_flag: the caller's predicated float32 form
// rewrites the output (its LDS tiles reach N = 128 at these widths).
// G = F = 128 on 103 .. 128 agents (XR form, round 6): every use of the X planes is of the wave's OWN row tile, so they need no LDS
// at all - a lane keeps its operand fragments of row 32 w + lane % 32 in 64 registers, read straight from HBM in that layout.  What
// is left - Q / U^T and A planes - is 139 KB: the one-launch form gat_mfma.hip (162 KB per instance, ends at N = 102) cannot reach.
#include "magat_common.h"
#include "f16x3.h"
#include "gat_route.h"


#ifdef MAGAT_DEBUG_HOOKS
// phase stamps (debug builds: tools/exp/mid_phase_probe.py): [workgroup][wave][16] cycle counters of the LAST head a wave ran
#define MID_STAMP(i) do { if (p.dbg && (threadIdx.x & 63) == 0) p.dbg[((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
static long long* g_gat_mid_dbg = nullptr;
extern "C" int magat_gat_mid_set_debug_buffer(long long* dev_buf) { g_gat_mid_dbg = dev_buf; return MAGAT_OK; }
#else
#define MID_STAMP(i) do { } while (0)
#endif

namespace {

struct GatMidParams {
  const float* X;             // [B*N][ldx]
  const void* S;              // [B][N][N] f32 | f64
  const unsigned short* Hs;   // f16 planes [2][NC][G] of 2^8 Bt (rows: [P][G] W_p, then [P][K][F] H_pk)
  const float* bias;          // [F] or null
  float* Y;                   // [B*N][ldy]
  int B, N, P, NC, ldx, ldy, s_is_f64;
  int* range_flag;
  const float* x_scale;
  const char* wfrag;          // XR (G = 128): the same planes fragment-major (gat_mfma.hip's stream: 64 KB blocks [P] W_p, [P K] H_pk,
                              // a block = [32-row tile 4][k step 8][plane 2][lane 64][8 halves]) - one coalesced 1 KB read per fragment
  long long* dbg;             // debug builds: phase stamps
  float* Ypre; int ldpre;     // HS, head-mean: the heads' pre-activation outputs [B*N][P F] (the caller's workspace); a small kernel forms the mean
};

// HS (few instances: the batch-1 step of the reference's inference loop): a workgroup per (instance, HEAD) instead of per instance -
// one planning instance of 100 agents then runs on four CUs instead of one.  A head's arithmetic does not change; with head-mean
// the workgroups leave their pre-activation outputs in Ypre and gat_mid_mean_kernel sums them in the loop's order (bit-identical).
// rows whose scaled norm is below this have lost their direction in the f16 planes: the range flag (see gat_small.hip, kCosTiny)
constexpr float kMidCosTiny = 0.125f;
template <int F, int KT, int NT, bool CONCAT, bool HS = false, bool XR = false>
__global__ __launch_bounds__(64 * NT) void gat_mid_kernel(const GatMidParams p) {
  constexpr bool COS = false;
#include "gat_mid_body.inc"
}
// the cosine form (GAT_Similarity): one head, so the concat instantiation serves both merges and there is no head split
template <int F, int KT, int NT, bool XR = false>
__global__ __launch_bounds__(64 * NT) void gat_mid_cos_kernel(const GatMidParams p) {
  constexpr bool COS = true, CONCAT = true, HS = false;
#include "gat_mid_body.inc"
}

// head mean of the head-split form: y = relu((((0 + v_0) + v_1) + ..) / P) - the non-split kernel's sum, in its order
__global__ __launch_bounds__(256) void gat_mid_mean_kernel(const float* __restrict__ ypre, float* __restrict__ y, long long M, int P, int F,
                                                           int ldpre, int ldy) {
  const long long total = M * F;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += gridDim.x * 256LL) {
    const long long m = idx / F;
    const int c = (int)(idx - m * F);
    float s = 0.f;
    for (int q = 0; q < P; ++q) s += ypre[m * ldpre + q * F + c];
    y[m * ldy + c] = __builtin_amdgcn_fmed3f(s / (float)P, 0.f, __builtin_inff());
  }
}

template <int F, int NT, bool XR = false>
constexpr size_t mid_lds() {
  constexpr size_t ROWS = 32 * NT, RS = 2 * F + 16, SA = 2 * ROWS + 16;
  constexpr size_t q = 2 * ROWS * RS, u = 2 * F * SA;
  return (XR ? 0 : 2 * ROWS * RS) + (q > u ? q : u) + 2 * ROWS * SA;
}

// workgroups of a launch without head split: as many as fit the chip's LDS at once (at most four per CU), they walk the rest
inline long long mid_blocks(int B, size_t lds, int cus) {
  long long per_cu = (long long)(magat_gat::kLdsBytes / lds);
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 4) per_cu = 4;
  return B > cus * per_cu ? cus * per_cu : B;
}

// slot: LDS-attribute slots of the four kernels of this (width, taps, row tiles) class - concat, mean, and the two head-split forms
// f.hsplit (few instances, the batch-1 step): a workgroup per (instance, head); head-mean then needs the caller's scratch rows
template <int F, int KT, int NT, bool XR = false>
int launch_mid(const GatMidParams& p, int concat, int slot, int slot_hs, const magat_gat::OneLaunch& f, hipStream_t st) {
  constexpr size_t lds = mid_lds<F, NT, XR>();
  static_assert(lds <= magat_gat::kLdsBytes, "LDS");
  const void* fn = concat ? reinterpret_cast<const void*>(&gat_mid_kernel<F, KT, NT, true, false, XR>)
                          : reinterpret_cast<const void*>(&gat_mid_kernel<F, KT, NT, false, false, XR>);
  if (magat_ensure_dyn_lds(fn, slot + (concat ? 0 : 1), lds) != MAGAT_OK) return MAGAT_ERR_LAUNCH;
  const long long blocks = mid_blocks(p.B, lds, f.cus);
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_LAYER, st);
  if (f.hsplit) {
    const void* fh = concat ? reinterpret_cast<const void*>(&gat_mid_kernel<F, KT, NT, true, true, XR>)
                            : reinterpret_cast<const void*>(&gat_mid_kernel<F, KT, NT, false, true, XR>);
    if (magat_ensure_dyn_lds(fh, slot_hs + (concat ? 0 : 1), lds) != MAGAT_OK) {
      magat_prof_end(pid, st);
      return MAGAT_ERR_LAUNCH;
    }
    const unsigned g = (unsigned)(p.B * p.P);
    if (concat) hipLaunchKernelGGL((gat_mid_kernel<F, KT, NT, true, true, XR>), dim3(g), dim3(64 * NT), lds, st, p);
    else {
      hipLaunchKernelGGL((gat_mid_kernel<F, KT, NT, false, true, XR>), dim3(g), dim3(64 * NT), lds, st, p);
      const long long M = (long long)p.B * p.N;
      hipLaunchKernelGGL(gat_mid_mean_kernel, dim3((unsigned)((M * F + 255) / 256)), dim3(256), 0, st, p.Ypre, p.Y, M, p.P, F, p.ldpre, p.ldy);
    }
    magat_form_note(MAGAT_FORM_GAT_HSPLIT);
  } else if (concat) hipLaunchKernelGGL((gat_mid_kernel<F, KT, NT, true, false, XR>), dim3((unsigned)blocks), dim3(64 * NT), lds, st, p);
  else {
    hipLaunchKernelGGL((gat_mid_kernel<F, KT, NT, false, false, XR>), dim3((unsigned)blocks), dim3(64 * NT), lds, st, p);
    if (XR) {      // (its head mean: the same sum in the same order, from the pre-activation rows)
      const long long M = (long long)p.B * p.N;
      long long mb = (M * F + 255) / 256;
      if (mb > 4096) mb = 4096;
      hipLaunchKernelGGL(gat_mid_mean_kernel, dim3((unsigned)mb), dim3(256), 0, st, p.Ypre, p.Y, M, p.P, F, p.ldpre, p.ldy);
    }
  }
  magat_prof_end(pid, st);
  magat_form_note(MAGAT_FORM_GAT_MID);
  return magat_check_launch();
}

template <int F, int KT, int NT, bool XR = false>
int launch_mid_cos(const GatMidParams& p, int slot, int cus, hipStream_t st) {
  constexpr size_t lds = mid_lds<F, NT, XR>() + 32 * NT * sizeof(float);      // + qn[ROWS]
  static_assert(lds <= magat_gat::kLdsBytes, "LDS");
  if (magat_ensure_dyn_lds(reinterpret_cast<const void*>(&gat_mid_cos_kernel<F, KT, NT, XR>), slot, lds) != MAGAT_OK) return MAGAT_ERR_LAUNCH;
  const long long blocks = mid_blocks(p.B, lds, cus);
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_LAYER, st);
  hipLaunchKernelGGL((gat_mid_cos_kernel<F, KT, NT, XR>), dim3((unsigned)blocks), dim3(64 * NT), lds, st, p);
  magat_prof_end(pid, st);
  magat_form_note(MAGAT_FORM_GAT_MID);
  return magat_check_launch();
}
template <int F, int KT>
int launch_mid_cos_nt(const GatMidParams& p, int slot, int cus, hipStream_t st) {
  const int nt = (p.N + 31) / 32;
  if (nt == 2) return launch_mid_cos<F, KT, 2>(p, slot, cus, st);
  if (nt == 3) return launch_mid_cos<F, KT, 3>(p, slot + 1, cus, st);
  return launch_mid_cos<F, KT, 4>(p, slot + 2, cus, st);
}

template <int F, int KT>
int launch_mid_nt(const GatMidParams& p, int concat, int slot, const magat_gat::OneLaunch& f, hipStream_t st) {
  const int nt = (p.N + 31) / 32;
  if (nt == 2) return launch_mid<F, KT, 2>(p, concat, slot, slot + 24, f, st);
  if (nt == 3) return launch_mid<F, KT, 3>(p, concat, slot + 2, slot + 26, f, st);
  return launch_mid<F, KT, 4>(p, concat, slot + 4, slot + 28, f, st);
}

}  // namespace

// head mean of pre-activation rows [M][ldpre >= P F] (gat_mfma.hip's head-split form merges its heads with it too)
int magat_gat_mean_launch(const float* ypre, float* y, long long M, int P, int F, int ldpre, int ldy, hipStream_t st) {
  long long mb = (M * F + 255) / 256;
  if (mb > 4096) mb = 4096;
  hipLaunchKernelGGL(gat_mid_mean_kernel, dim3((unsigned)mb), dim3(256), 0, st, ypre, y, M, P, F, ldpre, ldy);
  return magat_check_launch();
}

// Hs: the f16 planes [2][NC][G] of the layer's pack (packed + magat_gat_f16_block_offset(NC, G))
int magat_gat_mid_forward(const float* X, int ldx, const void* S, int s_is_f64, const float* Hs, int NC, const float* bias, float* Y,
                          int ldy, int B, int N, int G, int K, int P, int concat, int* range_flag, hipStream_t st,
                          const float* x_scale, float* ypre, int ldpre, const float* wfrag, int cosine,
                          const magat_gat::OneLaunch& form) {
  // (at most four row tiles, the instantiated widths - 128 features as four row tiles only -, 16-byte reads of the X rows)
  if (N > 128 || (G != 32 && G != 64 && G != 128) || (G == 128 && N < 97)) return MAGAT_ERR_UNSUPPORTED;
  if ((ldx & 3) || (reinterpret_cast<uintptr_t>(X) & 15)) return MAGAT_ERR_UNSUPPORTED;
  GatMidParams p;
  p.X = X; p.S = S; p.Hs = reinterpret_cast<const unsigned short*>(Hs); p.bias = bias; p.Y = Y;
  p.B = B; p.N = N; p.P = P; p.NC = NC; p.ldx = ldx; p.ldy = ldy; p.s_is_f64 = s_is_f64;
  p.range_flag = range_flag; p.x_scale = x_scale;
  p.dbg = nullptr;
#ifdef MAGAT_DEBUG_HOOKS
  p.dbg = g_gat_mid_dbg;
#endif
  p.Ypre = (ypre && ldpre >= P * G) ? ypre : nullptr; p.ldpre = ldpre;
  p.wfrag = reinterpret_cast<const char*>(wfrag);
  if (G == 128 && !wfrag) return MAGAT_ERR_NULL;
  if (cosine) {      // LDS-attribute slots: three row-tile counts per (width, taps) pair, then the two of the 128-wide form
    if (G == 128) return K == 3 ? launch_mid_cos<128, 3, 4, true>(p, MAGAT_LDS_GATD_COS_0 + 12, form.cus, st)
                                : launch_mid_cos<128, 2, 4, true>(p, MAGAT_LDS_GATD_COS_0 + 13, form.cus, st);
    if (G == 32) return K == 3 ? launch_mid_cos_nt<32, 3>(p, MAGAT_LDS_GATD_COS_0, form.cus, st) : launch_mid_cos_nt<32, 2>(p, MAGAT_LDS_GATD_COS_0 + 3, form.cus, st);
    return K == 3 ? launch_mid_cos_nt<64, 3>(p, MAGAT_LDS_GATD_COS_0 + 6, form.cus, st) : launch_mid_cos_nt<64, 2>(p, MAGAT_LDS_GATD_COS_0 + 9, form.cus, st);
  }
  // (the 128-wide form always merges heads through Ypre, a head split without concat too)
  if ((G == 128 || form.hsplit) && !concat && !p.Ypre) return MAGAT_ERR_WORKSPACE;
  // LDS-attribute slots: 6 per (width, taps) pair (three tile counts x two merges), 24 more for their head-split forms, then the
  // eight of the 128-wide form (taps x merge, + head split)
  if (G == 128)
    return K == 3 ? launch_mid<128, 3, 4, true>(p, concat, MAGAT_LDS_GATD_0 + 48, MAGAT_LDS_GATD_0 + 52, form, st)
                  : launch_mid<128, 2, 4, true>(p, concat, MAGAT_LDS_GATD_0 + 50, MAGAT_LDS_GATD_0 + 54, form, st);
  if (G == 32) return K == 3 ? launch_mid_nt<32, 3>(p, concat, MAGAT_LDS_GATD_0, form, st) : launch_mid_nt<32, 2>(p, concat, MAGAT_LDS_GATD_0 + 6, form, st);
  return K == 3 ? launch_mid_nt<64, 3>(p, concat, MAGAT_LDS_GATD_0 + 12, form, st) : launch_mid_nt<64, 2>(p, concat, MAGAT_LDS_GATD_0 + 18, form, st);
}
