// GraphFilterBatchAttentional.forward (KeyQuery attention) for SMALL graphs and NARROW features as one launch of matrix-core
// products: N <= 32 agents, G = F in {32, 64}, K = 2 | 3 - the published MAGAT settings (scripts/train_DMap.sh:42-46: 10 agents,
// bottleneckFeature 32, four heads; reference utils/graphUtils/graphML.py:4636-4671, 1724-1827, 1180-1286).  Same algebra and the
// same f16x3 arithmetic as gat_mfma.hip (two f16 planes per operand, three v_mfma_f32_32x32x16_f16 per product, fp32
// accumulation; per instance b and head p):
//   G1  Q[j][g]   = sum_f X[j][f] W_p[g][f]           (operands swapped: the tile is Q^T, the planes are stored as they are)
//   G2  E^T[j][i] = sum_g Q[j][g] X[i][g]; masked softmax over j in the accumulator layout (a lane owns column i) -> A planes
//   G3  U_k[i][c] = sum_f X[i][f] H_pk[c][f],  k = 0..K-1
//   hops acc_k[j][c] += sum_i A[j][i] U^T[c][i],  k = K-2 .. 0  (Horner);  Y_p = relu(acc_0 2^-8 + bias) | head mean
// but organised the other way round: a graph of <= 32 agents is ONE 32-row tile, so A WAVE OWNS A PLANNING INSTANCE - its X, Q, A
// and U^T planes are wave-private LDS (20-34 KB per wave), no workgroup barrier exists in the kernel, and the head mean is summed
// in the wave's registers.  Weights are read straight from the row-major f16 planes of the layer's pack (magat_gat_pack_weights:
// [2][NC][G] halves of 2^8 Bt: a lane's MFMA row operand is 16 contiguous bytes of a weight row; 16 KB per head at G = 32, L2 /
// L1 hits).  Values beyond the f16 range raise range_flag and the caller's predicated two-launch float32 form rewrites the output.
#include "magat_common.h"
#include "f16x3.h"
#include "gat_route.h"

namespace {

struct GatSmallParams {
  const float* X;             // [B*N][ldx]
  const void* S;              // [B][N][N] f32 | f64
  const unsigned* rmask_pre;  // [B][N][4] edge masks of a GSO plan (word 0 used), or null
  const unsigned short* Hs;   // f16 planes [2][NC][G] of 2^8 Bt (rows: [P][G] W_p, then [P][K][F] H_pk)
  const float* bias;          // [F] or null
  float* Y;                   // [B*N][ldy]
  int B, N, P, NC, ldx, ldy, s_is_f64;
  int* range_flag;
  const float* x_scale;
};

// COS (GAT_Similarity, graphML.py:1449-1564; one head): cosine scores e_ij = x_i . q_j / (max(|x_i|, 1e-9) max(|q_j|, 1e-9)) under
// GAT_origin's mask |float(S) + I| > 1e-9.  A lane owns agent fr both as row j of Q in G1 and as column i of the score tile in G2:
// |q_j|^2 comes from its G1 accumulators (all column tiles, + the lane ^ 32 partner) in float32 before the plane split and leaves
// 1 / max(|q_j|, 1e-9) in a wave-private LDS array [32]; |x_i|^2 from the float32 X row; the G2 epilogue scales the scores and the
// softmax runs with plain log2(e) (the cosine does not depend on x_scale).  A non-zero row whose scaled norm is below kCosTiny
// has lost its DIRECTION in the f16 planes (their absolute step is 2^-24): it raises the range flag like an overflow, and the
// caller's predicated float32 form (maps GEMM, gat_cos_prepare_kernel, gat_dense_kernel) rewrites the output.
constexpr float kCosTiny = 0.125f;
template <int F, int KT, bool CONCAT>
__global__ __launch_bounds__(256, F == 32 ? 2 : 1) void gat_small_kernel(const GatSmallParams p) {      // (32 features: two waves per SIMD - a second workgroup per CU at large batches)
  constexpr bool COS = false;
#include "gat_small_body.inc"
}
// the cosine form: one head, so one merge instantiation serves both merges (relu(y / 1) = relu(y), the same rows of Y)
template <int F, int KT>
__global__ __launch_bounds__(256, F == 32 ? 2 : 1) void gat_small_cos_kernel(const GatSmallParams p) {
  constexpr bool COS = true, CONCAT = true;
#include "gat_small_body.inc"
}


template <int F, int KT>
int launch_small(const GatSmallParams& p, int concat, int slot, int cus, hipStream_t st, bool cosine = false) {
  constexpr size_t wlds = 128 * (2 * F + 16) + 64 * 80 + 2 * F * 80;
  const size_t lds = 4 * (wlds + (cosine ? 128 : 0));
  if (cosine) concat = 1;
  const void* fn = cosine ? reinterpret_cast<const void*>(&gat_small_cos_kernel<F, KT>)
                   : concat ? reinterpret_cast<const void*>(&gat_small_kernel<F, KT, true>)
                          : reinterpret_cast<const void*>(&gat_small_kernel<F, KT, false>);
  if (magat_ensure_dyn_lds(fn, slot + (concat ? 0 : 1), lds) != MAGAT_OK) return MAGAT_ERR_LAUNCH;
  // a wave per instance, four instances per workgroup
  long long blocks = ((long long)p.B + 3) / 4;
  const long long cap = (long long)cus * (lds <= 80 * 1024 ? 2 : 1);
  if (blocks > cap) blocks = cap;
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_LAYER, st);
  if (cosine) hipLaunchKernelGGL((gat_small_cos_kernel<F, KT>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else if (concat) hipLaunchKernelGGL((gat_small_kernel<F, KT, true>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  else hipLaunchKernelGGL((gat_small_kernel<F, KT, false>), dim3((unsigned)blocks), dim3(256), lds, st, p);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

}  // namespace

// Hs: the f16 planes [2][NC][G] of the layer's pack (packed + magat_gat_f16_block_offset(NC, G))
int magat_gat_small_forward(const float* X, int ldx, const void* S, int s_is_f64, const unsigned* rmask_pre, const float* Hs,
                            int NC, const float* bias, float* Y, int ldy, int B, int N, int G, int K, int P, int concat,
                            int* range_flag, hipStream_t st, const float* x_scale, int cosine, const magat_gat::OneLaunch& form) {
  // (one 32-row tile per wave, the instantiated widths, 16-byte reads of the X rows)
  if (N > 32 || (G != 32 && G != 64) || (ldx & 3) || (reinterpret_cast<uintptr_t>(X) & 15)) return MAGAT_ERR_UNSUPPORTED;
  GatSmallParams p;
  p.X = X; p.S = S; p.rmask_pre = rmask_pre; p.Hs = reinterpret_cast<const unsigned short*>(Hs); p.bias = bias; p.Y = Y;
  p.B = B; p.N = N; p.P = P; p.NC = NC; p.ldx = ldx; p.ldy = ldy; p.s_is_f64 = s_is_f64;
  p.range_flag = range_flag; p.x_scale = x_scale;
  const int cus = form.cus;
  if (cosine) {
    if (G == 32) return K == 3 ? launch_small<32, 3>(p, 1, MAGAT_LDS_GATS_COS_0, cus, st, true) : launch_small<32, 2>(p, 1, MAGAT_LDS_GATS_COS_0 + 1, cus, st, true);
    return K == 3 ? launch_small<64, 3>(p, 1, MAGAT_LDS_GATS_COS_0 + 2, cus, st, true) : launch_small<64, 2>(p, 1, MAGAT_LDS_GATS_COS_0 + 3, cus, st, true);
  }
  if (G == 32) return K == 3 ? launch_small<32, 3>(p, concat, MAGAT_LDS_GATS_0, cus, st) : launch_small<32, 2>(p, concat, MAGAT_LDS_GATS_0 + 2, cus, st);
  return K == 3 ? launch_small<64, 3>(p, concat, MAGAT_LDS_GATS_0 + 4, cus, st) : launch_small<64, 2>(p, concat, MAGAT_LDS_GATS_0 + 6, cus, st);
}
