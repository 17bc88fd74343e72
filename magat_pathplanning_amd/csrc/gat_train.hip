// Backward of the graph layers on CSR graphs (the forward that keeps what it needs, magat_gat_train_forward_f32, runs the
// forward kernels and lives with them in gat_csr_f32.hip).
#include "magat_common.h"
#include "gat_pack.h"
#include "gat_csr_route.h"
#include "gat_cos_parts.h"

// =====================================================================================================
// Training support: forward that keeps what the backward needs, and the
// backward of the graph part of the layer.  The layer is
//     T_{K-1} = U_{K-1};  T_k = U_k + A^T T_{k+1};  Ypre = T_0 + bias;  A = row-softmax(E) on the edges
//     E_ij = x_i . q_j (KeyQuery)  |  lrelu(c1_j + c2_i) (GAT_modified);   [Q | U | c1 c2] = X @ Bt^T + cb
// Given dYpre the kernels below produce dZ (gradient wrt every column of Z) and the direct part of dX;
// the two dense products dX += dZ @ Bt and dBt = dZ^T @ X are plain library GEMMs done by the caller.
//     dT_0 = dYpre;   dT_{k+1} = A dT_k;   dA_ij = sum_k T_{k+1}[i] . dT_k[j];   dU_k = dT_k
//     dE_ij = a_ij (dA_ij - sum_j' a_ij' dA_ij')
//     KeyQuery: dX_i += sum_j dE_ij q_j,  dQ_j = sum_i dE_ij x_i
//     modified: g_ij = dE_ij * lrelu'(c1_j + c2_i),  dc2_i = sum_j g_ij,  dc1_j = sum_i g_ij
//     GAT_Similarity (magat_gat_train_backward_cos_f32): KeyQuery on the normalised rows (X = Xhat, Z's score columns = q^),
//     then dXd and dQ go back through the normalisation in place (gat_cos_backward_kernel, gat_cos_parts.h)
// =====================================================================================================
namespace {

struct TrainParams {
  const float* X;
  const float* Z;
  const float* T;        // [(K-2)][M][P*F]   T_k at slot K-2-k  (1 <= k <= K-2)
  const float* att;      // [P][nnz]
  float* datt;           // [P][nnz]  dA, then dE / g in place
  float* dZ;             // [M][NC]
  float* dXd;            // [M][G]
  const int* rowptr; const int* colidx; const int* cscptr; const int* cscsrc; const int* cscpos;
  int B, N, K, P, mode, NC, qoff, uoff, c1off, c2off;
  long long nnz, M;
  int k;                 // hop being differentiated (reads dT_k, writes dT_{k+1})
};

template <int F>
__global__ __launch_bounds__(256) void bwd_hop_kernel(const TrainParams p) {
  constexpr int VEC = F >= 64 ? F / 64 : 1, LANES = F >= 64 ? 64 : F;
  typedef float fvec __attribute__((ext_vector_type(VEC)));
  const int N = p.N, tiles = (N + 3) / 4;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD, per = p.P * tiles;
  const int b = xcd + MAGAT_NUM_XCD * (slot / per);
  if (b >= p.B) return;
  const int head = (slot % per) / tiles, tile = slot % tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = tile * 4 + wave;
  if (i >= N) return;
  const bool on = lane < LANES;
  const int* rp = p.rowptr + (long long)b * (N + 1);
  const int e0 = rp[i], e1 = rp[i + 1];
  const float* att = p.att + (long long)head * p.nnz;
  float* datt = p.datt + (long long)head * p.nnz;
  const long long row0 = (long long)b * N;
  const int k = p.k, K = p.K;
  // T_{k+1}[i]
  fvec tn;
#pragma unroll
  for (int c = 0; c < VEC; ++c) tn[c] = 0.f;
  if (on) {
    if (k + 1 == K - 1)
      tn = *reinterpret_cast<const fvec*>(p.Z + (row0 + i) * p.NC + p.uoff + (head * K + (K - 1)) * F + VEC * lane);
    else
      tn = *reinterpret_cast<const fvec*>(p.T + ((long long)(K - 2 - (k + 1)) * p.M + row0 + i) * p.P * F + head * F +
                                          VEC * lane);
  }
  const long long ucur = p.uoff + (head * K + k) * F + VEC * lane;       // dT_k lives in dZ's U_k block
  fvec acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int j = p.colidx[e];
    const float a = att[e];
    fvec d;
#pragma unroll
    for (int c = 0; c < VEC; ++c) d[c] = 0.f;
    if (on) d = *reinterpret_cast<const fvec*>(p.dZ + (row0 + j) * p.NC + ucur);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < VEC; ++c) {
      acc[c] = fmaf(a, d[c], acc[c]);
      dot = fmaf(tn[c], d[c], dot);
    }
    dot = wave_sum(dot);
    if (lane == 0) datt[e] = (k == 0 ? 0.f : datt[e]) + dot;
  }
  if (on) *reinterpret_cast<fvec*>(p.dZ + (row0 + i) * p.NC + p.uoff + (head * K + k + 1) * F + VEC * lane) = acc;
}

// softmax backward per row (all heads), then the row-side score gradients
template <int G>
__global__ __launch_bounds__(256) void bwd_scores_rows_kernel(const TrainParams p) {
  constexpr int VEC = G >= 64 ? G / 64 : 1, LANES = G >= 64 ? 64 : G;
  typedef float fvec __attribute__((ext_vector_type(VEC)));
  const int N = p.N, tiles = (N + 3) / 4;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int b = xcd + MAGAT_NUM_XCD * (slot / tiles);
  if (b >= p.B) return;
  const int tile = slot % tiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = tile * 4 + wave;
  if (i >= N) return;
  const bool on = lane < LANES;
  const int* rp = p.rowptr + (long long)b * (N + 1);
  const int e0 = rp[i], e1 = rp[i + 1];
  const long long row0 = (long long)b * N;
  fvec accx;
#pragma unroll
  for (int c = 0; c < VEC; ++c) accx[c] = 0.f;
  for (int head = 0; head < p.P; ++head) {
    const float* att = p.att + (long long)head * p.nnz;
    float* datt = p.datt + (long long)head * p.nnz;
    float s = 0.f;
    for (int e = e0 + lane; e < e1; e += 64) s = fmaf(att[e], datt[e], s);
    s = wave_sum(s);
    if (p.mode == MAGAT_MODE_KEYQUERY) {
      for (int e = e0; e < e1; ++e) {
        const float dE = att[e] * (datt[e] - s);
        if (on) {
          const fvec q = *reinterpret_cast<const fvec*>(p.Z + (row0 + p.colidx[e]) * p.NC + p.qoff + head * G + VEC * lane);
#pragma unroll
          for (int c = 0; c < VEC; ++c) accx[c] = fmaf(dE, q[c], accx[c]);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) datt[e] = dE;
      }
    } else {
      const float c2 = p.Z[(row0 + i) * p.NC + p.c2off + head];
      float g2 = 0.f;
      for (int e = e0 + lane; e < e1; e += 64) {
        const float pre = p.Z[(row0 + p.colidx[e]) * p.NC + p.c1off + head] + c2;
        const float g = att[e] * (datt[e] - s) * (pre > 0.f ? 1.f : 0.2f);
        datt[e] = g;
        g2 += g;
      }
      g2 = wave_sum(g2);
      if (lane == 0) p.dZ[(row0 + i) * p.NC + p.c2off + head] = g2;
    }
  }
  if (p.mode == MAGAT_MODE_KEYQUERY && on) *reinterpret_cast<fvec*>(p.dXd + (row0 + i) * G + VEC * lane) = accx;
}

// column-side score gradients: dQ_j (KeyQuery) or dc1_j (modified), via the CSC view
template <int G>
__global__ __launch_bounds__(256) void bwd_scores_cols_kernel(const TrainParams p) {
  constexpr int VEC = G >= 64 ? G / 64 : 1, LANES = G >= 64 ? 64 : G;
  typedef float fvec __attribute__((ext_vector_type(VEC)));
  const int N = p.N, tiles = (N + 3) / 4;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int b = xcd + MAGAT_NUM_XCD * (slot / tiles);
  if (b >= p.B) return;
  const int tile = slot % tiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = tile * 4 + wave;
  if (j >= N) return;
  const bool on = lane < LANES;
  const int* cp = p.cscptr + (long long)b * (N + 1);
  const int s0 = cp[j], s1 = cp[j + 1];
  const long long row0 = (long long)b * N;
  for (int head = 0; head < p.P; ++head) {
    const float* dE = p.datt + (long long)head * p.nnz;
    if (p.mode == MAGAT_MODE_KEYQUERY) {
      fvec acc;
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = 0.f;
      for (int s = s0; s < s1; ++s) {
        const float g = dE[p.cscpos[s]];
        if (on) {
          const fvec x = *reinterpret_cast<const fvec*>(p.X + (row0 + p.cscsrc[s]) * G + VEC * lane);
#pragma unroll
          for (int c = 0; c < VEC; ++c) acc[c] = fmaf(g, x[c], acc[c]);
        }
      }
      if (on) *reinterpret_cast<fvec*>(p.dZ + (row0 + j) * p.NC + p.qoff + head * G + VEC * lane) = acc;
    } else {
      float g1 = 0.f;
      for (int s = s0 + lane; s < s1; s += 64) g1 += dE[p.cscpos[s]];
      g1 = wave_sum(g1);
      if (lane == 0) p.dZ[(row0 + j) * p.NC + p.c1off + head] = g1;
    }
  }
}

// dU_0 = dYpre
__global__ void bwd_seed_kernel(const float* __restrict__ dY, float* __restrict__ dZ, long long M, int P, int F, int K,
                                int NC, int uoff) {
  const int FC = F / 4;
  const long long total = M * P * FC;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % FC);
    const long long r = idx / FC;
    const int head = (int)(r % P);
    const long long m = r / P;
    *reinterpret_cast<f32x4*>(dZ + m * NC + uoff + (head * K) * F + 4 * c) =
        *reinterpret_cast<const f32x4*>(dY + (m * P + head) * F + 4 * c);
  }
}


// ---- GraphFilterBatch backward (graphML.py:5485-5579 differentiated).  The layer is linear:  Y = b + sum_k A^k X H_k^T
// with A the row operator of "x @ S" (row n gathers S[m][n] X[m]: the CSC view in the forward).  Hence  dU_k = (A^T)^k dY
// - the same hop with the CSR rows of S as gather lists - and the rest is two plain GEMMs of the caller:
// dX = [dU_0 .. dU_{K-1}] Bt,  dH = dU^T X.   dZ [M][K*F]: slice k = dU_k.  One wave per agent row, 4 rows per workgroup.
template <int F>
__global__ __launch_bounds__(256) void gnn_bwd_hop_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                          const float* __restrict__ vals, float* __restrict__ dZ, int B,
                                                          int N, int K, int k) {
  constexpr int VEC = F >= 64 ? F / 64 : 1, LANES = F >= 64 ? 64 : F;
  typedef float fvec __attribute__((ext_vector_type(VEC)));
  const int tiles = (N + 3) / 4;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int b = xcd + MAGAT_NUM_XCD * (slot / tiles);
  if (b >= B) return;
  const int tile = slot % tiles, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = tile * 4 + wave;
  if (i >= N || lane >= LANES) return;
  const int* rp = rowptr + (long long)b * (N + 1);
  const int e0 = rp[i], e1 = rp[i + 1];
  const long long row0 = (long long)b * N, ld = (long long)K * F;
  const float* src = dZ + (long long)(k - 1) * F + VEC * lane;
  fvec acc;
#pragma unroll
  for (int c = 0; c < VEC; ++c) acc[c] = 0.f;
  for (int e = e0; e < e1; ++e) {
    const float a = vals[e];
    const fvec d = *reinterpret_cast<const fvec*>(src + (row0 + colidx[e]) * ld);
#pragma unroll
    for (int c = 0; c < VEC; ++c) acc[c] = fmaf(a, d[c], acc[c]);
  }
  *reinterpret_cast<fvec*>(dZ + (row0 + i) * ld + (long long)k * F + VEC * lane) = acc;
}

__global__ void gnn_bwd_seed_kernel(const float* __restrict__ dY, float* __restrict__ dZ, long long M, int F, int K) {
  const int FC = F / 4;
  const long long total = M * FC;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % FC);
    const long long m = idx / FC;
    *reinterpret_cast<f32x4*>(dZ + m * K * F + 4 * c) = *reinterpret_cast<const f32x4*>(dY + m * F + 4 * c);
  }
}

using magat_csr::rows_grid;      // workgroups of a wave-per-row launch (gat_csr_route.h)
using magat_csr::dims_ok;
using magat_csr::kGridMax;

template <int W, typename KFn>
int launch_rows(KFn kern, const TrainParams& p, int per_instance_factor, hipStream_t st) {
  const long long grid = rows_grid(p.B, p.N, per_instance_factor);
  if (grid > kGridMax) return MAGAT_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, st, p);
  return magat_check_launch();
}

}  // namespace

extern "C" int magat_gat_train_backward_f32(const float* dYpre, const float* X, const float* Z, const float* att,
                                            const float* T, const int* rowptr, const int* colidx, const int* cscptr,
                                            const int* cscsrc, const int* cscpos, long long nnz, float* dZ, float* dXd,
                                            float* datt, int B, int N, int G, int F, int K, int P, int mode,
                                            void* stream) {
  if (!dYpre || !X || !Z || !att || !rowptr || !cscptr || !cscsrc || !cscpos || !dZ || !dXd || !datt) return MAGAT_ERR_NULL;
  if (nnz > 0 && !colidx) return MAGAT_ERR_NULL;
  if (K > 2 && !T) return MAGAT_ERR_NULL;
  if (!dims_ok(B, N, nnz, K, P)) return MAGAT_ERR_BAD_SHAPE;
  if (mode < MAGAT_MODE_KEYQUERY || mode > MAGAT_MODE_GAT_ORIGIN) return MAGAT_ERR_UNSUPPORTED;
  if (G != F || !supported_width(G)) return MAGAT_ERR_UNSUPPORTED;
  // the largest grid of the call (the hops: P heads per instance), refused here and not behind the memsets and the seed launch
  if (K > 1 && rows_grid(B, N, P) > kGridMax) return MAGAT_ERR_BAD_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PackLayout L = pack_layout(G, F, K, P, mode);
  TrainParams p = {};
  p.X = X; p.Z = Z; p.T = T; p.att = att; p.datt = datt; p.dZ = dZ; p.dXd = dXd;
  p.rowptr = rowptr; p.colidx = colidx; p.cscptr = cscptr; p.cscsrc = cscsrc; p.cscpos = cscpos;
  p.B = B; p.N = N; p.K = K; p.P = P; p.mode = mode; p.NC = L.NC; p.qoff = L.qoff; p.uoff = L.uoff;
  p.c1off = L.c1off; p.c2off = L.c2off; p.nnz = nnz; p.M = (long long)B * N;
  if (hipMemsetAsync(dZ, 0, (size_t)p.M * L.NC * sizeof(float), st) != hipSuccess) return MAGAT_ERR_LAUNCH;
  if (hipMemsetAsync(dXd, 0, (size_t)p.M * G * sizeof(float), st) != hipSuccess) return MAGAT_ERR_LAUNCH;
  {
    long long blocks = (p.M * P * (F / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bwd_seed_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dYpre, dZ, p.M, P, F, K, L.NC, L.uoff);
    int rc = magat_check_launch();
    if (rc != MAGAT_OK) return rc;
  }
  if (K == 1) return MAGAT_OK;     // no graph terms: dZ = [0 | dYpre]
  int rc = MAGAT_OK;
  for (int k = 0; k <= K - 2; ++k) {
    p.k = k;
    MAGAT_WIDTH_SWITCH(F, rc = launch_rows<WW>(bwd_hop_kernel<WW>, p, P, st));
    if (rc != MAGAT_OK) return rc;
  }
  MAGAT_WIDTH_SWITCH(G, rc = launch_rows<WW>(bwd_scores_rows_kernel<WW>, p, 1, st));
  if (rc != MAGAT_OK) return rc;
  MAGAT_WIDTH_SWITCH(G, rc = launch_rows<WW>(bwd_scores_cols_kernel<WW>, p, 1, st));
  return rc;
}

extern "C" int magat_gat_train_backward_cos_f32(const float* dYpre, const float* Xhat, const float* Z, const float* att,
                                                const float* T, const float* norms, const int* rowptr, const int* colidx,
                                                const int* cscptr, const int* cscsrc, const int* cscpos, long long nnz,
                                                float* dZ, float* dXd, float* datt, int B, int N, int G, int K, void* stream) {
  if (!dYpre || !Xhat || !Z || !att || !norms || !rowptr || !cscptr || !cscsrc || !cscpos || !dZ || !dXd || !datt)
    return MAGAT_ERR_NULL;
  if (nnz > 0 && !colidx) return MAGAT_ERR_NULL;
  if (K > 2 && !T) return MAGAT_ERR_NULL;
  if (!dims_ok(B, N, nnz, K, 1)) return MAGAT_ERR_BAD_SHAPE;
  if (!supported_width(G) || N > magat_csr::kCsrMaxN) return MAGAT_ERR_UNSUPPORTED;      // (N: the limit of the forward that made the CSC view)
  const long long M = (long long)B * N;
  if (M > kGridMax || (K > 1 && rows_grid(B, N, 1) > kGridMax)) return MAGAT_ERR_BAD_SHAPE;
  int rc = magat_gat_train_backward_f32(dYpre, Xhat, Z, att, T, rowptr, colidx, cscptr, cscsrc, cscpos, nnz, dZ, dXd, datt, B, N,
                                        G, G, K, 1, MAGAT_MODE_KEYQUERY, stream);
  if (rc != MAGAT_OK || K == 1) return rc;      // (K = 1: no scores - dXd and the score columns of dZ are zero, and stay so)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const PackLayout L = pack_layout(G, G, K, 1, MAGAT_MODE_KEYQUERY);
  const int rpb = 256 / (G / 4);
  long long blocks = (M + rpb - 1) / rpb;
  if (blocks > 2048) blocks = 2048;      // (memory-bound: the workgroups stride over the rest)
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_PREPARE, st);
  MAGAT_WIDTH_SWITCH(G, hipLaunchKernelGGL((gat_cos_backward_kernel<WW>), dim3((unsigned)blocks), dim3(256), 0, st, Xhat, Z, norms,
                                           dXd, dZ, M, L.NC, L.qoff));
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_gnn_backward_csr_f32(const float* dY, const int* rowptr, const int* colidx, const float* vals,
                                          long long nnz, float* dZ, int B, int N, int F, int K, void* stream) {
  if (!dY || !rowptr || !dZ) return MAGAT_ERR_NULL;
  if (nnz > 0 && K > 1 && (!colidx || !vals)) return MAGAT_ERR_NULL;
  if (!dims_ok(B, N, nnz, K, 1)) return MAGAT_ERR_BAD_SHAPE;
  if (!supported_width(F)) return MAGAT_ERR_UNSUPPORTED;
  const long long grid = rows_grid(B, N, 1);
  if (K > 1 && grid > kGridMax) return MAGAT_ERR_BAD_SHAPE;      // (before the seed launch)
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long M = (long long)B * N;
  long long blocks = (M * (F / 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gnn_bwd_seed_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dY, dZ, M, F, K);
  int rc = magat_check_launch();
  for (int k = 1; k < K && rc == MAGAT_OK; ++k) {
    MAGAT_WIDTH_SWITCH(F, hipLaunchKernelGGL(gnn_bwd_hop_kernel<WW>, dim3((unsigned)grid), dim3(256), 0, st, rowptr, colidx,
                                             vals, dZ, B, N, K, k));
    rc = magat_check_launch();
  }
  return rc;
}
