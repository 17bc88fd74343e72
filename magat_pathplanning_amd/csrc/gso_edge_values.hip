// The GSO's VALUES on the edge structure of gso_edges.hip: lambda_max per instance and one float32 per CSR entry, so that the layers
// which multiply by the GSO (GraphFilterBatch: W / lambda_max(W), or D^-1/2 W D^-1/2 / lambda_max) follow the edge route too - no
// (B,N,N) tensor, no pair test per Lanczos step, N <= 4096.
//
// One launch, one workgroup per instance, no host synchronisation, plain stores, the same result on every call.  The rule is the
// workgroup form of gso_kernel (sim_frontend.hip), step for step, with the rows of W read as colidx slices instead of bit rows or
// distance tests: Lanczos on inv o W o inv from the normalised all-ones vector without re-orthogonalisation; the largest eigenvalue
// of T_steps located by the 256-probe multisection on the pivot form of the Sturm count every 8 steps up to 160, then every 32, then
// every eighth of the largest power of two below the step count; stop at the second location in a row that moved by at most 1e-13
// relative, at breakdown, or after N steps.  256 threads, rows i = t + 256 q, neighbours in ascending column order, the same
// fixed-order block sums: tests/gso_lanczos_restatement.py describes this kernel as it describes that one.
//
// LDS: v, v_prev and inv as float64 [N] (96 KB at 4096 agents); w is written over v_prev's slot, a thread's own rows.  The
// tridiagonal matrix (alpha [cap], beta [cap + 2], cap = max(N, 160)) stands behind them while both fit the 160 KB of a workgroup
// beside the kernel's static 144 bytes (the reduction slots and the waves' probe answers): 40 N + 16 + 144 <= 163840, N <= 4092 -
// and in the caller's workspace otherwise (4093 .. 4096 agents); the workgroup's own stores to it are ordered by __syncthreads() like the LDS
// ones.  An instance's colidx slice is read from memory at every step (4 bytes an edge: it stays in L2).
#include "magat_common.h"

namespace {
constexpr int GEV_N_MAX = 4096;       // the edge structure's limit (gso_edges.hip)
constexpr int GEV_THREADS = 256;      // four waves, as gso_kernel
constexpr int GEV_LMIN = 160;         // gso_kernel's GSO_LMIN: locations every 8 steps up to here
constexpr size_t GEV_STATIC_LDS = 16 * sizeof(double) + (GEV_THREADS / 64) * sizeof(int);      // red [16], wbest [4] of the kernel
#ifdef MAGAT_HOST_WAVE
size_t gev_lds_limit = 128 * 1024;    // the stand-in's dynamic LDS; tools/host_wave/gso_edge_values_check.cpp lowers it to reach the workspace form
#else
constexpr size_t gev_lds_limit = 160 * 1024;      // LDS of a workgroup, static and dynamic together
#endif

__host__ __device__ inline int gev_cap(int N) { return N > GEV_LMIN ? N : GEV_LMIN; }
inline size_t gev_tri_bytes(int N) { return (2 * (size_t)gev_cap(N) + 2) * sizeof(double); }
inline size_t gev_vec_bytes(int N) { return 3 * (size_t)N * sizeof(double); }

// (a double through two 32-bit shuffles: what __shfl_xor does with a double)
__device__ __forceinline__ double gev_shfl_xor(double v, int o) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)u, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(u >> 32), o, 64);
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}
// block_sum of sim_frontend.hip: the butterfly inside a wave, then the waves' partials in their order
__device__ __forceinline__ double gev_block_sum(double v, double* red, int t) {
  for (int o = 32; o > 0; o >>= 1) v += gev_shfl_xor(v, o);
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < GEV_THREADS / 64; ++w) s += red[w];
  return s;
}

template <bool TRI_LDS>
__global__ __launch_bounds__(GEV_THREADS) void gso_edge_values_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                                      long long cap, int symmetric_norm, int normalize,
                                                                      double* __restrict__ lambda_out, float* __restrict__ vals,
                                                                      double* tri_ws, int N) {
  HIP_DYNAMIC_SHARED(unsigned long long, lds)
  __shared__ double red[16];
  __shared__ int wbest[GEV_THREADS / 64];
  static_assert(sizeof(red) + sizeof(wbest) == GEV_STATIC_LDS, "the LDS plan of magat_gso_edge_values counts these");
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int* rp = rowptr + (size_t)b * (N + 1);      // absolute offsets
  const long long first = rp[0], end = rp[N];
  // capacity contract: colidx holds the entries below cap only (rowptr stays true).  An instance that reaches beyond is not walked -
  // the structure is re-built with a larger capacity (EdgeStructure.ready) and the values are launched again behind it
  if (end > cap) {
    if (t == 0) lambda_out[b] = 0.0;
    return;
  }
  double* v = reinterpret_cast<double*>(lds);
  double* vprev = v + N;
  double* inv = vprev + N;
  const int lcap = gev_cap(N);
  double* alpha = TRI_LDS ? inv + N : tri_ws + (size_t)b * (2 * (size_t)lcap + 2);      // [lcap]
  double* beta = alpha + lcap;                                                          // [lcap + 2]  beta[k] couples v_{k-1} and v_k
  for (int i = t; i < N; i += GEV_THREADS) {
    const int deg = rp[i + 1] - rp[i];
    double s = 1.0;
    if (symmetric_norm) s = deg > 0 ? sqrt(1.0 / (double)deg) : 0.0;      // isolated agents -> 0, as gso_kernel
    inv[i] = s;
  }
  __syncthreads();
  const bool has_edges = end > first;
  double lam = 0.0;
  if (has_edges && normalize) {
    const double s0 = 1.0 / sqrt((double)N);
    for (int i = t; i < N; i += GEV_THREADS) {
      v[i] = s0;
      vprev[i] = 0.0;
    }
    if (t == 0) beta[0] = 0.0;
    __syncthreads();
    double prev = -1.0, bk = 0.0;      // bk = beta[k]
    int stable = 0;
    for (int k = 0; k < lcap; ++k) {
      // w_i = inv_i (W (inv o v))_i - beta_k vprev_i, written over vprev_i (no other thread reads that slot); alpha = v . w
      double dot = 0.0;
      for (int i = t; i < N; i += GEV_THREADS) {
        double acc = 0.0;
        const int e1 = rp[i + 1];
        for (int e = rp[i]; e < e1; ++e) {
          const int j = colidx[e];
          acc += inv[j] * v[j];
        }
        const double wi = inv[i] * acc - bk * vprev[i];
        vprev[i] = wi;
        dot += v[i] * wi;
      }
      const double ak = gev_block_sum(dot, red, t);
      double nrm = 0.0;
      for (int i = t; i < N; i += GEV_THREADS) {
        const double wi = vprev[i] - ak * v[i];
        vprev[i] = wi;
        nrm += wi * wi;
      }
      const double bn = sqrt(gev_block_sum(nrm, red, t));
      if (t == 0) {
        alpha[k] = ak;
        beta[k + 1] = bn;
      }
      const int steps = k + 1;
      const bool breakdown = !(bn > 1e-13 * (fabs(ak) + bk + 1.0));      // invariant subspace reached: T_steps is exact
      // hand-over (every read of v by the product lies in front of the block sums' barriers)
      for (int i = t; i < N; i += GEV_THREADS) {
        const double wi = vprev[i];
        vprev[i] = v[i];
        if (!breakdown) v[i] = wi / bn;
      }
      __syncthreads();      // v, alpha and beta are written
      int chk = 8;
      if (steps > GEV_LMIN) {
        chk = (1 << (31 - __builtin_clz((unsigned)steps))) >> 3;
        if (chk < 32) chk = 32;
      }
      if (breakdown || (steps % chk) == 0 || steps == lcap || steps >= N) {
        // largest eigenvalue of T_steps by multisection on the Sturm count from the Gershgorin interval: every thread probes its
        // own abscissa, the interval shrinks 257-fold per pass
        double lo = alpha[0], hi = alpha[0];
        for (int r = 0; r < steps; ++r) {
          const double off = (r > 0 ? fabs(beta[r]) : 0.0) + (r + 1 < steps ? fabs(beta[r + 1]) : 0.0);
          lo = fmin(lo, alpha[r] - off);
          hi = fmax(hi, alpha[r] + off);
        }
        for (int pass = 0; pass < 12 && hi - lo > 4e-16 * fmax(fabs(lo), fabs(hi)); ++pass) {
          const double x = lo + (hi - lo) * (double)(t + 1) / (double)(GEV_THREADS + 1);
          int below = 0;      // eigenvalues of T below x = negative pivots of T - x I
          double d = 1.0;
          for (int r = 0; r < steps; ++r) {
            d = (alpha[r] - x) - (r > 0 ? beta[r] * beta[r] / d : 0.0);
            if (d == 0.0) d = 1e-300;
            if (d < 0.0) ++below;
          }
          // the last thread with lambda_max >= x_t: a ballot per wave, the waves' answers through LDS
          const unsigned long long ge = __ballot(below < steps);
          if (lane == 0) wbest[wave] = ge ? wave * 64 + 63 - (int)__clzll(ge) : -1;
          __syncthreads();
          int bt = wbest[0];
          for (int w = 1; w < GEV_THREADS / 64; ++w) bt = wbest[w] > bt ? wbest[w] : bt;
          __syncthreads();      // (the next pass writes wbest again)
          const double nlo = bt >= 0 ? lo + (hi - lo) * (double)(bt + 1) / (double)(GEV_THREADS + 1) : lo;
          const double nhi = bt + 1 < GEV_THREADS ? lo + (hi - lo) * (double)(bt + 2) / (double)(GEV_THREADS + 1) : hi;
          lo = nlo;
          hi = nhi;
        }
        lam = 0.5 * (lo + hi);
        if (breakdown || steps >= N) break;
        if (fabs(lam - prev) <= 1e-13 * fabs(lam)) {
          if (++stable >= 2) break;
        } else {
          stable = 0;
        }
        prev = lam;
      }
      bk = bn;
    }
  }
  if (t == 0) lambda_out[b] = lam;
  if (!has_edges) return;
  // gso_kernel's expressions in float64, rounded once
  const double div = normalize ? lam : 1.0;
  const double plain = 1.0 / div;
  for (int i = t; i < N; i += GEV_THREADS) {
    const int e1 = rp[i + 1];
    for (int e = rp[i]; e < e1; ++e) vals[e] = symmetric_norm ? (float)((inv[i] * 1.0 * inv[colidx[e]]) / div) : (float)plain;
  }
}

}  // namespace

extern "C" size_t magat_gso_edge_values_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0 || N > GEV_N_MAX) return 0;
  return magat_align_up((size_t)B * gev_tri_bytes(N), 256);
}

extern "C" int magat_gso_edge_values(const int* rowptr, const int* colidx, const long long* nnz_dev, long long cap, int symmetric_norm,
                                     int normalize, double* lambda_out, float* vals, void* workspace, size_t workspace_bytes, int B,
                                     int N, void* stream) {
  if (!rowptr || !nnz_dev || !lambda_out) return MAGAT_ERR_NULL;
  if ((!colidx || !vals) && cap != 0) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || cap < 0) return MAGAT_ERR_BAD_SHAPE;
  const size_t need = magat_gso_edge_values_workspace_bytes(B, N);
  if (!need) return MAGAT_ERR_UNSUPPORTED;                      // N > 4096
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) || workspace_bytes < need) return MAGAT_ERR_WORKSPACE;
  // static and dynamic LDS together fit a workgroup's: 4093 .. 4096 agents keep the tridiagonal matrix in the workspace
  const bool tri_lds = GEV_STATIC_LDS + gev_vec_bytes(N) + gev_tri_bytes(N) <= gev_lds_limit;
  const size_t lds = gev_vec_bytes(N) + (tri_lds ? gev_tri_bytes(N) : 0);
  if (GEV_STATIC_LDS + lds > gev_lds_limit) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds > 64 * 1024 &&
      magat_ensure_dyn_lds(tri_lds ? reinterpret_cast<const void*>(&gso_edge_values_kernel<true>)
                                   : reinterpret_cast<const void*>(&gso_edge_values_kernel<false>),
                           tri_lds ? MAGAT_LDS_GSO_VALUES : MAGAT_LDS_GSO_VALUES_WS, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  double* tri = static_cast<double*>(workspace);
  magat_form_note(MAGAT_FORM_GSO_EDGES);
  const int pid = magat_prof_begin(MAGAT_TAG_GSO_EDGES, st);
  if (tri_lds) {
    hipLaunchKernelGGL(gso_edge_values_kernel<true>, dim3((unsigned)B), dim3(GEV_THREADS), lds, st, rowptr, colidx, cap,
                       symmetric_norm, normalize, lambda_out, vals, tri, N);
  } else {
    hipLaunchKernelGGL(gso_edge_values_kernel<false>, dim3((unsigned)B), dim3(GEV_THREADS), lds, st, rowptr, colidx, cap,
                       symmetric_norm, normalize, lambda_out, vals, tri, N);
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}
