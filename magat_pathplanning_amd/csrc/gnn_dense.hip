// GraphFilterBatch / BatchLSIGF (graphML.py:5485-5579, 5670-5689) on a dense GSO in ONE launch: the graph layer of the
// bottleneck GNN planners (DecentralPlannerBottleneckNet) for graphs of at most 128 nodes.
//
//   Y[b,n,f] = act(bias[f] + sum_k sum_g (x S^k)[g,n] h[f,0,k,g]),   S read as float(S) (graphML.py:5562)
//
// Form: Horner on F-wide rows,  acc = U_{K-1};  acc = S^T acc + U_k  (k = K-2 .. 0),  U_k = X H_k^T.  Output columns are
// independent through every hop, so a workgroup owns one instance and one FS-wide column slice of F: it holds that
// instance's float(S) (<= 64 KB), its X rows and the slice's hop state in LDS and writes nothing but its block of Y.  A
// thread owns one column and 4 consecutive rows (THREADS = FS x the row groups N needs: 1 | 2 | 4 waves per SIMD); every product is a true float32 FMA (k-ordered chains, no split
// arithmetic: the layer has no range guard and needs none).  Every entry of S is multiplied in, zeros included, so a NaN
// entry spreads exactly as it does through the reference's dense matmul.
#include "magat_common.h"

namespace {

struct GnnDenseParams {
  const float* X;       // [B*Nin][ldx]
  const void* S;        // [B][N][N] float32 | float64
  const float* W;       // raw taps (F,1,K,G)
  const float* bias;    // [F] or null
  float* Y;             // [B*Nin][ldy]
  int ldx, ldy, B, N, Nin, G, F, K, s64, relu;
};

template <int FS, int THREADS>
__global__ __launch_bounds__(THREADS) void gnn_dense_kernel(GnnDenseParams p) {
  constexpr int RPT = 4;              // rows per thread
  constexpr int RG = THREADS / FS;    // row groups
  constexpr int NP = RG * RPT;        // padded node count (>= N)
  extern __shared__ float lds[];
  const int N = p.N, G = p.G, K = p.K;
  const int slices = p.F / FS;
  const int b = blockIdx.x / slices;
  const int f0 = (blockIdx.x - b * slices) * FS;
  float* Sl = lds;                    // [N][NP]  float(S), columns >= N zero
  float* Xl = Sl + N * NP;            // [NP][G]  X rows, rows >= Nin zero (the reference's zero padding)
  float* Al = Xl + NP * G;            // [NP][FS] hop state of the slice

  const long long sb = (long long)b * N * N;
  if (p.s64) {
    const double* S = static_cast<const double*>(p.S) + sb;
    for (int i = threadIdx.x; i < N * N; i += THREADS) {
      const int m = i / N, n = i - m * N;
      Sl[m * NP + n] = (float)S[i];          // round to nearest even, as .float()
    }
  } else {
    const float* S = static_cast<const float*>(p.S) + sb;
    for (int i = threadIdx.x; i < N * N; i += THREADS) {
      const int m = i / N, n = i - m * N;
      Sl[m * NP + n] = S[i];
    }
  }
  if (NP > N)
    for (int i = threadIdx.x; i < N * (NP - N); i += THREADS) {
      const int m = i / (NP - N);
      Sl[m * NP + N + (i - m * (NP - N))] = 0.f;
    }
  const float* Xb = p.X + (long long)b * p.Nin * p.ldx;
  for (int i = threadIdx.x; i < NP * G; i += THREADS) {
    const int n = i / G, g = i - n * G;
    Xl[i] = n < p.Nin ? Xb[(long long)n * p.ldx + g] : 0.f;
  }
  __syncthreads();

  const int f = threadIdx.x % FS;
  const int r0 = (threadIdx.x / FS) * RPT;
  const float* Wf = p.W + (long long)(f0 + f) * K * G;
  float acc[RPT];
#pragma unroll
  for (int j = 0; j < RPT; ++j) acc[j] = 0.f;

  // acc += X H_k^T for this thread's rows and column
  auto map = [&](int k) {
    const float* h = Wf + k * G;
#pragma unroll 4
    for (int g = 0; g < G; g += 4) {
      const float h0 = h[g], h1 = h[g + 1], h2 = h[g + 2], h3 = h[g + 3];
#pragma unroll
      for (int j = 0; j < RPT; ++j) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(Xl + (r0 + j) * G + g);
        float a = acc[j];
        a = __builtin_fmaf(x.x, h0, a);
        a = __builtin_fmaf(x.y, h1, a);
        a = __builtin_fmaf(x.z, h2, a);
        acc[j] = __builtin_fmaf(x.w, h3, a);
      }
    }
  };

  map(K - 1);
  for (int k = K - 2; k >= 0; --k) {
    __syncthreads();                  // the previous hop has read Al
#pragma unroll
    for (int j = 0; j < RPT; ++j) Al[(r0 + j) * FS + f] = acc[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPT; ++j) acc[j] = 0.f;
    // acc = S^T acc_prev  (row n of "x @ S": sum over m of S[m,n] * acc_prev[m])
#pragma unroll 4
    for (int m = 0; m < N; ++m) {
      const float a = Al[m * FS + f];
#pragma unroll
      for (int j4 = 0; j4 < RPT / 4; ++j4) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(Sl + m * NP + r0 + 4 * j4);
        acc[4 * j4 + 0] = __builtin_fmaf(s.x, a, acc[4 * j4 + 0]);
        acc[4 * j4 + 1] = __builtin_fmaf(s.y, a, acc[4 * j4 + 1]);
        acc[4 * j4 + 2] = __builtin_fmaf(s.z, a, acc[4 * j4 + 2]);
        acc[4 * j4 + 3] = __builtin_fmaf(s.w, a, acc[4 * j4 + 3]);
      }
    }
    map(k);
  }

  const float bv = p.bias ? p.bias[f0 + f] : 0.f;
  float* Yb = p.Y + (long long)b * p.Nin * p.ldy + f0 + f;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int n = r0 + j;
    if (n < p.Nin) {
      float v = p.bias ? acc[j] + bv : acc[j];
      if (p.relu) v = magat_relu(v);      // (v < 0 ? 0 : v: a NaN stays NaN, as torch.relu)
      Yb[(long long)n * p.ldy] = v;
    }
  }
}

template <int FS, int THREADS>
int launch_gnn_dense(const GnnDenseParams& p, int slot, hipStream_t st) {
  constexpr int NP = (THREADS / FS) * 4;
  const size_t lds = sizeof(float) * ((size_t)p.N * NP + (size_t)NP * p.G + (size_t)NP * FS);
  const void* fn = reinterpret_cast<const void*>(&gnn_dense_kernel<FS, THREADS>);
  if (magat_ensure_dyn_lds(fn, slot, lds) != MAGAT_OK) return MAGAT_ERR_LAUNCH;
  const long long blocks = (long long)p.B * (p.F / FS);
  magat_form_note(MAGAT_FORM_GNN_DENSE);
  const int pid = magat_prof_begin(MAGAT_TAG_GNN_DENSE, st);
  hipLaunchKernelGGL((gnn_dense_kernel<FS, THREADS>), dim3((unsigned)blocks), dim3(THREADS), lds, st, p);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

}  // namespace

extern "C" int magat_gnn_dense_supported(int N, int G, int F, int K) {
  const bool width_ok = (G == 16 || G == 32 || G == 64 || G == 128) && (F == 16 || F == 32 || F == 64 || F == 128);
  return (N >= 1 && N <= 128 && K >= 1 && K <= 8 && width_ok) ? 1 : 0;
}

extern "C" int magat_gnn_forward_dense_f32(const float* X, int ldx, const void* S, int s_is_f64, const float* weight,
                                           const float* bias, float* Y, int ldy, int B, int N, int Nin, int G, int F, int K,
                                           int relu, void* stream) {
  if (!magat_gnn_dense_supported(N, G, F, K)) return MAGAT_ERR_UNSUPPORTED;
  if (B < 1 || Nin < 1 || Nin > N || ldx < G || ldy < F) return MAGAT_ERR_BAD_SHAPE;
  if (!X || !S || !weight || !Y) return MAGAT_ERR_NULL;
  if (ldy % 4) return MAGAT_ERR_BAD_SHAPE;                               // (the header's alignment rules of every
  if (reinterpret_cast<uintptr_t>(X) & 15) return MAGAT_ERR_UNSUPPORTED;   //  graph-layer entry point)
  if ((long long)B * (F / 16) >= (1LL << 31)) return MAGAT_ERR_UNSUPPORTED;
  GnnDenseParams p;
  p.X = X; p.S = S; p.W = weight; p.bias = bias; p.Y = Y;
  p.ldx = ldx; p.ldy = ldy; p.B = B; p.N = N; p.Nin = Nin; p.G = G; p.F = F; p.K = K;
  p.s64 = s_is_f64 ? 1 : 0; p.relu = relu ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // 4 rows per thread: as many row groups as N needs (the waves of a workgroup hide each other's LDS latency)
  if (F >= 32) {        // 32 columns per workgroup
    if (N <= 32) return launch_gnn_dense<32, 256>(p, MAGAT_LDS_GNND_0 + 0, st);
    if (N <= 64) return launch_gnn_dense<32, 512>(p, MAGAT_LDS_GNND_0 + 1, st);
    return launch_gnn_dense<32, 1024>(p, MAGAT_LDS_GNND_0 + 2, st);
  }
  // F = 16: 16 columns
  if (N <= 64) return launch_gnn_dense<16, 256>(p, MAGAT_LDS_GNND_0 + 3, st);
  return launch_gnn_dense<16, 512>(p, MAGAT_LDS_GNND_0 + 4, st);
}
