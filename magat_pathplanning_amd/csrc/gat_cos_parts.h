// Backward of GAT_Similarity's normalisation (training; magat_gat_train_backward_cos_f32 in gat_train.hip).  The forward
// (gat_cos_prepare_kernel, gat_f32.hip) made  v^ = v / c,  c = max(n, 1e-9f),  n = |v|  for v = x_m and v = q_m and kept the two
// unclamped norms; the KeyQuery backward kernels then hand over dv^ (dXd, the score columns of dZ).  Per row and operand
//     dv = (1 / c) (dv^ - (dv^ . v^) u),   u = v^ (c / n) if n > 0, else 0
// - for n >= 1e-9 the ordinary projection (u = v^); for a clamped row u is still the true unit vector, which is what torch's
// cosine_similarity differentiates to; for a zero row dv = dv^ 1e9.
// Plain C++ with the layout of gat_cos_prepare_kernel - G / 4 lanes per row, 16 bytes per lane, sums over __shfl_xor inside the
// row's lanes - so that a host build (tools/host_wave/gat_cos_check.cpp, one thread per lane) compiles the same text.  The loop
// is wave-uniform (a whole wave leaves it together, rows past M are masked): every shuffle is met by all 64 lanes.
#pragma once

struct __attribute__((aligned(16))) cos_f4 {
  float v[4];
};

template <int LPR>
__device__ __forceinline__ float cos_row_sum(float s) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// one lane's 4-float piece of a row: d = dv^ in, dv out; h = v^; n = the unclamped norm of the row
template <int LPR>
__device__ __forceinline__ void cos_norm_bwd_piece(cos_f4& d, const cos_f4& h, float n) {
  const float dot = cos_row_sum<LPR>(fmaf(d.v[3], h.v[3], fmaf(d.v[2], h.v[2], fmaf(d.v[1], h.v[1], d.v[0] * h.v[0]))));
  const float c = fmaxf(n, 1e-9f), ic = 1.f / c;
  const float s = n > 0.f ? c / n : 0.f;      // u = v^ s
#pragma unroll
  for (int e = 0; e < 4; ++e) d.v[e] = ic * (d.v[e] - dot * (h.v[e] * s));
}

// Xhat [M][G], Z [M][NC] (q^ in its G columns at qoff), norms [2][M] (|x|, |q|); dXd [M][G] and the G columns of dZ [M][NC] at
// qoff are rewritten in place.  256 threads; a grid-stride loop over rows.
template <int G>
__global__ __launch_bounds__(256) void gat_cos_backward_kernel(const float* __restrict__ Xhat, const float* __restrict__ Z,
                                                               const float* __restrict__ norms, float* __restrict__ dXd,
                                                               float* __restrict__ dZ, long long M, int NC, int qoff) {
  constexpr int LPR = G / 4;          // lanes per row: 4 .. 64, a row never straddles two waves
  constexpr int RPW = 64 / LPR;       // rows per wave
  constexpr int RPB = 4 * RPW;        // rows per workgroup step
  static_assert(LPR >= 4 && LPR <= 64 && (LPR & (LPR - 1)) == 0, "G in {16, 32, 64, 128, 256}");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % LPR;
  for (long long base = blockIdx.x * (long long)RPB + wave * RPW; base < M; base += (long long)gridDim.x * RPB) {
    const long long m = base + lane / LPR;
    const bool ok = m < M;
    cos_f4 dx = {{0.f, 0.f, 0.f, 0.f}}, hx = dx, dq = dx, hq = dx;
    float nx = 0.f, nq = 0.f;
    if (ok) {
      dx = *reinterpret_cast<const cos_f4*>(dXd + m * G + 4 * sub);
      hx = *reinterpret_cast<const cos_f4*>(Xhat + m * G + 4 * sub);
      dq = *reinterpret_cast<const cos_f4*>(dZ + m * NC + qoff + 4 * sub);
      hq = *reinterpret_cast<const cos_f4*>(Z + m * NC + qoff + 4 * sub);
      nx = norms[m];
      nq = norms[M + m];
    }
    cos_norm_bwd_piece<LPR>(dx, hx, nx);
    cos_norm_bwd_piece<LPR>(dq, hq, nq);
    if (ok) {
      *reinterpret_cast<cos_f4*>(dXd + m * G + 4 * sub) = dx;
      *reinterpret_cast<cos_f4*>(dZ + m * NC + qoff + 4 * sub) = dq;
    }
  }
}
