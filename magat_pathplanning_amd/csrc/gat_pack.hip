// Weight packing of the graph layers: Bt [NC][G] + column bias [NC] and the planes / fragment streams behind them (layout: gat_pack.h).
#include "magat_common.h"
#include "gat_pack.h"

namespace {

__global__ void pack_kernel(const float* __restrict__ weight, const float* __restrict__ wbias,
                            const float* __restrict__ mixer, const float* __restrict__ taps,
                            float* __restrict__ packed, int G, int F, int K, int P, int mode, PackLayout L) {
  float* Bt = packed;
  float* cb = packed + (long long)L.NC * G;
  // bf16x3 planes of Bt for the split-MFMA GEMM (raw bf16 bits), 16-byte aligned behind the column bias
  unsigned short* Bs = reinterpret_cast<unsigned short*>(packed + (((long long)L.NC * (G + 1) + 3) & ~3LL));
  unsigned short* Hs = reinterpret_cast<unsigned short*>(packed + magat_gat_f16_block_offset(L.NC, G));
  // the same two planes once more in MFMA-fragment order for gat_mfma.hip (G = 128): 128-row blocks of Bt, per block
  // [32-row tile 4][k step 8][plane 2][lane 64][8 halfs], lane = row % 32 + 32 * (k % 16 / 8)
  // (KeyQuery only: the rank-1 modes' stream at the same offset is written by pack_frag_rank1_kernel, with its own size)
  unsigned short* Fs = (G == 128 && (L.NC & 127) == 0 && (mode == MAGAT_MODE_KEYQUERY || mode == MAGAT_MODE_SIMILARITY))
                           ? reinterpret_cast<unsigned short*>(packed + magat_gat_frag_offset(L.NC, G)) : nullptr;
  const long long total = (long long)L.NC * G;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total + L.NC;
       idx += (long long)gridDim.x * blockDim.x) {
    if (idx >= total) {  // column bias
      const int col = (int)(idx - total);
      float v = 0.f;
      if (mode == MAGAT_MODE_GAT_MODIFIED && col >= L.c1off && col < L.c2off + P) {   // GAT_origin has no weight_bias
        const int which = col >= L.c2off, hp = which ? col - L.c2off : col - L.c1off;
        for (int f = 0; f < F; ++f) v = fmaf(mixer[(long long)hp * 2 * F + which * F + f], wbias[hp * F + f], v);
      }
      cb[col] = v;
      continue;
    }
    const int col = (int)(idx / G), g = (int)(idx % G);
    float v = 0.f;
    if ((mode == MAGAT_MODE_KEYQUERY || mode == MAGAT_MODE_SIMILARITY) && col < L.uoff) {
      v = weight[(long long)col * G + g];  // (P,1,G,G): row p*G+g' = W_p[g',:]
    } else if (col >= L.uoff && col < L.uoff + P * K * F) {
      const int r = col - L.uoff, hp = r / (K * F), k = (r / F) % K, f = r % F;
      if (mode == MAGAT_MODE_GAT_ORIGIN)
        // scalar taps (E=1,K) x W: the reference reshapes permute(0,3,1,2)(W) = (P,G,E,F) straight into (P,F,E,1,G)
        // (graphML.py:1967-1969), so with F == G the filter is W TRANSPOSED: h[p,f,k,g] = h_k * W[p,0,g,f]
        v = taps[k] * weight[((long long)hp * F + g) * G + f];
      else
        v = taps[(((long long)hp * F + f) * K + k) * G + g];  // (P,F,1,K,G)
    } else if (mode != MAGAT_MODE_KEYQUERY && mode != MAGAT_MODE_GNN && mode != MAGAT_MODE_SIMILARITY && col >= L.c1off &&
               col < L.c2off + P) {
      const int which = col >= L.c2off, hp = which ? col - L.c2off : col - L.c1off;
      for (int f = 0; f < F; ++f)
        v = fmaf(mixer[(long long)hp * 2 * F + which * F + f], weight[((long long)hp * F + f) * G + g], v);
    }
    Bt[idx] = v;
    const unsigned short h1 = magat_bf16_rne(v);
    const float r1 = v - magat_bf16_f32(h1);
    const unsigned short h2 = magat_bf16_rne(r1);
    Bs[idx] = h1;
    Bs[total + idx] = h2;
    Bs[2 * total + idx] = magat_bf16_rne(r1 - magat_bf16_f32(h2));
    // f16x2 planes of v * 2^8 (fixed scale: |v| up to 255 representable, residual plane normal down to |v| ~ 5e-4,
    // absolute error floor 1e-10 below that) followed by the inverse scale: the "f16x3" operand of the maps GEMM
    const float vs = v * 256.f;
    const _Float16 g1 = (_Float16)vs;
    const _Float16 g2 = (_Float16)(vs - (float)g1);
    Hs[idx] = __builtin_bit_cast(unsigned short, g1);
    Hs[total + idx] = __builtin_bit_cast(unsigned short, g2);
    if (Fs) {
      const int r = col & 127;
      const long long fo = (long long)(col >> 7) * 32768 + (((r >> 5) * 8 + (g >> 4)) * 2) * 512 +
                           ((r & 31) + 32 * ((g & 15) >> 3)) * 8 + (g & 7);
      Fs[fo] = __builtin_bit_cast(unsigned short, g1);
      Fs[fo + 512] = __builtin_bit_cast(unsigned short, g2);
    }
    if (idx == 0) *reinterpret_cast<float*>(Hs + 2 * total) = 1.f / 256.f;
  }
}

// GAT_modified / GAT_origin at G = F = 128: the weight stream of the one-launch kernel (gat_mfma.hip MODE 1) in the SAME shape
// as KeyQuery's - P blocks of 128 x 128 for G1, then P K tap blocks - as fragment-major f16 planes of 2^8 v.  The G1 block of
// head p holds the two score vectors a1 W_p (row 0) and a2 W_p (row 1), zeros elsewhere; kconst[p] = a1 . wb + a2 . wb.
__global__ void pack_frag_rank1_kernel(const float* __restrict__ weight, const float* __restrict__ wbias,
                                       const float* __restrict__ mixer, const float* __restrict__ taps,
                                       unsigned short* __restrict__ Fs, float* __restrict__ kconst, int K, int P, int mode) {
  constexpr int G = 128, F = 128;
  const long long total = (long long)(P * G + P * K * F) * G;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total + P;
       idx += (long long)gridDim.x * blockDim.x) {
    if (idx >= total) {
      const int hp = (int)(idx - total);
      float v = 0.f;
      if (mode == MAGAT_MODE_GAT_MODIFIED && wbias)
        for (int f = 0; f < F; ++f)
          v = fmaf(mixer[(long long)hp * 2 * F + f] + mixer[(long long)hp * 2 * F + F + f], wbias[hp * F + f], v);
      kconst[hp] = v;
      continue;
    }
    const int col = (int)(idx / G), g = (int)(idx % G);
    float v = 0.f;
    if (col < P * G) {
      const int hp = col / G, r = col % G;
      if (r < 2)
        for (int f = 0; f < F; ++f)
          v = fmaf(mixer[(long long)hp * 2 * F + r * F + f], weight[((long long)hp * F + f) * G + g], v);
    } else {
      const int r = col - P * G, hp = r / (K * F), k = (r / F) % K, f = r % F;
      v = mode == MAGAT_MODE_GAT_ORIGIN ? taps[k] * weight[((long long)hp * F + g) * G + f]
                                        : taps[(((long long)hp * F + f) * K + k) * G + g];
    }
    const float vs = v * 256.f;
    const _Float16 g1 = (_Float16)vs;
    const _Float16 g2 = (_Float16)(vs - (float)g1);
    const int rr = col & 127;
    const long long fo = (long long)(col >> 7) * 32768 + (((rr >> 5) * 8 + (g >> 4)) * 2) * 512 +
                         ((rr & 31) + 32 * ((g & 15) >> 3)) * 8 + (g & 7);
    Fs[fo] = __builtin_bit_cast(unsigned short, g1);
    Fs[fo + 512] = __builtin_bit_cast(unsigned short, g2);
  }
}

static bool gat_rank1_frag(int G, int F, int mode) {
  return G == 128 && F == 128 && (mode == MAGAT_MODE_GAT_MODIFIED || mode == MAGAT_MODE_GAT_ORIGIN);
}

}  // namespace

extern "C" size_t magat_gat_packed_floats(int G, int F, int K, int P, int mode) {
  if (G <= 0 || F <= 0 || K <= 0 || P <= 0) return 0;
  const PackLayout L = pack_layout(G, F, K, P, mode);
  if (gat_rank1_frag(G, F, mode))      // + the one-launch kernel's weight stream and the per-head score constants
    return magat_gat_frag_offset(L.NC, G) + (size_t)(P * G + P * K * F) * G + (((size_t)P + 3) & ~(size_t)3);
  if (G == 128 && (L.NC & 127) == 0 && (mode == MAGAT_MODE_KEYQUERY || mode == MAGAT_MODE_SIMILARITY))      // + the bf16 fragments of gat_csr_fused.hip (NC * G bf16)
    return magat_gat_csr_fused_offset(L.NC, G) + (size_t)L.NC * G / 2 + 4;
  return magat_gat_f16_block_offset(L.NC, G) + (size_t)L.NC * G + 4;
}

extern "C" int magat_gat_pack_weights(const float* weight, const float* weight_bias, const float* mixer,
                                      const float* taps, float* packed, int G, int F, int K, int P, int mode,
                                      void* stream) {
  if ((!weight && mode != MAGAT_MODE_GNN) || !taps || !packed) return MAGAT_ERR_NULL;
  if (mode == MAGAT_MODE_GAT_MODIFIED && (!weight_bias || !mixer)) return MAGAT_ERR_NULL;
  if (mode == MAGAT_MODE_GAT_ORIGIN && !mixer) return MAGAT_ERR_NULL;
  if (G <= 0 || F <= 0 || K <= 0 || P <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (mode < MAGAT_MODE_KEYQUERY || mode > MAGAT_MODE_SIMILARITY) return MAGAT_ERR_UNSUPPORTED;
  if (mode == MAGAT_MODE_SIMILARITY && (P != 1 || G != F)) return MAGAT_ERR_UNSUPPORTED;
  const PackLayout L = pack_layout(G, F, K, P, mode);
  const long long total = (long long)L.NC * (G + 1);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pack_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), weight, weight_bias,
                     mixer, taps, packed, G, F, K, P, mode, L);
  if (G == 128 && F == 128 && K == 2 && mode == MAGAT_MODE_KEYQUERY && (P == 1 || P == 2 || P == 4)) {
    const int rc = magat_gat_csr_fused_pack(packed, packed + magat_gat_csr_fused_offset(L.NC, G), P, static_cast<hipStream_t>(stream));
    if (rc != MAGAT_OK) return rc;
  }
  if (gat_rank1_frag(G, F, mode)) {
    float* frag = packed + magat_gat_frag_offset(L.NC, G);
    hipLaunchKernelGGL(pack_frag_rank1_kernel, dim3(2048), dim3(256), 0, static_cast<hipStream_t>(stream), weight, weight_bias,
                       mixer, taps, reinterpret_cast<unsigned short*>(frag), frag + (size_t)(P * G + P * K * F) * G, K, P, mode);
  }
  return magat_check_launch();
}
