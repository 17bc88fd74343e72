// The packed weights of a graph layer (magat_gat_pack_weights, gat_pack.hip): the ONE definition of their layout, for the kernels
// that read the pack (gat_f32.hip, gat_csr_f32.hip, gat_train.hip) and the kernels that write it.  Included after magat_common.h.
#pragma once
#include "gat_route.h"

// packed GAT weights: [Bt NC*G | colbias NC | pad to 4][bf16x3 planes 3*NC*G u16 | pad to 4 floats][f16x2 planes of
// Bt * 2^8: 2*NC*G u16][float 2^-8][pad]: float offset of the f16 block
__host__ __device__ inline size_t magat_gat_f16_block_offset(int NC, int G) {
  const size_t a = (((size_t)NC * (G + 1) + 3) & ~(size_t)3) + ((size_t)3 * NC * G + 1) / 2;
  return (a + 3) & ~(size_t)3;
}

// fragment-major f16x2 planes of Bt * 2^8 in 128-row blocks (G = 128, NC % 128 == 0; gat_mfma.hip): float offset behind the
// row-major planes; NC * G more floats
__host__ __device__ inline size_t magat_gat_frag_offset(int NC, int G) {
  return (magat_gat_f16_block_offset(NC, G) + (size_t)NC * G + 4 + 3) & ~(size_t)3;
}
// bf16-storage CSR layer with the maps inside the graph kernels (gat_csr_fused.hip: KeyQuery, K = 2, G = F = 128, concat):
// the fragment-major bf16 weights sit behind the one-launch kernel's fragments in the packed block (NC * G / 2 more floats)
__host__ __device__ inline size_t magat_gat_csr_fused_offset(int NC, int G) {
  return (magat_gat_frag_offset(NC, G) + (size_t)NC * G + 3) & ~(size_t)3;
}

namespace {
// columns of Bt (= of the hoisted maps Z = X @ Bt^T + colbias): NC in all, the score maps at qoff, the filter taps at uoff, the
// two score columns per head of the rank-1 modes at c1off / c2off
struct PackLayout {
  int NC, qoff, uoff, c1off, c2off;
};
PackLayout pack_layout(int G, int F, int K, int P, int mode) {
  PackLayout L;
  if (mode == MAGAT_MODE_KEYQUERY || mode == MAGAT_MODE_SIMILARITY) {      // (GAT_Similarity: KeyQuery's layout, P = 1)
    L.qoff = 0;
    L.uoff = P * G;
    L.c1off = L.c2off = 0;
  } else if (mode == MAGAT_MODE_GNN) {     // filter taps only
    L.qoff = 0;
    L.uoff = 0;
    L.c1off = L.c2off = 0;
  } else {
    L.qoff = 0;
    L.uoff = 0;
    L.c1off = P * K * F;
    L.c2off = L.c1off + P;
  }
  L.NC = magat_gat::pack_columns(G, F, K, P, mode);      // (one definition: the dense route sizes Z by it)
  return L;
}

using magat_gat::supported_width;      // feature widths the graph kernels are instantiated for
}  // namespace

// CALL with WW = the width W as a constant expression (W: a supported_width)
#define MAGAT_WIDTH_SWITCH(W, CALL)        \
  switch (W) {                             \
    case 16: { constexpr int WW = 16; CALL; } break;   \
    case 32: { constexpr int WW = 32; CALL; } break;   \
    case 64: { constexpr int WW = 64; CALL; } break;   \
    case 128: { constexpr int WW = 128; CALL; } break; \
    default: { constexpr int WW = 256; CALL; }         \
  }
