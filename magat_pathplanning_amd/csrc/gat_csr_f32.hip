// GraphFilterBatchAttentional.forward for LARGE / SPARSE graphs (CSR GSO, any N): BASELINE config 5
// (1000 agents, comm-radius graph).  Same algebra as gat_f32.hip (reference graphML.py:4636-4671, 1724-1827,
// 1180-1286, 713-823) with the GSO given as its edge structure:
//   rowptr [B*(N+1)] absolute offsets into colidx, colidx[e] = j for the e-th edge i -> j of row i
//   (edge (i,j) present  <=>  |S[b,i,j]| > 1e-9 in the dense form).
// Neighbour rows no longer fit LDS (N*G*4 = 512 KB at N=1000), so the kernels gather feature rows straight
// from global memory with 512-byte coalesced row reads that hit the XCD's L2 (all heads of an instance are
// mapped to one XCD); the per-row work mirrors the dense kernel: 8-lane dot products + DPP reductions for the
// scores, wave-uniform scalar loops for the hops.
//   1. csr_transpose_kernel : CSC view (in-edges of every node, sorted by source, with the CSR position of each
//                             edge) - needed because the reference aggregates over COLUMNS of the row-softmax
//                             (x @ aij, graphML.py:1757)
//   2. Z = X @ [W_p | H_pk]^T on fp32 MFMA (conv_gemm_f32.hip)
//   3. csr_scores_kernel    : e_ij, row softmax -> att[p][e]   (CSR order)
//   4. csr_hop_kernel (K-1x): T <- U_k + A^T T, last one fused with bias / ReLU / concat store
#include <cstdlib>

#include "magat_common.h"
#include "gat_pack.h"
#include "gat_csr_route.h"

namespace cr = magat_csr;

namespace {

typedef unsigned short u16;

// Storage type of the node-feature tensors (X, Z, hop intermediates, Y): float, or bf16 (u16) for the bf16-storage
// variant of BASELINE config 5.  Arithmetic is fp32 either way; attention values stay fp32.
template <typename ST> __device__ __forceinline__ float to_f32(ST v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<u16>(u16 v) { return magat_bf16_f32(v); }
template <typename ST> __device__ __forceinline__ ST from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ u16 from_f32<u16>(float v) { return magat_bf16_rne(v); }
template <typename ST, int V>
struct __attribute__((aligned(sizeof(ST) * V))) Pack {
  ST v[V];
};
template <int V, typename ST>
__device__ __forceinline__ void load_vec(const ST* ptr, float (&o)[V]) {
  const Pack<ST, V> r = *reinterpret_cast<const Pack<ST, V>*>(ptr);
#pragma unroll
  for (int c = 0; c < V; ++c) o[c] = to_f32<ST>(r.v[c]);
}
template <int V, typename ST>
__device__ __forceinline__ void store_vec(ST* ptr, const float (&o)[V]) {
  Pack<ST, V> r;
#pragma unroll
  for (int c = 0; c < V; ++c) r.v[c] = from_f32<ST>(o[c]);
  *reinterpret_cast<Pack<ST, V>*>(ptr) = r;
}

struct CsrParams {
  const void* X;       // [B*N, G]   (ST)
  const void* Z;       // [B*N, NC]  (ST)
  const int* rowptr;   // [B*(N+1)]
  const int* colidx;   // [nnz]
  const int* cscptr;   // [B*(N+1)] (workspace)
  const int* cscsrc;   // [nnz] source node i of each in-edge
  const int* cscpos;   // [nnz] position of that edge in CSR order
  float* att;          // [P][nnz] attention values in CSR order
  const void* Told;    // hop input rows (ST)  (row = (b*N+i), head offset applied by caller)
  void* Tnew;          // (ST)
  const float* bias;
  void* Y;             // (ST)
  int B, N, K, P, mode, concat;
  int NC, qoff, uoff, c1off, c2off, ldy;
  long long nnz;
  int k;               // hop index (U_k added)
  long long told_off;              // element offset of the first Told row inside its buffer
  int told_ld, told_head_stride;   // addressing of Told rows: Told + told_off + (b*N+i)*told_ld + head*told_head_stride
  int last;
  int act_relu;           // apply ReLU in the last hop's store (inference); 0 in training (autograd owns it)
  int y_f32;              // bf16 storage only: Y is a float32 buffer - the last store widens the bf16-ROUNDED result (the values
                          // a bf16 Y would hold; saves the caller's cast kernel)
};

// the layer's result rows: ST, or (bf16 storage, y_f32) the same rounded values as float32
template <int V, typename ST>
__device__ __forceinline__ void store_y(void* Y, int y_f32, long long off, const float (&o)[V]) {
  if (sizeof(ST) == 2 && y_f32) {
    float r[V];
#pragma unroll
    for (int c = 0; c < V; ++c) r[c] = __builtin_bit_cast(float, (unsigned)magat_bf16_rne(o[c]) << 16);
    store_vec<V, float>(static_cast<float*>(Y) + off, r);
  } else {
    store_vec<V, ST>(static_cast<ST*>(Y) + off, o);
  }
}

// ---- 1. CSR -> CSC (per instance), deterministic: counting sort + per-column insertion sort by source
__global__ __launch_bounds__(256) void csr_transpose_kernel(const int* __restrict__ rowptr,
                                                            const int* __restrict__ colidx, int* __restrict__ cscptr,
                                                            int* __restrict__ csctmp, int N) {
  extern __shared__ int cnt[];          // [N+1] counts -> offsets, then [N] cursors
  int* cur = cnt + N + 1;
  const int b = blockIdx.x, t = threadIdx.x;
  const int* rp = rowptr + (long long)b * (N + 1);
  const int e0 = rp[0], e1 = rp[N];
  for (int j = t; j <= N; j += 256) cnt[j] = 0;
  __syncthreads();
  for (int e = e0 + t; e < e1; e += 256) atomicAdd(&cnt[colidx[e] + 1], 1);
  __syncthreads();
  if (t < 64) {                         // exclusive scan by one wave
    int carry = 0;
    for (int base = 0; base <= N; base += 64) {
      const int j = base + t;
      int v = j <= N ? cnt[j] : 0, inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (t >= o) inc += u;
      }
      if (j <= N) cnt[j] = carry + inc;
      carry += __shfl(inc, 63, 64);
    }
  }
  __syncthreads();
  int* cp = cscptr + (long long)b * (N + 1);
  for (int j = t; j <= N; j += 256) cp[j] = e0 + cnt[j];
  for (int j = t; j < N; j += 256) cur[j] = cnt[j];
  __syncthreads();
  for (int e = e0 + t; e < e1; e += 256) {      // unordered parallel fill (slot order depends on timing) ...
    const int slot = e0 + atomicAdd(&cur[colidx[e]], 1);
    csctmp[slot] = e;
  }
}

// ... which csr_sort_columns_kernel turns into a deterministic order: one wave per column rank-sorts the column's
// CSR positions (= source rows ascending) and looks the source row of each in-edge up by bisection in rowptr.
__global__ __launch_bounds__(256) void csr_sort_columns_kernel(const int* __restrict__ rowptr,
                                                               const int* __restrict__ cscptr,
                                                               const int* __restrict__ csctmp, int* __restrict__ cscsrc,
                                                               int* __restrict__ cscpos, int N, long long cols) {
  const int lane = threadIdx.x & 63;
  const long long col = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (col >= cols) return;
  const int b = (int)(col / N), j = (int)(col % N);
  const int* rp = rowptr + (long long)b * (N + 1);
  const int* cp = cscptr + (long long)b * (N + 1);
  const int a = cp[j], d = cp[j + 1] - a;
  for (int t = lane; t < d; t += 64) {
    const int v = csctmp[a + t];
    int rank = 0;
    for (int u = 0; u < d; ++u) rank += csctmp[a + u] < v ? 1 : 0;
    int lo = 0, hi = N - 1;                      // last row i with rp[i] <= v
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (rp[mid] <= v) lo = mid; else hi = mid - 1;
    }
    cscpos[a + rank] = v;
    cscsrc[a + rank] = lo;
  }
}

// ---- 3. scores + row softmax.  8 lanes per row, 32 rows per 256-thread block.
template <int G, typename ST>
__global__ __launch_bounds__(256) void csr_scores_kernel(const CsrParams p) {
  constexpr int GC = G / 4, CP8 = GC / 8 > 0 ? GC / 8 : 1, LE = GC < 8 ? GC : 8;
  const int N = p.N;
  const int rows_per_block = 256 / LE;
  const int tiles = (N + rows_per_block - 1) / rows_per_block;
  // block -> (instance, head, row tile): heads and tiles of an instance stay on one XCD
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int per = p.P * tiles;
  const int b = xcd + MAGAT_NUM_XCD * (slot / per);
  if (b >= p.B) return;
  const int head = (slot % per) / tiles, tile = slot % tiles;
  const int t = threadIdx.x, es = t % LE, i = tile * rows_per_block + t / LE;
  if (i >= N) return;
  const int* rp = p.rowptr + (long long)b * (N + 1);
  const int e0 = rp[i], e1 = rp[i + 1];
  if (e1 <= e0) return;
  const ST* Zb = static_cast<const ST*>(p.Z) + (long long)b * N * p.NC;
  float* att = p.att + (long long)head * p.nnz;
  // Row softmax without cross-lane memory traffic: the raw scores are written by one lane and later rewritten
  // by that same lane (program order makes its own stores visible to it); max and sum are carried online in
  // registers, identically in every lane of the group.
  float mx = -__builtin_inff(), sum = 0.f;
  auto online = [&](float d) {
    const float m2 = fmaxf(mx, d);
    sum = sum * __expf(mx - m2) + __expf(d - m2);
    mx = m2;
  };
  if (p.mode == MAGAT_MODE_KEYQUERY) {
    const ST* xr = static_cast<const ST*>(p.X) + ((long long)b * N + i) * G;
    float xi[CP8][4];
#pragma unroll
    for (int q = 0; q < CP8; ++q) load_vec<4, ST>(xr + 4 * (es + LE * q), xi[q]);
    const int qo = p.qoff + head * G;
    for (int e = e0; e < e1; e += 2) {
      const int j0 = p.colidx[e];
      const bool two = e + 1 < e1;
      const int j1 = two ? p.colidx[e + 1] : j0;
      const ST* q0 = Zb + (long long)j0 * p.NC + qo;
      const ST* q1 = Zb + (long long)j1 * p.NC + qo;
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int q = 0; q < CP8; ++q) {
        float a0[4], a1[4];
        load_vec<4, ST>(q0 + 4 * (es + LE * q), a0);
        load_vec<4, ST>(q1 + 4 * (es + LE * q), a1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          d0 = fmaf(xi[q][c], a0[c], d0);
          d1 = fmaf(xi[q][c], a1[c], d1);
        }
      }
      if (LE == 8) {
        d0 = oct_sum(d0);
        d1 = oct_sum(d1);
      } else {
#pragma unroll
        for (int o = LE / 2; o > 0; o >>= 1) {
          d0 += __shfl_xor(d0, o, 64);
          d1 += __shfl_xor(d1, o, 64);
        }
      }
      if (es == 0) {
        att[e] = d0;
        if (two) att[e + 1] = d1;
      }
      online(d0);
      if (two) online(d1);
    }
    if (es == 0) {
      const float inv = 1.f / sum;
      for (int e = e0; e < e1; ++e) att[e] = __expf(att[e] - mx) * inv;
    }
  } else {
    const float c2 = to_f32<ST>(Zb[(long long)i * p.NC + p.c2off + head]);
    for (int e = e0 + es; e < e1; e += LE) {
      const float v = to_f32<ST>(Zb[(long long)p.colidx[e] * p.NC + p.c1off + head]) + c2;
      const float l = v > 0.f ? v : 0.2f * v;
      att[e] = l;
      online(l);
    }
    // combine the lanes' (max, sum) pairs
    float gm = mx;
    if (LE == 8) gm = oct_max(gm);
    else
#pragma unroll
      for (int o = LE / 2; o > 0; o >>= 1) gm = fmaxf(gm, __shfl_xor(gm, o, 64));
    float gs = sum > 0.f ? sum * __expf(mx - gm) : 0.f;
    if (LE == 8) gs = oct_sum(gs);
    else
#pragma unroll
      for (int o = LE / 2; o > 0; o >>= 1) gs += __shfl_xor(gs, o, 64);
    const float inv = 1.f / gs;
    for (int e = e0 + es; e < e1; e += LE) att[e] = __expf(att[e] - gm) * inv;
  }
}

// ---- 4. one Horner hop: out[j] = U_k[j] + sum_{in-edges (i -> j)} att[pos] * Told[i]; wave per output row
template <int F, typename ST>
__global__ __launch_bounds__(256) void csr_hop_kernel(const CsrParams p) {
  constexpr int VEC = F >= 64 ? F / 64 : 1;
  constexpr int LANES = F >= 64 ? 64 : F;
  const int N = p.N;
  const int tiles = (N + 3) / 4;         // 4 rows (waves) per block
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int per = p.P * tiles;
  const int b = xcd + MAGAT_NUM_XCD * (slot / per);
  if (b >= p.B) return;
  const int head = (slot % per) / tiles, tile = slot % tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = tile * 4 + wave;
  if (j >= N || lane >= LANES) return;
  const int* cp = p.cscptr + (long long)b * (N + 1);
  const int s0 = cp[j], s1 = cp[j + 1];
  const float* att = p.att + (long long)head * p.nnz;
  const ST* Tb = static_cast<const ST*>(p.Told) + p.told_off + (long long)b * N * p.told_ld +
                 (long long)head * p.told_head_stride + VEC * lane;
  const ST* Zr = static_cast<const ST*>(p.Z) + ((long long)b * N + j) * p.NC + p.uoff + (head * p.K + p.k) * F + VEC * lane;
  float acc[VEC];
  load_vec<VEC, ST>(Zr, acc);
  for (int s = s0; s < s1; s += 2) {
    const int i0 = p.cscsrc[s];
    const float a0 = att[p.cscpos[s]];
    float t0[VEC];
    load_vec<VEC, ST>(Tb + (long long)i0 * p.told_ld, t0);
    if (s + 1 < s1) {
      const int i1 = p.cscsrc[s + 1];
      const float a1 = att[p.cscpos[s + 1]];
      float t1[VEC];
      load_vec<VEC, ST>(Tb + (long long)i1 * p.told_ld, t1);
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = fmaf(a1, t1[c], fmaf(a0, t0[c], acc[c]));
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = fmaf(a0, t0[c], acc[c]);
    }
  }
  if (p.last) {
    if (p.bias) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] += p.bias[VEC * lane + c];
    }
    if (p.act_relu) {
#pragma unroll
      for (int c = 0; c < VEC; ++c) acc[c] = magat_relu(acc[c]);
    }
    store_y<VEC, ST>(p.Y, p.y_f32, ((long long)b * N + j) * p.ldy + head * F + VEC * lane, acc);
  } else {
    store_vec<VEC, ST>(static_cast<ST*>(p.Tnew) + (((long long)b * N + j) * p.P + head) * F + VEC * lane, acc);
  }
}

// K == 1: Y = U_0 + bias (no graph work)
template <int F, typename ST>
__global__ void csr_k1_kernel(const CsrParams p) {
  const long long total = (long long)p.B * p.N * p.P * (F / 4);
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % (F / 4));
    const long long r = idx / (F / 4);
    const int head = (int)(r % p.P);
    const long long m = r / p.P;
    float v[4];
    load_vec<4, ST>(static_cast<const ST*>(p.Z) + m * p.NC + p.uoff + head * F + 4 * c, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (p.bias) v[q] += p.bias[4 * c + q];
      if (p.act_relu) v[q] = magat_relu(v[q]);
    }
    store_y<4, ST>(p.Y, p.y_f32, m * p.ldy + head * F + 4 * c, v);
  }
}


// ---- LDS-tiled forms of the score and hop kernels for N <= 1024 (BASELINE config 5: N = 1000) ------------------------------
// The per-edge gathers above read every neighbour row from L2 (256-512 B per edge and head: 3.6 GB per c5 step, the
// kernels sat at 13 % of the HBM roof).  Here one workgroup owns an (instance, head) pair and walks the feature axis in
// passes of 128 BYTES per row (32 fp32 or 64 bf16 features): the pass's [N][128 B] slice of the gathered tensor (Q_p for
// the scores, the hop input for a hop) is streamed into LDS once (LDS-direct loads), and every edge then gathers its
// 16 bytes per lane from LDS.  8 lanes per graph row, 8 rows per wave step.  Partial scores of the passes are accumulated
// in att[] by the lane that owns the edge (edge k of a row belongs to lane k & 7 of the row's group: same-thread
// read-after-write, always coherent); owners prefetch their previous partials as one batch before the edge loop, and the
// value enters the 8-lane reduction of the dot product as an extra term of its owner - no dependent load in the loop.
// LPR = lanes per graph row (8: 128-byte slices, one 1024-thread workgroup per CU at N = 1000; 4: 64-byte slices, 512-thread
// workgroups, two per CU - one streams its slice in while the other computes).  32 edges of a row take the batched path.
constexpr int TILED_EDGES = 32;
template <int LPR>
__device__ __forceinline__ float grp_sum(float d) {
  if (LPR == 8) return oct_sum(d);
  d += __shfl_xor(d, 1, 64);
  d += __shfl_xor(d, 2, 64);
  return d;
}

template <typename ST, int LPR>
__device__ __forceinline__ void tile_dma(char* tile, const ST* src_base, long long row_stride_elems, int N, int t) {
  // rows n = 0..N-1, 16 LPR bytes each from src_base + n * row_stride: one wave instruction moves 64 / LPR rows (1 KB)
  constexpr int RPI = 64 / LPR;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), nw = (int)(blockDim.x >> 6);
  for (int g = wave; g * RPI < N; g += nw) {
    const int n = g * RPI + lane / LPR;
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)tile + (unsigned)g * 1024u);
    if (n < N) {
      const char* src = reinterpret_cast<const char*>(src_base + (long long)n * row_stride_elems) + (lane & (LPR - 1)) * 16;
      asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0v) : "memory", "m0");
    }
  }
}

typedef unsigned tv_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 tv_bf2 __attribute__((ext_vector_type(2)));
template <typename ST> struct TileVec;            // the 16 bytes a lane owns of a tile row, as floats
template <> struct TileVec<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ float dot(const unsigned (&a)[4], const unsigned (&b)[4]) {     // raw 16-byte pieces
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) d = fmaf(__builtin_bit_cast(float, a[c]), __builtin_bit_cast(float, b[c]), d);
    return d;
  }
  static __device__ __forceinline__ void load(const void* p, float (&o)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  }
};
template <> struct TileVec<u16> {
  static constexpr int E = 8;
  static __device__ __forceinline__ float dot(const unsigned (&a)[4], const unsigned (&b)[4]) {   // v_dot2c_f32_bf16: exact
    float d = 0.f;                                                                               // products, fp32 accumulation
#pragma unroll
    for (int c = 0; c < 4; ++c)
      d = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(tv_bf2, a[c]), __builtin_bit_cast(tv_bf2, b[c]), d, false);
    return d;
  }
  static __device__ __forceinline__ void load(const void* p, float (&o)[8]) {
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
    const u32x4_ v = *reinterpret_cast<const u32x4_*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[2 * q] = __builtin_bit_cast(float, v[q] << 16);
      o[2 * q + 1] = __builtin_bit_cast(float, v[q] & 0xffff0000u);
    }
  }
};

// The walk order of an instance's rows: RANKED BY EDGE COUNT (descending), so that the 8 rows of a wave step have (almost) the same
// number of edges - a step runs as many edge slots as its longest row has, and in index order that was ~9.5 slots for the 5.4
// edges per row of config 5.  Counting sort in LDS behind the tile (one thread per row; the order inside a bin is whatever the
// LDS atomics make it - no result depends on it: a row's arithmetic does not know its position), and the (row, first edge,
// edge count) of EVERY position this wave walks - at most 8 steps of 8 rows (N <= 1024, 16 waves) - lands in one register
// triple per lane for the whole kernel: lane 8 s + g holds step s, group g.  (Read inside the step's prefetch, the row pointers
// were a second dependent round trip in front of the column and score loads of every step - round 5.)
constexpr int TILED_SCRATCH = 13 * 1024;      // histogram [64] | rows [1024] | first edges [1024] | edge counts [1024]
__device__ __forceinline__ void tiled_row_order(char* scratch, const int* __restrict__ ptr, int N, int t, int q, int& rowh,
                                                int& e0h, int& degh) {
  int* hist = reinterpret_cast<int*>(scratch);
  int* ord = reinterpret_cast<int*>(scratch + 1024);
  const int lane = t & 63;
  if (t < 64) hist[t] = 0;
  __syncthreads();
  int e0 = 0, d = 0, key = 0, slot = 0;
  if (t < N) {
    e0 = ptr[t];
    d = ptr[t + 1] - e0;
    key = 63 - (d < 63 ? d : 63);
    slot = atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  const int c = hist[lane];          // (every wave scans the 64 bins for itself)
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int base = __shfl(incl - c, key, 64);
  if (t < N) {
    ord[base + slot] = t;
    ord[1024 + base + slot] = e0;
    ord[2048 + base + slot] = d;
  }
  __syncthreads();
  const bool ok = q < N;
  rowh = ok ? ord[q] : 0;
  e0h = ok ? ord[1024 + q] : 0;
  degh = ok ? ord[2048 + q] : 0;
}

template <typename ST, int LPR>
__global__ __launch_bounds__(1024) void csr_tiled_scores_kernel(const CsrParams p, int G) {
  extern __shared__ __attribute__((aligned(1024))) char tile[];
  constexpr int E = TileVec<ST>::E;                 // features per lane and pass
  constexpr int TILE_ROW_BYTES = 16 * LPR, RPS = 64 / LPR;          // bytes of a row slice; graph rows per wave step
  constexpr int FPP = TILE_ROW_BYTES / (int)sizeof(ST);   // features per pass
  constexpr int R = TILED_EDGES / LPR;
  const int N = p.N, NP = G / FPP;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int b = xcd + MAGAT_NUM_XCD * (slot / p.P), head = slot % p.P;
  if (b >= p.B) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, es = lane & (LPR - 1), eg = lane / LPR, gbase = lane & ~(LPR - 1);
  const int rstep = RPS * (int)(blockDim.x >> 6);
  const int* rp = p.rowptr + (long long)b * (N + 1);
  const ST* Zb = static_cast<const ST*>(p.Z) + (long long)b * N * p.NC + p.qoff + head * G;
  const ST* Xb = static_cast<const ST*>(p.X) + (long long)b * N * G;
  float* att = p.att + (long long)head * p.nnz;
  static_assert(LPR == 8, "lane 8 s + g <-> (row step s, row group g)");
  int rowh, e0h, degh;
  tile_dma<ST, LPR>(tile, Zb, p.NC, N, t);      // the first pass's slice streams in while the rows are ranked (scratch: behind the tile)
  tiled_row_order(tile + (size_t)((N + RPS - 1) / RPS) * 1024, rp, N, t, RPS * wave + (lane >> 3) * rstep + (lane & 7), rowh, e0h, degh);
  // everything a row step needs from global memory, requested one step ahead (the loop body then only touches LDS)
  struct Row {
    int e0, deg;
    bool ok;
    unsigned xv[4];          // the lane's 16 bytes of x_i, raw
    int cj[R];
    float pre[R];
  };
  for (int h = 0; h < NP; ++h) {
    const bool first = h == 0, last = h == NP - 1;
    auto fetch = [&](int ib, int sidx, Row& w) {
      w.ok = ib + eg < N;
      const int ir = __shfl(rowh, 8 * sidx + eg, 64);
      w.e0 = __shfl(e0h, 8 * sidx + eg, 64);
      w.deg = __shfl(degh, 8 * sidx + eg, 64);
      {
        const tv_u32x4 v = *reinterpret_cast<const tv_u32x4*>(Xb + (long long)ir * G + h * FPP + es * E);
        w.xv[0] = v[0]; w.xv[1] = v[1]; w.xv[2] = v[2]; w.xv[3] = v[3];
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        w.cj[r] = 0;
        w.pre[r] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        // (rows ranked by edge count: past the first batch of 8 edges most wave steps have nothing to ask for)
        if (r > 0 && __builtin_amdgcn_ballot_w64(LPR * r < w.deg) == 0ull) break;
        const bool mine_ok = es + LPR * r < w.deg;
        w.cj[r] = mine_ok ? p.colidx[w.e0 + es + LPR * r] : 0;
        // (agent-scope load: served by L2.  The value was stored by THIS thread in the previous pass, but a plain load may
        //  hit the copy of the line this CU's L1 still holds from the pass before that)
        w.pre[r] = (!first && mine_ok)
                       ? __hip_atomic_load(att + w.e0 + es + LPR * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
      }
    };
    Row cur, nxt;
    if (RPS * wave < N) fetch(RPS * wave, 0, cur);        // in flight together with the slice
    if (h > 0) {
      __syncthreads();                                // every wave is done with the previous slice
#ifndef CSR_WHATIF_NODMA      // (timing experiments, tools/csr_layer_bench.py: wrong results)
      tile_dma<ST, LPR>(tile, Zb + h * FPP, p.NC, N, t);
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef CSR_WHATIF_NOLOOP
    if (p.N > 0) continue;
#endif
    for (int ib = RPS * wave, sidx = 0; ib < N; ib += rstep, ++sidx) {
      if (ib + rstep < N) fetch(ib + rstep, sidx + 1, nxt);
      const int e0 = cur.e0, deg = cur.deg;
      float mine[R];
#pragma unroll
      for (int r = 0; r < R; ++r) mine[r] = 0.f;
      float mx = -__builtin_inff(), sum = 0.f;
      auto online = [&](float d) {
        const float m2 = fmaxf(mx, d);
        sum = sum * __expf(mx - m2) + __expf(d - m2);
        mx = m2;
      };
      auto edge_dot = [&](int j) -> float {
        const tv_u32x4 v = *reinterpret_cast<const tv_u32x4*>(tile + j * TILE_ROW_BYTES + es * 16);
        const unsigned q[4] = {v[0], v[1], v[2], v[3]};
        return TileVec<ST>::dot(cur.xv, q);
      };
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (__builtin_amdgcn_ballot_w64(LPR * r < deg) == 0ull) break;
#pragma unroll
        for (int k = 0; k < LPR; k += 2) {
          // (no row of this wave step has an edge left: at 5.4 edges per row - config 5 - the longest of 8 rows has ~9, and a
          //  full batch of 8 slots for it ran 6-7 empty ones)
          if (k > 0 && __builtin_amdgcn_ballot_w64(LPR * r + k < deg) == 0ull) break;
          const int ka = LPR * r + k, kb = ka + 1;
          const bool va = ka < deg, vb = kb < deg;
          // neighbour index of edge k from its owner lane (past the row's degree: row 0 of the slice, never used)
          const int ja = __shfl(cur.cj[r], gbase + k, 64), jb = __shfl(cur.cj[r], gbase + k + 1, 64);
          float da = edge_dot(ja), db = edge_dot(jb);
          if (es == k) da += cur.pre[r];
          if (es == k + 1) db += cur.pre[r];
          da = grp_sum<LPR>(da);
          db = grp_sum<LPR>(db);
          if (es == k && va) mine[r] = da;
          if (es == k + 1 && vb) mine[r] = db;
        }
      }
      // last pass: the row's softmax over the batched edges from their OWNERS' registers - one maximum and one sum over the
      // 8-lane group (an owner has R candidates) instead of an online update per edge in every lane (two exponentials and a
      // dependent chain per edge: the loop is bound by its vector instructions, not by latency - tools/csr_layer_bench.py)
      if (last) {
        float m = -__builtin_inff();
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (es + LPR * r < deg) m = fmaxf(m, mine[r]);
        m = LPR == 8 ? oct_max(m) : fmaxf(fmaxf(m, __shfl_xor(m, 1, 64)), fmaxf(__shfl_xor(m, 2, 64), __shfl_xor(m, 3, 64)));
        float sl = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (es + LPR * r < deg) sl += __expf(mine[r] - m);
        sum = grp_sum<LPR>(sl);
        mx = m;                                           // (rows without edges: -inf and 0, as the online form leaves them)
      }
      // rows with more than 8 R edges: the rest one by one, owner = lane 0 (dependent loads: rare)
      for (int k = LPR * R; k < deg; ++k) {
        float d = edge_dot(p.colidx[e0 + k]);
        if (es == 0 && !first) d += __hip_atomic_load(att + e0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d = grp_sum<LPR>(d);
        if (es == 0) att[e0 + k] = d;
        if (last) online(d);
      }
      if (!last) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (es + LPR * r < deg) att[e0 + es + LPR * r] = mine[r];
      } else {
        const float inv = sum > 0.f ? 1.f / sum : 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (es + LPR * r < deg) att[e0 + es + LPR * r] = __expf(mine[r] - mx) * inv;
        if (es == 0)
          for (int k = LPR * R; k < deg; ++k)
            att[e0 + k] = __expf(__hip_atomic_load(att + e0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - mx) * inv;
      }
      cur = nxt;
    }
  }
}

// one Horner hop out[j] = U_k[j] + sum over in-edges (i -> j) of att * Told[i], Told slice in LDS
template <typename ST, int LPR>
__global__ __launch_bounds__(1024) void csr_tiled_hop_kernel(const CsrParams p, int F) {
  extern __shared__ __attribute__((aligned(1024))) char tile[];
  constexpr int E = TileVec<ST>::E;
  constexpr int TILE_ROW_BYTES = 16 * LPR, RPS = 64 / LPR;
  constexpr int FPP = TILE_ROW_BYTES / (int)sizeof(ST);
  constexpr int R = TILED_EDGES / LPR;
  const int N = p.N, NP = F / FPP;
  const int bid = blockIdx.x, xcd = bid % MAGAT_NUM_XCD, slot = bid / MAGAT_NUM_XCD;
  const int b = xcd + MAGAT_NUM_XCD * (slot / p.P), head = slot % p.P;
  if (b >= p.B) return;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, es = lane & (LPR - 1), eg = lane / LPR, gbase = lane & ~(LPR - 1);
  const int rstep = RPS * (int)(blockDim.x >> 6);
  const int* cp = p.cscptr + (long long)b * (N + 1);
  const float* att = p.att + (long long)head * p.nnz;
  const ST* Tb = static_cast<const ST*>(p.Told) + p.told_off + (long long)b * N * p.told_ld +
                 (long long)head * p.told_head_stride;
  const ST* Ub = static_cast<const ST*>(p.Z) + (long long)b * N * p.NC + p.uoff + (head * p.K + p.k) * F;
  // rows ranked by IN-edge count, their column pointers in registers for the whole kernel (see the score kernel)
  static_assert(LPR == 8, "lane 8 s + g <-> (row step s, row group g)");
  int rowh, s0h, degh;
  tile_dma<ST, LPR>(tile, Tb, p.told_ld, N, t);      // (the first slice under the ranking, as in the score kernel)
  tiled_row_order(tile + (size_t)((N + RPS - 1) / RPS) * 1024, cp, N, t, RPS * wave + (lane >> 3) * rstep + (lane & 7), rowh, s0h, degh);
  // A step's global reads in TWO stages, each requested a whole step before it is needed: the in-edge lists (source row, CSR
  // position) two steps ahead, the weights att[position] - which depend on them - and the U row one step ahead.
  struct Idx {
    int s0, deg, row;
    bool ok;
    int src[R], pos[R];
  };
  struct Val {
    float acc[E];
    float wgt[R];
  };
  for (int h = 0; h < NP; ++h) {
    auto fetch_idx = [&](int jb, int sidx, Idx& w) {
      w.ok = jb + eg < N;
      w.row = __shfl(rowh, 8 * sidx + eg, 64);
      w.s0 = __shfl(s0h, 8 * sidx + eg, 64);
      w.deg = __shfl(degh, 8 * sidx + eg, 64);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        w.src[r] = 0;
        w.pos[r] = -1;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r > 0 && __builtin_amdgcn_ballot_w64(LPR * r < w.deg) == 0ull) break;
        const bool mine_ok = es + LPR * r < w.deg;
#ifdef CSR_WHATIF_NOIDX
        w.src[r] = es + LPR * r; w.pos[r] = mine_ok ? w.s0 + es + LPR * r : -1;
#else
        w.src[r] = mine_ok ? p.cscsrc[w.s0 + es + LPR * r] : 0;
        w.pos[r] = mine_ok ? p.cscpos[w.s0 + es + LPR * r] : -1;
#endif
      }
    };
    auto fetch_val = [&](int jb, const Idx& ix, Val& w) {
      TileVec<ST>::load(Ub + (long long)ix.row * p.NC + h * FPP + es * E, w.acc);
#pragma unroll
      for (int r = 0; r < R; ++r) w.wgt[r] = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r > 0 && __builtin_amdgcn_ballot_w64(LPR * r < ix.deg) == 0ull) break;
        w.wgt[r] = ix.pos[r] >= 0 ? att[ix.pos[r]] : 0.f;
      }
    };
    Idx cur, nxt, nx2;
    Val cv, nv;
    float bv[E];                 // this lane's bias columns of the pass
#pragma unroll
    for (int c = 0; c < E; ++c) bv[c] = (p.last && p.bias) ? p.bias[h * FPP + es * E + c] : 0.f;
    const int jb0 = RPS * wave;
    if (jb0 < N) {
      fetch_idx(jb0, 0, cur);
      if (jb0 + rstep < N) fetch_idx(jb0 + rstep, 1, nxt);
      fetch_val(jb0, cur, cv);
    }
    if (h > 0) {
      __syncthreads();
#ifndef CSR_WHATIF_NODMA
      tile_dma<ST, LPR>(tile, Tb + h * FPP, p.told_ld, N, t);
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef CSR_WHATIF_NOLOOP
    if (p.N > 0) continue;
#endif
    for (int jb = jb0, sidx = 0; jb < N; jb += rstep, ++sidx) {
      if (jb + 2 * rstep < N) fetch_idx(jb + 2 * rstep, sidx + 2, nx2);
      if (jb + rstep < N) fetch_val(jb + rstep, nxt, nv);
      const int j = cur.row, deg = cur.deg;
      float acc[E];
#pragma unroll
      for (int c = 0; c < E; ++c) acc[c] = cv.acc[c];
#pragma unroll
      for (int r = 0; r < R; ++r) {
#ifdef CSR_WHATIF_NOKLOOP
        break;
#endif
        if (__builtin_amdgcn_ballot_w64(LPR * r < deg) == 0ull) break;
#pragma unroll
        for (int k = 0; k < LPR; ++k) {
          if (k > 0 && __builtin_amdgcn_ballot_w64(LPR * r + k < deg) == 0ull) break;      // (as in the score loop)
          // (i, a) of edge LPR r + k from its owner lane; edges past the row's degree carry weight 0 and row 0
          const int i = __shfl(cur.src[r], gbase + k, 64);
          const float a = __shfl(cv.wgt[r], gbase + k, 64);
          float tv[E];
          TileVec<ST>::load(tile + i * TILE_ROW_BYTES + es * 16, tv);
#pragma unroll
          for (int c = 0; c < E; ++c) acc[c] = fmaf(a, tv[c], acc[c]);
        }
      }
      for (int k = LPR * R; k < deg; ++k) {
        const int i = p.cscsrc[cur.s0 + k];
        const float a = att[p.cscpos[cur.s0 + k]];
        float tv[E];
        TileVec<ST>::load(tile + i * TILE_ROW_BYTES + es * 16, tv);
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = fmaf(a, tv[c], acc[c]);
      }
#ifdef CSR_WHATIF_NOSTORE
      if (acc[0] == 1.2345f && acc[3] == 7.f)
#endif
      if (cur.ok) {
        const int col = h * FPP + es * E;
        if (p.last) {
          if (p.bias) {
#pragma unroll
            for (int c = 0; c < E; ++c) acc[c] += bv[c];
          }
          if (p.act_relu) {
#pragma unroll
            for (int c = 0; c < E; ++c) acc[c] = magat_relu(acc[c]);
          }
          store_y<E, ST>(p.Y, p.y_f32, ((long long)b * N + j) * p.ldy + head * F + col, acc);
        } else {
          store_vec<E, ST>(static_cast<ST*>(p.Tnew) + (((long long)b * N + j) * p.P + head) * F + col, acc);
        }
      }
      cur = nxt; nxt = nx2; cv = nv;
    }
  }
}

// The launchers take their grid from the Route (gat_csr_route.h) and refuse one that an unsigned launch cannot express.
// (the 64-byte-slice tiled form - 512-thread workgroups, two per CU, option CSR_TILED bit 2 of rounds 2-4 - doubled the passes
//  and their per-row bookkeeping and measured 27 % slower: removed in round 5; LPR = 8 is the one instantiated)
template <typename ST, int LPR = 8>
int run_tiled(const CsrParams& p, int width, bool scores, long long grid, hipStream_t st) {
  constexpr int RPS = 64 / LPR;
  if (grid > cr::kGridMax) return MAGAT_ERR_BAD_SHAPE;
  const size_t lds = (size_t)((p.N + RPS - 1) / RPS) * 1024 + TILED_SCRATCH;
  const void* fn = scores ? reinterpret_cast<const void*>(&csr_tiled_scores_kernel<ST, LPR>)
                          : reinterpret_cast<const void*>(&csr_tiled_hop_kernel<ST, LPR>);
  const int slot = (scores ? MAGAT_LDS_CSR_TILED_A : MAGAT_LDS_CSR_TILED_B) + (sizeof(ST) == 2 ? 2 : 0) + (LPR == 4 ? 4 : 0);
  if (magat_ensure_dyn_lds(fn, slot, lds) != MAGAT_OK) return MAGAT_ERR_LAUNCH;
  const int threads = LPR == 4 ? 512 : 1024;
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_GRAPH, st);
  if (scores)
    hipLaunchKernelGGL((csr_tiled_scores_kernel<ST, LPR>), dim3((unsigned)grid), dim3(threads), lds, st, p, width);
  else
    hipLaunchKernelGGL((csr_tiled_hop_kernel<ST, LPR>), dim3((unsigned)grid), dim3(threads), lds, st, p, width);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
template <typename KFn>
int run_rows(KFn kern, const CsrParams& p, long long grid, hipStream_t st) {      // the per-edge score and hop kernels
  if (grid > cr::kGridMax) return MAGAT_ERR_BAD_SHAPE;
  const int pid = magat_prof_begin(MAGAT_TAG_GAT_GRAPH, st);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, st, p);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
template <int F, typename ST>
int run_k1(const CsrParams& p, long long grid, hipStream_t st) {
  hipLaunchKernelGGL((csr_k1_kernel<F, ST>), dim3((unsigned)grid), dim3(256), 0, st, p);
  return magat_check_launch();
}

template <typename ST>
__global__ void head_mean_relu_csr_kernel(const ST* __restrict__ ytmp, void* __restrict__ y, long long M, int P,
                                          int F, int ldy, int y_f32) {
  const int FC = F / 4;
  const long long total = M * FC;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long m = idx / FC;
    const int c = (int)(idx - m * FC);
    float s[4], u[4];
    load_vec<4, ST>(ytmp + m * (long long)P * F + 4 * c, s);
    for (int q = 1; q < P; ++q) {
      load_vec<4, ST>(ytmp + (m * P + q) * (long long)F + 4 * c, u);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] += u[e];
    }
    const float fp = (float)P;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = magat_relu(s[e] / fp);
    store_y<4, ST>(y, y_f32, m * ldy + 4 * c, s);
  }
}

// maps GEMM Z = X @ Bt^T + colbias in the storage type: fp32 (fp32 MFMA / bf16x6 split) or bf16 in, bf16 out
// (one bf16 MFMA product per element pair, fp32 accumulate; weights = plane 0 of the packed bf16x3 block)
template <typename ST>
int csr_maps_gemm(const ST* X, const float* packed, ST* Z, int M, int G, const PackLayout& L, void* stream, int32_t* status);
template <>
int csr_maps_gemm<float>(const float* X, const float* packed, float* Z, int M, int G, const PackLayout& L, void* stream,
                         int32_t* status) {
  return magat_gat_maps_gemm(X, packed, Z, M, G, L.NC, L.NC, stream, 0, status);
}
template <>
int csr_maps_gemm<u16>(const u16* X, const float* packed, u16* Z, int M, int G, const PackLayout& L, void* stream, int32_t*) {
  // (NC and G are multiples of 32: the route refuses the call otherwise, REFUSE_BF16_MAPS)
  magat_conv_gemm_desc d = {};
  d.in = reinterpret_cast<const float*>(X);
  d.wt = packed + (((size_t)L.NC * (G + 1) + 3) & ~(size_t)3);     // bf16x3 planes; plane 0 = RNE bf16 of Bt
  d.bias = packed + (size_t)L.NC * G;
  d.out = reinterpret_cast<float*>(Z);
  d.M = M; d.Cin = G; d.lda = G; d.Hin = d.Win = 1; d.kH = d.kW = 1; d.stride = 1; d.Hout = d.Wout = 1;
  d.Cout = L.NC; d.ldc = L.NC; d.tag = MAGAT_TAG_GAT_MAPS; d.in_fmt = 3; d.out_fmt = 2;
  return magat_conv_gemm_f32(&d, stream);
}

int route_rc(const cr::Route& r) {
  const cr::Code c = cr::refusal_code(r.refusal);
  return c == cr::CODE_OK ? MAGAT_OK : c == cr::CODE_BAD_SHAPE ? MAGAT_ERR_BAD_SHAPE : MAGAT_ERR_UNSUPPORTED;
}
cr::RouteIn route_in(int B, int N, long long nnz, int G, int F, int K, int P, int mode, int concat, size_t esz, bool have_csc,
                     cr::Pass pass) {
  cr::RouteIn in = {};
  in.B = B; in.N = N; in.nnz = nnz; in.G = G; in.F = F; in.K = K; in.P = P; in.mode = mode; in.concat = concat;
  in.esz = (int)esz; in.have_csc = have_csc; in.pass = pass;
  in.csr_tiled = magat_opt(MAGAT_OPT_CSR_TILED); in.csr_fused = magat_opt(MAGAT_OPT_CSR_FUSED);
  return in;
}

// Where hop h writes: the ping-pong pair of the inference workspace, or block h of the T_k the training forward keeps
// (T_k for k = K-2-h; `kept` = elements of a block).  Hop h > 0 reads what hop h - 1 wrote.
struct HopBuffers {
  void* buf[2];
  size_t kept;
  template <typename ST> ST* at(int h) const {
    return kept ? static_cast<ST*>(buf[0]) + h * kept : static_cast<ST*>(buf[h & 1]);
  }
};

// Transposition, scores / K = 1 and hops of a route, for the inference entries and the training forward alike
template <typename ST>
int csr_walk(const cr::Route& r, CsrParams p, int G, int F, int* csctmp, const HopBuffers& hb, hipStream_t st) {
  int rc = MAGAT_OK;
  if (r.k1 == cr::K1_ALONE) {
    MAGAT_WIDTH_SWITCH(F, rc = (run_k1<WW, ST>(p, r.grid_k1, st)));
    return rc;
  }
  if (r.transpose) {
    const int pid = r.transpose_booked ? magat_prof_begin(MAGAT_TAG_GSO_CSR, st) : 0;
    hipLaunchKernelGGL(csr_transpose_kernel, dim3((unsigned)r.grid_transpose), dim3(256), (size_t)(2 * p.N + 2) * sizeof(int), st,
                       p.rowptr, p.colidx, const_cast<int*>(p.cscptr), csctmp, p.N);
    hipLaunchKernelGGL(csr_sort_columns_kernel, dim3((unsigned)r.grid_sort), dim3(256), 0, st, p.rowptr, p.cscptr, csctmp,
                       const_cast<int*>(p.cscsrc), const_cast<int*>(p.cscpos), p.N, (long long)p.B * p.N);
    if (r.transpose_booked) magat_prof_end(pid, st);
    if ((rc = magat_check_launch()) != MAGAT_OK) return rc;
  }
  if (r.scores == cr::GRAPH_TILED) rc = run_tiled<ST>(p, G, true, r.grid_scores, st);
  else if (r.scores == cr::GRAPH_EDGE) MAGAT_WIDTH_SWITCH(G, rc = run_rows((csr_scores_kernel<WW, ST>), p, r.grid_scores, st));
  if (rc != MAGAT_OK) return rc;
  if (r.k1 == cr::K1_AFTER_SCORES) {
    MAGAT_WIDTH_SWITCH(F, rc = (run_k1<WW, ST>(p, r.grid_k1, st)));
    if (rc != MAGAT_OK) return rc;
  }
  // hops k = K-2 .. 0; the first reads U_{K-1} straight out of Z
  for (int h = 0; h < r.hops; ++h) {
    p.k = r.hops - 1 - h;
    p.last = p.k == 0;
    if (h == 0) {
      p.Told = p.Z;                          // row (b*N+i): + i*NC, head: + head*K*F
      p.told_off = p.uoff + (p.K - 1) * F;
      p.told_ld = p.NC;
      p.told_head_stride = p.K * F;
    } else {
      p.Told = hb.at<ST>(h - 1);
      p.told_off = 0;
      p.told_ld = p.P * F;
      p.told_head_stride = F;
    }
    p.Tnew = hb.at<ST>(h);
    if (r.hop_kind == cr::GRAPH_TILED) rc = run_tiled<ST>(p, F, false, r.grid_hop, st);
    else MAGAT_WIDTH_SWITCH(F, rc = run_rows((csr_hop_kernel<WW, ST>), p, r.grid_hop, st));
    if (rc != MAGAT_OK) return rc;
  }
  return MAGAT_OK;
}

CsrParams csr_params(const void* X, const void* Z, const int* rowptr, const int* colidx, const int* cscptr, const int* cscsrc,
                     const int* cscpos, float* att, const float* bias, void* Y, int ldy, long long nnz, int B, int N, int G, int F,
                     int K, int P, int mode) {
  const PackLayout L = pack_layout(G, F, K, P, mode);
  CsrParams p = {};
  p.X = X; p.Z = Z; p.rowptr = rowptr; p.colidx = colidx; p.cscptr = cscptr; p.cscsrc = cscsrc; p.cscpos = cscpos;
  p.att = att; p.bias = bias; p.Y = Y; p.ldy = ldy; p.nnz = nnz;
  p.B = B; p.N = N; p.K = K; p.P = P; p.mode = mode;
  p.NC = L.NC; p.qoff = L.qoff; p.uoff = L.uoff; p.c1off = L.c1off; p.c2off = L.c2off;
  return p;
}

// Validate, ask gat_csr_route.h which launches the call takes, set up the parameters, walk
template <typename ST>
int csr_forward(const ST* X, const int* rowptr, const int* colidx, long long nnz, const float* packed,
                const float* bias, void* Y, int ldy, float* att_opt, void* workspace, size_t workspace_bytes, int B,
                int N, int G, int F, int K, int P, int mode, int concat, void* stream,
                const float* edge_vals = nullptr, const int* pre_cscptr = nullptr, const int* pre_cscsrc = nullptr,
                const int* pre_cscpos = nullptr, int y_f32 = 0) {
  if (!X || !rowptr || !packed || !Y || (nnz > 0 && !colidx)) return MAGAT_ERR_NULL;
  const bool have_csc = pre_cscptr && pre_cscsrc && pre_cscpos;     // made by magat_gso_csr_build (once per GSO)
  cr::RouteIn in = route_in(B, N, nnz, G, F, K, P, mode, concat, sizeof(ST), have_csc, cr::PASS_INFER);
  in.ldy = ldy; in.attention = att_opt != nullptr; in.edge_vals = edge_vals != nullptr; in.y_f32 = y_f32 != 0;
  in.x_aligned = (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  in.cus = gat_device_cus();
  const cr::Route r = cr::route(in);
  if (r.refusal != cr::REFUSE_NONE && r.refusal != cr::REFUSE_BF16_MAPS) return route_rc(r);
  const cr::Workspace& w = r.ws;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) || workspace_bytes < w.total)
    return MAGAT_ERR_WORKSPACE;
  if (r.refusal != cr::REFUSE_NONE) return route_rc(r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  ST* Z = reinterpret_cast<ST*>(ws + w.z);
  const int* cscptr = have_csc ? pre_cscptr : reinterpret_cast<int*>(ws + w.cscptr);
  const int* cscsrc = have_csc ? pre_cscsrc : reinterpret_cast<int*>(ws + w.cscsrc);
  const int* cscpos = have_csc ? pre_cscpos : reinterpret_cast<int*>(ws + w.cscpos);
  const bool gnn = mode == MAGAT_MODE_GNN, cosine = mode == MAGAT_MODE_SIMILARITY;
  float* att = gnn ? const_cast<float*>(edge_vals) : (att_opt ? att_opt : reinterpret_cast<float*>(ws + w.att));
  ST* Ytmp = reinterpret_cast<ST*>(ws + w.ytmp);

  if (r.fused) {
    // maps on the matrix cores inside the score / hop kernels: Q and U never exist in memory (gat_csr_fused.hip)
    return magat_gat_csr_fused_forward(reinterpret_cast<const uint16_t*>(X), rowptr, colidx, cscptr, cscsrc, cscpos, nnz,
                                                packed + magat_gat_csr_fused_offset(r.NC, G), bias, Y, ldy, y_f32,
                                                reinterpret_cast<float*>(ws + w.att), att_opt,
                                                reinterpret_cast<int*>(ws + w.order), B, N, P, (int)r.grid_fused_scores,
                                                (int)r.grid_fused_hop, st);
    // (MAGAT_ERR_UNSUPPORTED before any launch: result rows / bias not 16-byte aligned, ldy not a multiple of 8 bf16 / 4 float32
    //  elements - magat_hip.h "Alignment" (2); the workspace the caller sized for this form holds no maps, so there is no
    //  fall-through to the unfused kernels)
  }
  const PackLayout L = pack_layout(G, F, K, P, mode);
  int rc = r.maps == cr::MAPS_F32 ? magat_gat_maps_gemm(reinterpret_cast<const float*>(X), packed, reinterpret_cast<float*>(Z), B * N, G,
                                                       L.NC, L.NC, stream, 0, nullptr, 1)
                                  : csr_maps_gemm<ST>(X, packed, Z, B * N, G, L, stream, reinterpret_cast<int32_t*>(ws + w.status));
  if (rc != MAGAT_OK) return rc;
  const void* Xs = X;      // what the scores read as x_i (the taps come from Z)
  if (r.prepare) {
    rc = magat_gat_cos_prepare(reinterpret_cast<const float*>(X), reinterpret_cast<float*>(Z), reinterpret_cast<float*>(ws + w.xhat),
                               (long long)B * N, G, L.qoff, L.NC, 0, stream);
    if (rc != MAGAT_OK) return rc;
    Xs = ws + w.xhat;
  }
  // (the per-head rows of the mean form stay in the storage type)
  CsrParams p = csr_params(Xs, Z, rowptr, colidx, cscptr, cscsrc, cscpos, att, bias, concat ? Y : static_cast<void*>(Ytmp),
                           concat ? ldy : P * F, nnz, B, N, G, F, K, P, cosine ? MAGAT_MODE_KEYQUERY : mode);
  p.concat = concat; p.y_f32 = concat ? y_f32 : 0; p.act_relu = r.act_relu;
  const HopBuffers hb = {{ws + w.t0, ws + w.t1}, 0};
  rc = csr_walk<ST>(r, p, G, F, reinterpret_cast<int*>(ws + w.csctmp), hb, st);
  if (rc != MAGAT_OK || !r.head_mean) return rc;
  const int pid = magat_prof_begin(MAGAT_TAG_HEAD_MEAN, st);
  hipLaunchKernelGGL((head_mean_relu_csr_kernel<ST>), dim3((unsigned)r.grid_mean), dim3(256), 0, st, Ytmp, Y, (long long)B * N, P, F,
                     ldy, y_f32);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

// the three *_workspace_bytes exports: the layout's total, 0 for a call without dimensions
size_t ws_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode, int concat, size_t esz, bool have_csc) {
  if (!cr::dims_ok(B, N, nnz, K, P, G, F)) return 0;
  const cr::RouteIn in = route_in(B, N, nnz, G, F, K, P, mode, concat, esz, have_csc, cr::PASS_INFER);
  return cr::workspace(in, cr::fused_form(in)).total;
}

}  // namespace

// float32 <-> bf16 (RNE) row blocks around the bf16-storage layer: src [M][ld_src] -> dst [M][ld_dst], `width` columns
namespace {
__global__ void cast_f32_bf16_kernel(const float* __restrict__ src, u16* __restrict__ dst, long long M, int width,
                                     int ld_src, int ld_dst, const int* __restrict__ run_if) {
  if (run_if && *run_if == 0) return;      // (predicated form: behind the encoder's range-guard re-run)
  const int wq = width / 4;
  const long long total = M * wq;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long m = idx / wq;
    const int c = (int)(idx - m * wq) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + m * ld_src + c);
    uint2 o;
    o.x = (unsigned)magat_bf16_rne(v[0]) | ((unsigned)magat_bf16_rne(v[1]) << 16);
    o.y = (unsigned)magat_bf16_rne(v[2]) | ((unsigned)magat_bf16_rne(v[3]) << 16);
    *reinterpret_cast<uint2*>(dst + m * ld_dst + c) = o;
  }
}
__global__ void cast_bf16_f32_kernel(const u16* __restrict__ src, float* __restrict__ dst, long long M, int width,
                                     int ld_src, int ld_dst) {
  const int wq = width / 4;
  const long long total = M * wq;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long m = idx / wq;
    const int c = (int)(idx - m * wq) * 4;
    const uint2 v = *reinterpret_cast<const uint2*>(src + m * ld_src + c);
    *reinterpret_cast<f32x4*>(dst + m * ld_dst + c) =
        f32x4{__builtin_bit_cast(float, v.x << 16), __builtin_bit_cast(float, v.x & 0xffff0000u),
              __builtin_bit_cast(float, v.y << 16), __builtin_bit_cast(float, v.y & 0xffff0000u)};
  }
}
}  // namespace

int magat_cast_rows_if(const void* src, void* dst, int to_bf16, long long M, int width, int ld_src, int ld_dst, void* stream,
                       const int32_t* run_if);
extern "C" int magat_cast_rows(const void* src, void* dst, int to_bf16, long long M, int width, int ld_src, int ld_dst,
                               void* stream) {
  return magat_cast_rows_if(src, dst, to_bf16, M, width, ld_src, ld_dst, stream, nullptr);
}
// run_if (float32 -> bf16 only): device flag, the launch returns at once when it is zero
int magat_cast_rows_if(const void* src, void* dst, int to_bf16, long long M, int width, int ld_src, int ld_dst, void* stream,
                       const int32_t* run_if) {
  if (!src || !dst) return MAGAT_ERR_NULL;
  if (run_if && !to_bf16) return MAGAT_ERR_UNSUPPORTED;
  if (M <= 0 || width <= 0 || (width & 3) || (ld_src & 3) || (ld_dst & 3) || ld_src < width || ld_dst < width)
    return MAGAT_ERR_BAD_SHAPE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  long long blocks = (M * (width / 4) + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  const int pid = magat_prof_begin(run_if ? MAGAT_TAG_UNTAGGED : MAGAT_TAG_GAT_CAST, st);      // (predicated: inside the guard's span)
  if (to_bf16)
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)(run_if && blocks > 512 ? 512 : blocks)), dim3(256), 0, st,
                       static_cast<const float*>(src), static_cast<u16*>(dst), M, width, ld_src, ld_dst,
                       reinterpret_cast<const int*>(run_if));
  else
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const u16*>(src),
                       static_cast<float*>(dst), M, width, ld_src, ld_dst);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" size_t magat_gat_csr_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode,
                                                int concat) {
  return ws_bytes(B, N, nnz, G, F, K, P, mode, concat, sizeof(float), false);
}
extern "C" size_t magat_gat_csr_bf16_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode,
                                                     int concat) {
  return ws_bytes(B, N, nnz, G, F, K, P, mode, concat, sizeof(u16), false);
}
// workspace of the *_csc_* entry points (the caller brings the column view: no transpose scratch)
extern "C" size_t magat_gat_csc_workspace_bytes(int B, int N, long long nnz, int G, int F, int K, int P, int mode,
                                                int concat, int bf16) {
  return ws_bytes(B, N, nnz, G, F, K, P, mode, concat, bf16 ? sizeof(u16) : sizeof(float), true);
}

extern "C" int magat_gat_forward_csr_f32(const float* X, const int* rowptr, const int* colidx, long long nnz,
                                         const float* packed, const float* bias, float* Y, int ldy, float* att_opt,
                                         void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K,
                                         int P, int mode, int concat, void* stream) {
  return csr_forward<float>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, att_opt, workspace, workspace_bytes, B, N, G,
                            F, K, P, mode, concat, stream);
}

extern "C" int magat_gnn_forward_csr_f32(const float* X, const int* rowptr, const int* colidx, const float* vals,
                                         long long nnz, const float* packed, const float* bias, float* Y, int ldy,
                                         void* workspace, size_t workspace_bytes, int B, int N, int G, int F, int K,
                                         void* stream) {
  return csr_forward<float>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, nullptr, workspace, workspace_bytes, B, N, G,
                            F, K, 1, MAGAT_MODE_GNN, 1, stream, vals);
}

extern "C" int magat_gat_forward_csr_bf16(const uint16_t* X, const int* rowptr, const int* colidx, long long nnz,
                                          const float* packed, const float* bias, uint16_t* Y, int ldy,
                                          float* att_opt, void* workspace, size_t workspace_bytes, int B, int N, int G,
                                          int F, int K, int P, int mode, int concat, void* stream) {
  return csr_forward<u16>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, att_opt, workspace, workspace_bytes, B, N, G, F,
                          K, P, mode, concat, stream);
}

// forward with the CSC view made by magat_gso_csr_build (skips the per-call transpose)
extern "C" int magat_gat_forward_csc_f32(const float* X, const int* rowptr, const int* colidx, const int* cscptr,
                                         const int* cscsrc, const int* cscpos, long long nnz, const float* packed,
                                         const float* bias, float* Y, int ldy, float* att_opt, void* workspace,
                                         size_t workspace_bytes, int B, int N, int G, int F, int K, int P, int mode,
                                         int concat, void* stream) {
  if (!cscptr || !cscsrc || !cscpos) return MAGAT_ERR_NULL;
  return csr_forward<float>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, att_opt, workspace, workspace_bytes, B, N, G,
                            F, K, P, mode, concat, stream, nullptr, cscptr, cscsrc, cscpos);
}
extern "C" int magat_gat_forward_csc_bf16(const uint16_t* X, const int* rowptr, const int* colidx, const int* cscptr,
                                          const int* cscsrc, const int* cscpos, long long nnz, const float* packed,
                                          const float* bias, uint16_t* Y, int ldy, float* att_opt, void* workspace,
                                          size_t workspace_bytes, int B, int N, int G, int F, int K, int P, int mode,
                                          int concat, void* stream) {
  if (!cscptr || !cscsrc || !cscpos) return MAGAT_ERR_NULL;
  return csr_forward<u16>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, att_opt, workspace, workspace_bytes, B, N, G, F,
                          K, P, mode, concat, stream, nullptr, cscptr, cscsrc, cscpos);
}
extern "C" int magat_gat_forward_csc_bf16_f32out(const uint16_t* X, const int* rowptr, const int* colidx, const int* cscptr,
                                                 const int* cscsrc, const int* cscpos, long long nnz, const float* packed,
                                                 const float* bias, float* Y, int ldy, float* att_opt, void* workspace,
                                                 size_t workspace_bytes, int B, int N, int G, int F, int K, int P, int mode,
                                                 int concat, void* stream) {
  if (!cscptr || !cscsrc || !cscpos) return MAGAT_ERR_NULL;
  return csr_forward<u16>(X, rowptr, colidx, nnz, packed, bias, Y, ldy, att_opt, workspace, workspace_bytes, B, N, G, F,
                          K, P, mode, concat, stream, nullptr, cscptr, cscsrc, cscpos, 1);
}

// Training forward: the split-form forward on float32 MFMA maps that keeps what the backward
// (gat_train.hip) needs - Z, the attention values and the hop intermediates T_k
// (Xhat, norms: GAT_Similarity's form, magat_gat_train_forward_cos_f32 - mode is KeyQuery then, P = 1)
static int train_forward(const float* X, const int* rowptr, const int* colidx, long long nnz, const float* packed,
                         const float* bias, float* Ypre, float* att, float* Z, float* T, int* cscptr, int* cscsrc, int* cscpos,
                         int* csctmp, int B, int N, int G, int F, int K, int P, int mode, void* stream, float* Xhat = nullptr,
                         float* norms = nullptr) {
  if (!X || !rowptr || !packed || !Ypre || !att || !Z || !cscptr || !cscsrc || !cscpos || !csctmp) return MAGAT_ERR_NULL;
  if (nnz > 0 && !colidx) return MAGAT_ERR_NULL;
  if (K > 2 && !T) return MAGAT_ERR_NULL;
  const cr::Route r = cr::route(route_in(B, N, nnz, G, F, K, P, mode, 1, sizeof(float), false, Xhat ? cr::PASS_TRAIN_COS : cr::PASS_TRAIN));
  if (r.refusal != cr::REFUSE_NONE) return route_rc(r);
  const long long M = (long long)B * N;
  const PackLayout L = pack_layout(G, F, K, P, mode);
  int rc = magat_gat_maps_gemm(X, packed, Z, (int)M, G, L.NC, L.NC, stream, 0, nullptr, 1);
  if (rc != MAGAT_OK) return rc;
  if (r.prepare) {      // q^ in place in Z, x^ in Xhat, the norms kept
    magat_form_note(MAGAT_FORM_GAT_COS_TRAIN);
    rc = magat_gat_cos_prepare(X, Z, Xhat, M, G, L.qoff, L.NC, 0, stream, nullptr, norms);
    if (rc != MAGAT_OK) return rc;
    X = Xhat;      // (read below for the scores' x_i only: the taps come from Z)
  }
  CsrParams p = csr_params(X, Z, rowptr, colidx, cscptr, cscsrc, cscpos, att, bias, Ypre, P * F, nnz, B, N, G, F, K, P, mode);
  p.concat = 1;
  const HopBuffers hb = {{T, nullptr}, (size_t)M * P * F};
  return csr_walk<float>(r, p, G, F, csctmp, hb, static_cast<hipStream_t>(stream));
}


extern "C" int magat_gat_train_forward_f32(const float* X, const int* rowptr, const int* colidx, long long nnz,
                                           const float* packed, const float* bias, float* Ypre, float* att, float* Z,
                                           float* T, int* cscptr, int* cscsrc, int* cscpos, int* csctmp, int B, int N,
                                           int G, int F, int K, int P, int mode, void* stream) {
  return train_forward(X, rowptr, colidx, nnz, packed, bias, Ypre, att, Z, T, cscptr, cscsrc, cscpos, csctmp, B, N, G, F, K, P,
                       mode, stream);
}

// GAT_Similarity's training forward (P = 1, F = G): the same launches on (Xhat, Z) behind gat_cos_prepare_kernel, which also
// keeps the two norms of every row for the backward (magat_gat_train_backward_cos_f32, gat_train.hip).  After the call the score
// columns of Z hold q^, not q.
extern "C" int magat_gat_train_forward_cos_f32(const float* X, const int* rowptr, const int* colidx, long long nnz,
                                               const float* packed, const float* bias, float* Ypre, float* att, float* Z,
                                               float* T, float* Xhat, float* norms, int* cscptr, int* cscsrc, int* cscpos,
                                               int* csctmp, int B, int N, int G, int K, void* stream) {
  if (!Xhat || !norms) return MAGAT_ERR_NULL;
  return train_forward(X, rowptr, colidx, nnz, packed, bias, Ypre, att, Z, T, cscptr, cscsrc, cscpos, csctmp, B, N, G, G, K, 1,
                       MAGAT_MODE_KEYQUERY, stream, Xhat, norms);
}
