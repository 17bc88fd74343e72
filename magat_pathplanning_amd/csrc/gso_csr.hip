// Dense GSO (B, N, N) -> its edge structure for the CSR kernels (gat_csr_f32.hip, gat_csr_fused.hip, the GNN planners): row
// degrees + fill (any N), the one-pass CSR + CSC builder (N <= 1024), and addGSO's in-place scrub on its own.
#include <cstdlib>

#include "magat_common.h"

// Dense GSO -> CSR edge structure (|S| > 1e-9), two calls: count (rowptr via caller-side prefix) is avoided by
// writing per-row degrees first.  deg [B*N] ints.
// edge rule of the reference: |S| > 1e-9 in S's dtype; rule 1 (GAT_origin) |float(S) + delta_ij| > 1e-9f; rule 2
// (GraphFilterBatch multiplies by the values): float(S) != 0
template <typename T>
__device__ __forceinline__ bool gso_edge(T v, bool diag, int self_loops) {
  if (self_loops == 2) return (float)v != 0.f;                          // GraphFilterBatch: every non-zero float(S)
  if (self_loops) return fabsf((float)v + (diag ? 1.f : 0.f)) > 1e-9f;
  return (v < 0 ? -v : v) > (T)1e-9;
}

template <typename T>
__global__ void gso_row_degree_kernel(const T* __restrict__ S, int* __restrict__ deg, int N, long long rows,
                                      int self_loops) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* r = S + row * N;
  const int i = (int)(row % N);
  int c = 0;
  for (int j = lane; j < N; j += 64) c += gso_edge(r[j], j == i, self_loops) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) deg[row] = c;
}
template <typename T>
__global__ void gso_fill_csr_kernel(const T* __restrict__ S, const int* __restrict__ rowstart,
                                    int* __restrict__ colidx, int N, long long rows, int self_loops) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* r = S + row * N;
  const int i = (int)(row % N);
  int base = rowstart[row];
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    bool f = false;
    if (j < N) f = gso_edge(r[j], j == i, self_loops);
    const unsigned long long m = __ballot(f);
    if (f) colidx[base + __popcll(m & ((1ull << lane) - 1ull))] = j;
    base += __popcll(m);
  }
}

extern "C" int magat_gso_row_degrees(const void* S, int s_is_f64, int self_loops, int* deg, int B, int N,
                                     void* stream) {
  if (!S || !deg) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0) return MAGAT_ERR_BAD_SHAPE;
  const long long rows = (long long)B * N;
  const unsigned blocks = (unsigned)((rows + 3) / 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (s_is_f64)
    hipLaunchKernelGGL(gso_row_degree_kernel<double>, dim3(blocks), dim3(256), 0, st, static_cast<const double*>(S),
                       deg, N, rows, self_loops);
  else
    hipLaunchKernelGGL(gso_row_degree_kernel<float>, dim3(blocks), dim3(256), 0, st, static_cast<const float*>(S), deg,
                       N, rows, self_loops);
  return magat_check_launch();
}

extern "C" int magat_gso_fill_csr(const void* S, int s_is_f64, int self_loops, const int* rowstart, int* colidx, int B,
                                  int N, void* stream) {
  if (!S || !rowstart || !colidx) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0) return MAGAT_ERR_BAD_SHAPE;
  const long long rows = (long long)B * N;
  const unsigned blocks = (unsigned)((rows + 3) / 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (s_is_f64)
    hipLaunchKernelGGL(gso_fill_csr_kernel<double>, dim3(blocks), dim3(256), 0, st, static_cast<const double*>(S),
                       rowstart, colidx, N, rows, self_loops);
  else
    hipLaunchKernelGGL(gso_fill_csr_kernel<float>, dim3(blocks), dim3(256), 0, st, static_cast<const float*>(S),
                       rowstart, colidx, N, rows, self_loops);
  return magat_check_launch();
}

namespace {
// ---- GSO -> CSR + CSC in ONE pass over the dense tensor (magat_gso_csr_build) ------------------------------------------
// The dense (B,N,N) GSO of a large instance is big (4 MB per instance at N = 1000): addGSO's in-place scrub, the edge test
// and the row degrees are one streaming read of it (written back only where a value changes), leaving a bit matrix
// (N^2/8 bytes per instance).  A second kernel - one workgroup per instance, a thread per row of the bit matrix - then produces
// everything the CSR kernels need, deterministically (no global atomics; LDS atomics only hand out slots whose order a rank
// placement undoes): rowptr / colidx (ascending j per row), cscptr,
// and per in-edge its source row and CSR position (ascending i per column).
constexpr int GSO_W64_MAX = 16;          // N <= 1024

template <typename T>
__global__ __launch_bounds__(256) void gso_mask_kernel(T* __restrict__ S, unsigned long long* __restrict__ masks,
                                                       int* __restrict__ inst_tot, int N, int W64, long long rows,
                                                       int scrub_nan, int gso_mode, int rule) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (row >= rows) return;
  // The row is READ through one pointer and (rarely: addGSO's scrub) WRITTEN through another the compiler cannot relate to it:
  // with the conditional write-back in the same loop as the loads of the same array, every load waited for the store in front
  // of it (the plain row-degree kernel streams the same bytes at 4.5 TB/s, this loop ran at 2.6).  A lane only ever re-writes
  // the element it has just read itself, so no ordering between the two is needed.
  const T* __restrict__ rl = S + row * N;
  T* rs = S + row * N;
  asm volatile("" : "+v"(rs));
  const int i = (int)(row % N);
  int cnt = 0;
  unsigned long long mine = 0ull;      // word `lane` of the row's bit mask: ONE 128-byte store per row behind the loop
  // GSO_MASK_BATCH 64-column steps per batch: the loads of a batch go out before the first value is looked at (one load -> wait
  // -> test per step left the latency to the occupancy alone)
#ifndef GSO_MASK_BATCH
#define GSO_MASK_BATCH 4
#endif
  for (int w0 = 0; w0 < W64; w0 += GSO_MASK_BATCH) {
    T xv[GSO_MASK_BATCH];
#pragma unroll
    for (int u = 0; u < GSO_MASK_BATCH; ++u) {
      const int j = (w0 + u) * 64 + lane;
      xv[u] = (w0 + u < W64 && j < N) ? rl[j] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < GSO_MASK_BATCH; ++u) {
      const int w = w0 + u, j = w * 64 + lane;
      bool f = false;
      if (w < W64 && j < N) {
        T x = xv[u];
        bool dirty = false;
        if (scrub_nan && x != x) { x = (T)0; dirty = true; }
        if (gso_mode == 1 && x > (T)0 && x != (T)1) { x = (T)1; dirty = true; }
        if (dirty) rs[j] = x;
        f = gso_edge(x, j == i, rule);
      }
      const unsigned long long m = __ballot(f);
      cnt += __popcll(m);
      if (lane == w) mine = m;
    }
  }
  if (lane < W64) masks[row * W64 + lane] = mine;
  if (lane == 0) inst_tot[row] = cnt;      // per-ROW degree (summed per instance by gso_totals_kernel: 128 k same-line atomics
}                                          // serialised on one L2 channel took 1 ms)

#ifndef MAGAT_GSO_X4
#define MAGAT_GSO_X4 1
#endif
// float rows with N % 4 == 0 (rows 16-byte aligned): every lane loads FOUR columns per request and all requests of the row
// (N <= 1024: four) go out before the first value is looked at - 16 KB in flight per wave instead of 1 KB per load of the
// scalar form, which left the pass at the latency x occupancy product (3.9 TB/s at config 5).  A lane's four edge flags are a
// nibble at bit 4 (lane % 16) of the 64-column word its 16-lane row covers: the word is the OR over the row (DPP).
__device__ __forceinline__ unsigned gso_dpp_or(unsigned v, const int ctrl_tag) {
  switch (ctrl_tag) {
    case 0: return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);     // quad_perm [1,0,3,2]
    case 1: return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);     // quad_perm [2,3,0,1]
    case 2: return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);    // row_ror:4
    default: return v | (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);   // row_ror:8
  }
}
__global__ __launch_bounds__(256) void gso_mask_x4_kernel(float* __restrict__ S, unsigned long long* __restrict__ masks,
                                                          int* __restrict__ inst_tot, int N, int W64, long long rows,
                                                          int scrub_nan, int gso_mode, int rule) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f32x4* __restrict__ rl = reinterpret_cast<const f32x4*>(S + row * N);
  float* rs = S + row * N;                       // (write-back pointer the compiler cannot relate to the loads: see below)
  asm volatile("" : "+v"(rs));
  const int i = (int)(row % N);
  f32x4 xv[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j0 = s * 256 + lane * 4;
    xv[s] = j0 < N ? rl[s * 64 + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  unsigned long long mine = 0ull;                // word `lane` of the row's bit mask (lanes 0..15)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j0 = s * 256 + lane * 4;
    unsigned nib = 0;
    if (j0 < N) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float x = xv[s][c];
        bool dirty = false;
        if (scrub_nan && x != x) { x = 0.f; dirty = true; }
        if (gso_mode == 1 && x > 0.f && x != 1.f) { x = 1.f; dirty = true; }
        if (dirty) rs[j0 + c] = x;
        nib |= gso_edge(x, j0 + c == i, rule) ? (1u << c) : 0u;
      }
    }
    const int sh = 4 * (lane & 15);
    unsigned lo = sh < 32 ? nib << sh : 0u, hi = sh >= 32 ? nib << (sh - 32) : 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) { lo = gso_dpp_or(lo, t); hi = gso_dpp_or(hi, t); }
    // every lane of row q = lane / 16 now holds word 4 s + q; lane w < 16 keeps word w: from row w % 4 when w / 4 == s
    const int srcl = 16 * (lane & 3);
    const unsigned glo = (unsigned)__shfl((int)lo, srcl, 64), ghi = (unsigned)__shfl((int)hi, srcl, 64);
    if ((lane >> 2) == s) mine = ((unsigned long long)ghi << 32) | glo;
  }
  int cnt = lane < 16 ? __popcll(mine) : 0;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane < W64) masks[row * W64 + lane] = mine;
  if (lane == 0) inst_tot[row] = cnt;
}

// edge total of every instance: one workgroup per instance over its N row degrees
__global__ __launch_bounds__(256) void gso_totals_kernel(const int* __restrict__ rowdeg, int* __restrict__ inst_tot, int N) {
  __shared__ int part[4];
  const int b = blockIdx.x, t = threadIdx.x;
  int s = 0;
  for (int i = t; i < N; i += 256) s += rowdeg[(size_t)b * N + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  if (t == 0) inst_tot[b] = part[0] + part[1] + part[2] + part[3];
}

// One workgroup per instance.  Round 5: every phase walks the EDGES - a thread per row over the set bits of ITS row, which it
// holds in registers (16 words; the round-2 kernel kept the whole bit matrix in LDS and counted / filled the columns with a
// thread per column walking all N rows twice: 150-183 us per launch at config 5 with half of the chip's CUs, one per instance,
// tied up beside the encoder for that long).  Column degrees are LDS atomics, an in-edge takes its slot in its column's list
// from an LDS cursor, each column's short list is then sorted by source row (registers), which makes the result the same
// deterministic arrays as before (ascending i per column; ascending j per row comes with the bit order).  The three edge
// arrays are STAGED in LDS (the bit matrix no longer lives there) and leave as whole contiguous runs: written edge by edge,
// the scattered 4-byte stores alone took 70 us.  An instance with more edges than the stage holds writes and sorts through
// global memory instead (reads at agent scope: the entries come from other threads of the workgroup).
// Round 6: the cost per column is BOUNDED whatever the topology.  Staged path: a thread ranks its column's list
// itself only up to GSO_SELF_SORT entries; longer lists (hub columns) are ranked by the whole workgroup, one entry per thread
// (at most stage / 1024 = 12 steps of <= 1024 LDS reads each).  An instance with more edges than the stage holds no longer
// sorts anything: the stage region holds the TRANSPOSED bit matrix instead (LDS atomic ORs, N x N bits = 128 KB at N = 1024),
// and an in-edge's slot is its rank = the set bits of its column below its source row (<= 32 word popcounts) - the arrays are
// written once, in their final order, without a global-memory atomic or a read-back (was: an O(deg^2) selection sort of
// agent-scope loads per column, ~500 k L2 round trips per thread on a dense N = 1000 instance).
constexpr int GSO_SELF_SORT = 32;
constexpr int GSO_STAGE_EDGES = 12 * 1024;      // edges of one instance the LDS stage holds (3 x 4 bytes each: 144 KB; < 2^14)
__global__ __launch_bounds__(1024) void gso_structure_kernel(const unsigned long long* __restrict__ masks,
                                                             int* __restrict__ inst_tot, int* __restrict__ rowptr,
                                                             int* colidx, int* __restrict__ cscptr, int* cscsrc, int* cscpos,
                                                             long long cap, long long* __restrict__ nnz_out, int B, int N,
                                                             int W64, int stage_edges) {
  extern __shared__ __align__(16) int gsi[];
  int* ccnt = gsi;                    // [N] column degrees, then the fill cursors
  int* coff = ccnt + 1024;            // [N] exclusive column offsets (local)
  int* stage = coff + 1024;           // [3][stage_edges]: column of CSR position q | in-edge of slot k as (source row << 14 |
                                      // local CSR position), in arrival order | the same, every column's list sorted
                                      // (stage_edges = min(GSO_STAGE_EDGES, N * N): small graphs ask for little LDS)
  __shared__ int part[17];
  __shared__ int nbig, big[GSO_STAGE_EDGES / GSO_SELF_SORT];      // columns with more than GSO_SELF_SORT in-edges (staged path)
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // absolute offset of this instance = edges of all earlier instances (inst_tot was accumulated by the mask pass)
  int before = 0;
  for (int q = t; q < b; q += 1024) before += inst_tot[q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  if (lane == 0) part[wave] = before;
  // this thread's row of the bit matrix
  unsigned long long mrow[GSO_W64_MAX];
  {
    const unsigned long long* src = masks + ((size_t)b * N + (t < N ? t : 0)) * W64;
#pragma unroll
    for (int w = 0; w < GSO_W64_MAX; ++w) mrow[w] = (t < N && w < W64) ? src[w] : 0ull;
  }
  ccnt[t] = 0;
  if (t == 0) nbig = 0;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < 16; ++w) base += part[w];
  __syncthreads();
  // block-wide exclusive scan helper over up to 1024 values (one per thread)
  auto block_scan = [&](int v, int* out_total) -> int {
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; ++w) wbase += part[w];
    int tot = 0;
    for (int w = 0; w < 16; ++w) tot += part[w];
    __syncthreads();
    *out_total = tot;
    return wbase + inc - v;
  };
  // rows: degrees -> offsets; columns: one LDS atomic per edge
  int rdeg = 0;
#pragma unroll
  for (int w = 0; w < GSO_W64_MAX; ++w) {
    unsigned long long m = mrow[w];
    rdeg += __popcll(m);
    while (m) {
      const int bit = __builtin_ctzll(m);
      m &= m - 1;
      atomicAdd(&ccnt[w * 64 + bit], 1);
    }
  }
  int total = 0;
  const int rex = block_scan(rdeg, &total);      // (its barriers also order the atomics above in front of the reads below)
  const int cdeg = t < N ? ccnt[t] : 0;
  int total2 = 0;
  const int cex = block_scan(cdeg, &total2);
  coff[t] = cex;
  ccnt[t] = 0;
  __syncthreads();
  int* rp = rowptr + (size_t)b * (N + 1);
  int* cp = cscptr + (size_t)b * (N + 1);
  if (t < N) {
    rp[t] = base + rex;
    cp[t] = base + cex;
  }
  if (t == 0) {
    rp[N] = base + total;
    cp[N] = base + total;
  }
  if (b == B - 1 && t == 0 && nnz_out) *nnz_out = (long long)base + total;
  const bool staged = total <= stage_edges;
  if (staged) {
    int* const scol = stage;
    int* const sin = stage + stage_edges;
    int* const sout = stage + 2 * stage_edges;
    // a thread per row over its edges in ascending j: the column index of every CSR position, and the in-edge into the next
    // free slot of column j's list
    {
      int pos = rex;
#pragma unroll
      for (int w = 0; w < GSO_W64_MAX; ++w) {
        unsigned long long m = mrow[w];
        while (m) {
          const int bit = __builtin_ctzll(m);
          m &= m - 1;
          const int j = w * 64 + bit;
          scol[pos] = j;
          sin[coff[j] + atomicAdd(&ccnt[j], 1)] = (t << 14) | pos;
          ++pos;
        }
      }
    }
    __syncthreads();
    // a thread per column: its list ordered by source row - every entry goes to the slot its rank names (the lists are short:
    // 3-5 entries at config 5); a hub column is left to the whole workgroup
    if (t < N) {
      if (cdeg <= GSO_SELF_SORT) {
        for (int e = 0; e < cdeg; ++e) {
          const int w = sin[cex + e];
          int rank = 0;
          for (int f = 0; f < cdeg; ++f) rank += sin[cex + f] < w ? 1 : 0;
          sout[cex + rank] = w;
        }
      } else {
        big[atomicAdd(&nbig, 1)] = t;
      }
    }
    __syncthreads();
    for (int q = 0, nb = nbig; q < nb; ++q) {      // (the list's order is whatever the atomics made it: the result does not know)
      const int j = big[q], cx = coff[j], cd = ccnt[j];
      for (int e = t; e < cd; e += 1024) {
        const int w = sin[cx + e];
        int rank = 0;
        for (int f = 0; f < cd; ++f) rank += sin[cx + f] < w ? 1 : 0;
        sout[cx + rank] = w;
      }
    }
    __syncthreads();
    // the stage leaves as three contiguous runs
    const long long lim = cap - base < total ? cap - base : total;
    for (int q = t; q < lim; q += 1024) {
      const int w = sout[q];
      colidx[base + q] = scol[q];
      cscsrc[base + q] = w >> 14;
      cscpos[base + q] = base + (w & 16383);
    }
  } else {
    // more edges than the stage holds: the stage region takes the transposed bit matrix, an in-edge's slot is its rank
    const int W32 = (N + 31) >> 5;
    unsigned* const colm = reinterpret_cast<unsigned*>(stage);      // [N][W32] bit i of column j's words <=> edge (i -> j)
    for (int q = t; q < N * W32; q += 1024) colm[q] = 0u;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < GSO_W64_MAX; ++w) {
      unsigned long long m = mrow[w];
      while (m) {
        const int bit = __builtin_ctzll(m);
        m &= m - 1;
        atomicOr(&colm[(w * 64 + bit) * W32 + (t >> 5)], 1u << (t & 31));
      }
    }
    __syncthreads();
    {
      int pos = base + rex;
#pragma unroll
      for (int w = 0; w < GSO_W64_MAX; ++w) {
        unsigned long long m = mrow[w];
        while (m) {
          const int bit = __builtin_ctzll(m);
          m &= m - 1;
          const int j = w * 64 + bit;
          if (pos < cap) colidx[pos] = j;
          const unsigned* cw = colm + j * W32;
          int rank = __popc(cw[t >> 5] & ((1u << (t & 31)) - 1u));
          for (int v = 0; v < (t >> 5); ++v) rank += __popc(cw[v]);
          const long long k = (long long)base + coff[j] + rank;
          if (k < cap) {
            cscsrc[k] = t;
            cscpos[k] = pos;
          }
          ++pos;
        }
      }
    }
  }
  // leave inst_tot clear for the next build (every workgroup has read what it needs only after ALL of them pass this
  // point is not guaranteed - so the clearing is done by the NEXT build's memset, see the host code)
}

}  // namespace

extern "C" size_t magat_gso_csr_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0 || N > 64 * GSO_W64_MAX) return 0;
  const size_t w64 = (size_t)(N + 63) / 64;
  return magat_align_up((size_t)B * N * w64 * 8, 256) + magat_align_up((size_t)B * sizeof(int), 256) +
         magat_align_up((size_t)B * N * sizeof(int), 256);
}

extern "C" int magat_gso_csr_build_phase(void* S, int s_is_f64, int scrub_nan, int gso_mode, int edge_rule, int* rowptr,
                                         int* colidx, int* cscptr, int* cscsrc, int* cscpos, long long cap,
                                         long long* nnz_dev, void* workspace, size_t workspace_bytes, int B, int N,
                                         int phase, void* stream) {
  if (!S || !rowptr || !colidx || !cscptr || !cscsrc || !cscpos) return MAGAT_ERR_NULL;
  if (phase < 0 || phase > 2) return MAGAT_ERR_BAD_SHAPE;
  if (B <= 0 || N <= 0 || cap < 0 || edge_rule < 0 || edge_rule > 2 || gso_mode < 0 || gso_mode > 1)
    return MAGAT_ERR_BAD_SHAPE;
  const size_t need = magat_gso_csr_workspace_bytes(B, N);
  if (!need) return MAGAT_ERR_UNSUPPORTED;                      // N > 1024: magat_gso_row_degrees / magat_gso_fill_csr
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) || workspace_bytes < need) return MAGAT_ERR_WORKSPACE;
  const int W64 = (N + 63) / 64;
  // column counters / offsets + the edge stage, sized by the graph (a small N asks for little LDS: several instances per CU);
  // the stage must also hold the transposed bit matrix of an instance with more edges than it stages (N > 110 only)
  const long long nn = (long long)N * N;
  const int stage_edges = (int)(nn < GSO_STAGE_EDGES ? nn : GSO_STAGE_EDGES);
  size_t stage_ints = (size_t)3 * stage_edges;
  if (nn > GSO_STAGE_EDGES && (size_t)N * ((N + 31) / 32) > stage_ints) stage_ints = (size_t)N * ((N + 31) / 32);
  const size_t lds = (size_t)(2 * 1024 + stage_ints) * sizeof(int);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* masks = static_cast<unsigned long long*>(workspace);
  int* inst_tot = reinterpret_cast<int*>(static_cast<char*>(workspace) + magat_align_up((size_t)B * N * W64 * 8, 256));
  int* rowdeg = reinterpret_cast<int*>(reinterpret_cast<char*>(inst_tot) + magat_align_up((size_t)B * sizeof(int), 256));
  const long long rows = (long long)B * N;
  const int pid = magat_prof_begin(MAGAT_TAG_GSO_CSR, st);
  if (phase != 2) {
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    if (s_is_f64)
      hipLaunchKernelGGL(gso_mask_kernel<double>, dim3(blocks), dim3(256), 0, st, static_cast<double*>(S), masks, rowdeg,
                         N, W64, rows, scrub_nan, gso_mode, edge_rule);
    else if (MAGAT_GSO_X4 && N % 4 == 0 && !(reinterpret_cast<uintptr_t>(S) & 15))
      hipLaunchKernelGGL(gso_mask_x4_kernel, dim3(blocks), dim3(256), 0, st, static_cast<float*>(S), masks, rowdeg, N, W64,
                         rows, scrub_nan, gso_mode, edge_rule);
    else
      hipLaunchKernelGGL(gso_mask_kernel<float>, dim3(blocks), dim3(256), 0, st, static_cast<float*>(S), masks, rowdeg, N,
                         W64, rows, scrub_nan, gso_mode, edge_rule);
    hipLaunchKernelGGL(gso_totals_kernel, dim3(B), dim3(256), 0, st, rowdeg, inst_tot, N);
  }
  if (phase != 1) {
    if (magat_ensure_dyn_lds(reinterpret_cast<const void*>(&gso_structure_kernel), MAGAT_LDS_GSO_STRUCT, lds) != MAGAT_OK)
      return MAGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(gso_structure_kernel, dim3(B), dim3(1024), lds, st, masks, inst_tot, rowptr, colidx, cscptr, cscsrc,
                       cscpos, cap, nnz_dev, B, N, W64, stage_edges);
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_gso_csr_build(void* S, int s_is_f64, int scrub_nan, int gso_mode, int edge_rule, int* rowptr,
                                   int* colidx, int* cscptr, int* cscsrc, int* cscpos, long long cap, long long* nnz_dev,
                                   void* workspace, size_t workspace_bytes, int B, int N, void* stream) {
  return magat_gso_csr_build_phase(S, s_is_f64, scrub_nan, gso_mode, edge_rule, rowptr, colidx, cscptr, cscsrc, cscpos, cap,
                                   nnz_dev, workspace, workspace_bytes, B, N, 0, stream);
}

// addGSO's in-place scrub (decentralplanner_GAT_bottleneck.py:272-277)
template <typename T>
__global__ void gso_prepare_kernel(T* S, size_t count, int scrub_nan, int gso_mode) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    T v = S[i];
    if (scrub_nan && v != v) v = (T)0;
    if (gso_mode == 1 && v > (T)0) v = (T)1;
    if (gso_mode == 2) v = (T)1;
    S[i] = v;
  }
}

extern "C" int magat_gso_prepare(void* S, int s_is_f64, size_t count, int scrub_nan, int gso_mode, void* stream) {
  if (!S) return MAGAT_ERR_NULL;
  if (count == 0) return MAGAT_OK;
  size_t blocks = (count + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (s_is_f64)
    hipLaunchKernelGGL(gso_prepare_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st,
                       static_cast<double*>(S), count, scrub_nan, gso_mode);
  else
    hipLaunchKernelGGL(gso_prepare_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st,
                       static_cast<float*>(S), count, scrub_nan, gso_mode);
  return magat_check_launch();
}
