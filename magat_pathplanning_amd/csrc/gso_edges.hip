// Agent positions (B, N, 2) -> the communication graph as the edge structure the CSR kernels take (gat_csr_f32.hip,
// gat_csr_fused.hip): the arrays of magat_gso_csr_build (gso_csr.hip), without the dense GSO in between.  The attention layers
// read the GSO through its edge test only; the simulator's GSO (sim_frontend.hip) is a function of the positions - so the bit
// matrix both sides care about (N * N / 8 bytes per instance) is made straight from the distance test, N <= 4096.
//
// Two launches, no host synchronisation, no global atomics (the arrays are the same on every call):
//   1. edges_mask_kernel  - an instance's positions in LDS; a wave takes a row, a lane a column, one ballot gives the 64 columns'
//                           word.  Leaves the bit matrix, per word the number of set bits in front of it in its row, the row
//                           degrees, and the edge total of every chunk of rows (one workgroup = one chunk of one instance).
//   2. edges_fill_kernel  - the offset of the instance (totals of the chunks in front), the row scan, and per row the column
//                           indices by bit position.  The graph is symmetric, so the column view is the row view: cscptr =
//                           rowptr, cscsrc = colidx, and the CSR position of the in-edge i -> j is rowptr[i] + the set bits of
//                           row i below j = the stored prefix of j's word + one masked popcount.
// An instance is spread over ceil(N / rows per chunk) workgroups; a small batch takes 16 rows per chunk instead of 64, so that
// one instance of 4096 agents (16.7 M pair tests) still fills the chip.
#include "magat_common.h"
#include "sim_connect.h"

namespace {
constexpr int EDGES_N_MAX = 4096;       // 64 words of 64 columns: a lane per word
constexpr int EDGES_THREADS = 256;      // four waves

struct EdgesCell { int x, y; };

struct EdgesGeom {
  int W64, rpw, chunks;                 // words per row, rows per workgroup, workgroups per instance
  size_t off_pre, off_deg, off_tot, bytes;
};

EdgesGeom edges_geom(int B, int N) {
  EdgesGeom g;
  g.W64 = (N + 63) / 64;
  g.rpw = (long long)B * g.W64 < 512 ? 16 : 64;
  g.chunks = (N + g.rpw - 1) / g.rpw;
  const size_t words = (size_t)B * N * g.W64;
  g.off_pre = magat_align_up(words * 8, 256);                                       // bit matrix: u64 [B][N][W64]
  g.off_deg = g.off_pre + magat_align_up(words * 2, 256);                           // set bits in front of a word: u16 [B][N][W64]
  g.off_tot = g.off_deg + magat_align_up((size_t)B * N * sizeof(int), 256);         // row degrees: int [B][N]
  g.bytes = g.off_tot + magat_align_up((size_t)B * g.chunks * sizeof(int), 256);    // chunk totals: int [B][chunks]
  return g;
}

// squared distance < bound, for coordinates anywhere in int32 (the sum may pass 2^64: then nothing is closer)
__device__ __forceinline__ bool edges_close_wide(int xi, int yi, int xj, int yj, long long bound) {
  const long long dx = (long long)xi - xj, dy = (long long)yi - yj;
  const unsigned long long ax = (unsigned long long)(dx < 0 ? -dx : dx), ay = (unsigned long long)(dy < 0 ? -dy : dy);
  const unsigned long long sx = ax * ax, d2 = sx + ay * ay;
  return d2 >= sx && d2 < (unsigned long long)bound;
}

__global__ __launch_bounds__(EDGES_THREADS) void edges_mask_kernel(const int32_t* __restrict__ pos,
                                                                   const double* __restrict__ radii, double comm_radius,
                                                                   int rule, unsigned long long* __restrict__ masks,
                                                                   uint16_t* __restrict__ pre, int* __restrict__ rowdeg,
                                                                   int* __restrict__ chunk_tot, int N, int W64, int rpw,
                                                                   int chunks) {
  HIP_DYNAMIC_SHARED(unsigned long long, lds)      // the instance's cells [N]
  EdgesCell* cell = reinterpret_cast<EdgesCell*>(lds);
  __shared__ int wsum[4];
  __shared__ unsigned far_cells;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  if (t == 0) far_cells = 0u;
  __syncthreads();
  const int32_t* p = pos + (size_t)b * N * 2;
  bool far = false;
  for (int n = t; n < N; n += EDGES_THREADS) {
    const int x = p[2 * n], y = p[2 * n + 1];
    cell[n].x = x;
    cell[n].y = y;
    far = far || x < -16384 || x > 16383 || y < -16384 || y > 16383;
  }
  if (far) atomicOr(&far_cells, 1u);
  __syncthreads();
  // the reference's float64 test sqrt(d^2) < r as one integer bound per radius (sim_connect.h).  Cells within +-16383 (every
  // map the simulator takes): offsets below 2^15, squared distances below 2^31 - the test in 32-bit arithmetic.
  const long long bound = sim_dist2_bound(radii ? radii[b] : comm_radius);
  const bool narrow = far_cells == 0u;
  const int bound32 = bound > 0x7fffffffLL ? 0x7fffffff : (int)bound;
  const int row_end = (c + 1) * rpw < N ? (c + 1) * rpw : N;
  int wave_edges = 0;
  for (int i = c * rpw + wave; i < row_end; i += 4) {
    const int xi = cell[i].x, yi = cell[i].y;
    unsigned long long mine = 0ull;      // word `lane` of the row: one contiguous store per row behind the loop
    int mine_pre = 0, cnt = 0;
    for (int w = 0; w < W64; ++w) {
      const int j = w * 64 + lane;
      bool f = false;
      if (j < N) {
        const int xj = cell[j].x, yj = cell[j].y;
        if (j == i) {
          f = rule != 0;
        } else if (narrow) {
          const int dx = xi - xj, dy = yi - yj;
          f = dx * dx + dy * dy < bound32;
        } else {
          f = edges_close_wide(xi, yi, xj, yj, bound);
        }
      }
      const unsigned long long m = __ballot(f);
      if (lane == w) {
        mine = m;
        mine_pre = cnt;
      }
      cnt += __popcll(m);
    }
    const size_t row = (size_t)b * N + i;
    if (lane < W64) {
      masks[row * W64 + lane] = mine;
      pre[row * W64 + lane] = (uint16_t)mine_pre;
    }
    if (lane == 0) rowdeg[row] = cnt;
    wave_edges += cnt;
  }
  if (lane == 0) wsum[wave] = wave_edges;
  __syncthreads();
  if (t == 0) chunk_tot[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(EDGES_THREADS) void edges_fill_kernel(const unsigned long long* __restrict__ masks,
                                                                   const uint16_t* __restrict__ pre,
                                                                   const int* __restrict__ rowdeg,
                                                                   const int* __restrict__ chunk_tot, int* __restrict__ rowptr,
                                                                   int* colidx, int* __restrict__ cscptr, int* cscsrc, int* cscpos,
                                                                   long long cap, long long* __restrict__ nnz_out, int B, int N,
                                                                   int W64, int rpw, int chunks) {
  HIP_DYNAMIC_SHARED(unsigned long long, lds)      // the instance's row offsets [N + 1], without the instances in front
  int* rp = reinterpret_cast<int*>(lds);
  __shared__ long long red[EDGES_THREADS];
  __shared__ int part[EDGES_THREADS];
  __shared__ int wtot[4];
  __shared__ unsigned long long wrow[4][64];       // a wave's current row of the bit matrix
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  // edges of all earlier instances
  long long s = 0;
  for (int k = t; k < b * chunks; k += EDGES_THREADS) s += chunk_tot[k];
  red[t] = s;
  __syncthreads();
  for (int h = EDGES_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const long long base = red[0];
  // exclusive scan of the instance's row degrees: a thread takes T consecutive rows
  const int T = (N + EDGES_THREADS - 1) / EDGES_THREADS;
  const int i0 = t * T;
  const int* deg = rowdeg + (size_t)b * N;
  int mine_sum = 0;
  for (int e = 0; e < T; ++e) mine_sum += i0 + e < N ? deg[i0 + e] : 0;
  part[t] = mine_sum;
  __syncthreads();
  int before = 0;
  for (int u = wave * 64; u < t; ++u) before += part[u];
  if (lane == 63) wtot[wave] = before + mine_sum;
  __syncthreads();
  for (int w = 0; w < wave; ++w) before += wtot[w];
  const int total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  for (int e = 0; e < T; ++e) {
    if (i0 + e < N) {
      rp[i0 + e] = before;
      before += deg[i0 + e];
    }
  }
  if (t == 0) rp[N] = total;
  __syncthreads();
  const int r0 = c * rpw, r1 = r0 + rpw < N ? r0 + rpw : N;
  int* rpo = rowptr + (size_t)b * (N + 1);
  int* cpo = cscptr + (size_t)b * (N + 1);
  for (int i = r0 + t; i < r1; i += EDGES_THREADS) {
    const int v = (int)(base + rp[i]);
    rpo[i] = v;
    cpo[i] = v;
  }
  if (c == chunks - 1 && t == 0) {
    const int v = (int)(base + total);
    rpo[N] = v;
    cpo[N] = v;
    if (b == B - 1) *nnz_out = base + total;
  }
  // a wave per row j, a lane per column of the current word: CSR position k of the edge j -> i holds i (as column, and as the
  // source of the in-edge i -> j of column j's list, ascending i) and where that in-edge stands in row i
  for (int j = r0 + wave; j < r1; j += 4) {
    const size_t row = (size_t)b * N + j;
    const unsigned long long mine = lane < W64 ? masks[row * W64 + lane] : 0ull;
    wrow[wave][lane] = mine;
    unsigned long long words = __ballot(mine != 0ull);      // the row's non-empty words
    __builtin_amdgcn_wave_barrier();
    long long at = base + rp[j];
    const int jw = j >> 6;
    const unsigned long long jlow = (1ull << (j & 63)) - 1ull;
    while (words) {
      const int w = __builtin_ctzll(words);
      words &= words - 1ull;
      const unsigned long long m = wrow[wave][w];
      if ((m >> lane) & 1ull) {
        const long long k = at + __popcll(m & ((1ull << lane) - 1ull));
        if (k < cap) {
          const int i = w * 64 + lane;
          const size_t wi = ((size_t)b * N + i) * W64 + jw;
          colidx[k] = i;
          cscsrc[k] = i;
          cscpos[k] = (int)(base + rp[i] + pre[wi] + __popcll(masks[wi] & jlow));
        }
      }
      at += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();      // (the next row's words go into the same LDS row)
  }
}

}  // namespace

extern "C" size_t magat_gso_edges_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0 || N > EDGES_N_MAX) return 0;
  return edges_geom(B, N).bytes;
}

extern "C" int magat_gso_edges_build(const int32_t* pos, const double* radii, double comm_radius, int edge_rule, int* rowptr,
                                     int* colidx, int* cscptr, int* cscsrc, int* cscpos, long long cap, long long* nnz_dev,
                                     void* workspace, size_t workspace_bytes, int B, int N, void* stream) {
  if (!pos || !rowptr || !cscptr || !nnz_dev) return MAGAT_ERR_NULL;
  if ((!colidx || !cscsrc || !cscpos) && cap != 0) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || cap < 0 || edge_rule < 0 || edge_rule > 1 || (!radii && !(comm_radius > 0.0))) return MAGAT_ERR_BAD_SHAPE;
  const size_t need = magat_gso_edges_workspace_bytes(B, N);
  if (!need) return MAGAT_ERR_UNSUPPORTED;                      // N > 4096
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255) || workspace_bytes < need) return MAGAT_ERR_WORKSPACE;
  const EdgesGeom g = edges_geom(B, N);
  if ((long long)B * g.chunks > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* masks = reinterpret_cast<unsigned long long*>(ws);
  uint16_t* pre = reinterpret_cast<uint16_t*>(ws + g.off_pre);
  int* rowdeg = reinterpret_cast<int*>(ws + g.off_deg);
  int* chunk_tot = reinterpret_cast<int*>(ws + g.off_tot);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)B * (unsigned)g.chunks;
  magat_form_note(MAGAT_FORM_GSO_EDGES);
  const int pid = magat_prof_begin(MAGAT_TAG_GSO_EDGES, st);
  hipLaunchKernelGGL(edges_mask_kernel, dim3(grid), dim3(EDGES_THREADS), (size_t)N * sizeof(EdgesCell), st, pos, radii, comm_radius,
                     edge_rule, masks, pre, rowdeg, chunk_tot, N, g.W64, g.rpw, g.chunks);
  hipLaunchKernelGGL(edges_fill_kernel, dim3(grid), dim3(EDGES_THREADS), (size_t)(N + 2) / 2 * 8, st, masks, pre, rowdeg, chunk_tot,
                     rowptr, colidx, cscptr, cscsrc, cscpos, cap, nnz_dev, B, N, g.W64, g.rpw, g.chunks);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
