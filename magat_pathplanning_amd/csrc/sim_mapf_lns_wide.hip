// The wide form of the schedule improver of sim_mapf_lns.hip: the same neighbourhood re-planning rule, cell for cell (DESIGN
// 4.11; restated in tests/lns_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_improve_wide_workspace_bytes   per case: the layers, T * 6 * rows * words * 8 bytes, and d0, one int per agent
//   magat_sim_mapf_improve_wide                   one workgroup per case runs every iteration; one launch, no host round trip
// The layout of wmapf_plan_kernel (sim_mapf_wide.hip): `rows` threads, thread = map row, `words` 64-bit words per row in
// registers, the five reservation boards and the R layer of every t in the workspace (the boards zeroed here), votes and counts
// across the wavefronts through the LDS mail (row_board.h); search and backtrace are the wide solver's own
// (sim_mapf_wide_parts.h), with the board loads compiled out for a free path.  Per case, the rule of sim_mapf_lns.hip:
//   screening      threads over t; the free rows of the map in LDS for the threads that are not the cell's row.
//   set-up         all N paths reserved, threads over t: layer t belongs to one thread; d0[a] behind the layers.
//   iteration i    the seed by counting, threads over agents in chunks of `rows`: a ballot per wave, the waves' counts summed
//                  through the mail - a bisection over the delay, then the index inside the class (a thread's place is the
//                  count of the chunks and waves in front of it plus the bits below it in its wave's ballot).  The in-the-way
//                  scan along the seed's free path likewise: newcomers take the places behind the list in index order across
//                  waves and chunks, at most k.  The OLD paths of the neighbourhood are read from `paths` - the global rows
//                  are overwritten only on accept -, the NEW ones staged in LDS (8 paths of 1024 cells).
// All control flow around a barrier is uniform over the workgroup: every condition on it is a value read from one address by
// all threads or comes out of the mail.  Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_wide_parts.h"      // WMAPF_*, wide_rows / wide_words, wide_layers, wmapf_search, wmapf_backtrace

namespace {

constexpr int WLNS_MAX_K = 8;
constexpr int WLNS_MAX_ITERATIONS = 4096;

__host__ __device__ inline long long wlns_layer_words(int rows, int words) { return (long long)WMAPF_BOARDS * rows * words; }
__host__ __device__ inline long long wlns_case_words(int rows, int words, int N, int T) {      // layers, then d0 padded to whole words
  return (long long)T * wlns_layer_words(rows, words) + ((long long)N + 1) / 2;
}

// Reserves (SET) or un-reserves one path, threads over t: layer t belongs to one thread, so no two threads touch one word.
// cell(t), 0 <= t < len: the path's cell (row << 8 | col).  V[t] along the path and at its last cell behind it, A_d[t] at the
// entered cell of a real move.
template <bool SET, int NW, typename F>
__device__ void wlns_mark(const wide_layers<NW>& L, F cell, int len, int T, int tid, int nt) {
  for (int t = tid; t < T; t += nt) {
    const int at = cell(t < len ? t : len - 1), cr = at >> 8, cc = at & 255;
    u64* v = L.at(t, 0, cr) + (cc >> 6);
    if (SET) *v |= 1ull << (cc & 63);
    else *v &= ~(1ull << (cc & 63));
    if (t >= 1 && t < len) {
      const int from = cell(t - 1), dr = cr - (from >> 8), dc = cc - (from & 255);
      const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : dc == 1 ? 3 : 4;
      if (d < 4) {
        u64* a = L.at(t, 1 + d, cr) + (cc >> 6);
        if (SET) *a |= 1ull << (cc & 63);
        else *a &= ~(1ull << (cc & 63));
      }
    }
  }
}

// a global path row as cells, and a staged one
struct wlns_row {
  const int* p;
  __device__ __forceinline__ int operator()(int t) const { return p[2 * t] << 8 | p[2 * t + 1]; }
};
struct wlns_staged {
  const int* cells;
  __device__ __forceinline__ int operator()(int t) const { return cells[t]; }
};

// how many agents have delay = length - d0 >= x (the same for every thread; one round of the mail)
__device__ int wlns_count_ge(wide_seat& s, const int* len, const int* d0, int N, int x, int tid, int nt) {
  int cnt = 0;
  for (int base = 0; base < N; base += nt) {
    const int b = base + tid;
    cnt += __popcll(__builtin_amdgcn_ballot_w64(b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] >= x));
  }
  wide_post(s, 0, cnt);
  return wide_sum(s, wide_sync(s), 0);
}

template <int NW>
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_lns_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                              const uint8_t* __restrict__ solved, int* paths, int* lengths,
                                                              int* makespan, int* __restrict__ flow_before,
                                                              int* __restrict__ flow_after, int* __restrict__ accepted,
                                                              int* __restrict__ status, u64* workspace, int N, int T, int iterations,
                                                              int K) {
  __shared__ wide_mail mail;
  __shared__ u64 free_rows[WIDE_SIDE][NW];      // the free cells, for the threads that are not the cell's row
  __shared__ int cells[WMAPF_MAX_T];            // set-up: the path being reserved
  __shared__ int fcells[WMAPF_MAX_T];           // the seed's free path
  __shared__ int new_cells[WLNS_MAX_K][WMAPF_MAX_T];      // the stage: the re-planned paths
  __shared__ int nb[WLNS_MAX_K], old_len[WLNS_MAX_K], new_len[WLNS_MAX_K];
  __shared__ int seed_found;
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = rows
  wide_seat s{&mail, tid & 63, tid >> 6, nt >> 6, 0};
  const long long layer_words = wlns_layer_words(nt, NW);
  u64* mine = workspace + (long long)cs * wlns_case_words(nt, NW, N, T);
  const wide_layers<NW> L{mine, nt};
  int* d0 = reinterpret_cast<int*>(mine + (long long)T * layer_words);
  const long long a0 = (long long)cs * N;
  int* len = lengths + a0;
  int* rows = paths + a0 * T * 2;      // agent a's row: rows + a * T * 2
  if (tid == 0) {
    flow_before[cs] = 0;
    flow_after[cs] = 0;
    accepted[cs] = 0;
  }
  if (solved[cs] == 0) {
    if (tid == 0) status[cs] = 1;
    return;
  }
  // free cells: the rows of this wave, each read by the lanes over its columns, one ballot per word; rows >= H and bits >= W
  // stay zero
  const uint8_t* mp = map + cs * map_stride;
  wboard<NW> free = wb_zero<NW>();
  for (int r = 64 * s.wave; r < H && r < 64 * s.wave + 64; ++r) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int col = 64 * k + s.lane;
      const u64 word = __builtin_amdgcn_ballot_w64(col < W && mp[r * W + (col < W ? col : 0)] == 0);
      if (tid == r) free.w[k] = word;
    }
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) free_rows[tid][k] = free.w[k];
  __syncthreads();
  // screening, threads over t
  bool bad = false;
  for (int a = 0; a < N; ++a) {
    const int la = len[a];
    bad |= la < 1 || la > T;
    const int* p = rows + (long long)a * T * 2;
    for (int t = tid; t < T; t += nt) {
      const int r = p[2 * t], c = p[2 * t + 1];
      const bool inside = r >= 0 && r < H && c >= 0 && c < W;
      bad |= !inside || !has_bit(free_rows[inside ? r : 0][inside ? c >> 6 : 0], inside ? c & 63 : 0);
      if (t >= 1 && inside) {
        const int pr = p[2 * t - 2], pc = p[2 * t - 1];
        const bool pin = pr >= 0 && pr < H && pc >= 0 && pc < W;      // (a cell outside is refused by its own thread)
        const int dr = pin ? r - pr : 0, dc = pin ? c - pc : 0;
        bad |= !((dr == 0 && dc >= -1 && dc <= 1) || (dc == 0 && dr >= -1 && dr <= 1));
      }
    }
  }
  wide_post(s, 0, (int)wave_any(bad));
  if (wide_or(s, wide_sync(s), 0)) {
    if (tid == 0) status[cs] = 2;
    return;
  }
  // set-up: every path reserved, d0 of every agent, the flowtime
  for (int t = 0; t < T; ++t)      // the reservation boards; an R layer is written before it is read
    for (int i = tid; i < 5 * nt * NW; i += nt) mine[t * layer_words + i] = 0ull;
  __syncthreads();
  int flow = 0;
  for (int a = 0; a < N; ++a) {
    const int la = __builtin_amdgcn_readfirstlane(len[a]);
    const wlns_row row{rows + (long long)a * T * 2};
    for (int t = tid; t < la; t += nt) cells[t] = row(t);
    __syncthreads();
    wlns_mark<true>(L, wlns_staged{cells}, la, T, tid, nt);
    const int st = __builtin_amdgcn_readfirstlane(cells[0]), g = __builtin_amdgcn_readfirstlane(cells[la - 1]);
    const int tfree = wmapf_search<NW, false>(L, s, free, st >> 8, st & 255, g >> 8, g & 255, T, tid, nt);
    if (tid == 0) d0[a] = tfree < 0 ? la : tfree + 1;      // (the path itself is a witness: tfree <= la - 1)
    flow += la - 1;
    __syncthreads();      // `cells` is staged again
  }
  if (tid == 0) flow_before[cs] = flow;
  const int kk = K < N ? K : N;
  int taken = 0;
  for (int it = 0; it < iterations; ++it) {
    __syncthreads();      // d0, and the lengths and paths of an accepted iteration
    if (tid == 0) seed_found = -1;      // (set again behind the first round of the chunk loop below)
    // the seed: the (it mod N)-th agent by (-delay, index); 0 <= delay < T
    const int rank = it % N;
    int lo = 0, hi = T, above = 0;      // count(delay >= lo) > rank >= count(delay >= hi) = above
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1, cnt = wlns_count_ge(s, len, d0, N, mid, tid, nt);
      if (cnt > rank) lo = mid;
      else hi = mid, above = cnt;
    }
    for (int base = 0, seen = above; base < N && seen <= rank; base += nt) {      // the (rank - above)-th agent, in index order, with delay == lo
      const int b = base + tid;
      const bool in_class = b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] == lo;
      const u64 m = __builtin_amdgcn_ballot_w64(in_class);
      wide_post(s, 0, __popcll(m));
      const int p = wide_sync(s);
      const u64 below = s.lane ? m & (~0ull >> (64 - s.lane)) : 0ull;
      if (in_class && seen + wide_sum_before(s, p, 0) + __popcll(below) == rank) seed_found = b;
      seen += wide_sum(s, p, 0);
    }
    __syncthreads();
    const int seed = seed_found;
    if (seed < 0 || seed >= N) continue;      // (cannot happen: every delay lies in 0 .. T - 1)
    // the seed's free path
    const int ls = __builtin_amdgcn_readfirstlane(len[seed]);
    const int* ps = rows + (long long)seed * T * 2;
    const int sr = __builtin_amdgcn_readfirstlane(ps[0]), sc = __builtin_amdgcn_readfirstlane(ps[1]);
    const int gr = __builtin_amdgcn_readfirstlane(ps[2 * ls - 2]), gc = __builtin_amdgcn_readfirstlane(ps[2 * ls - 1]);
    const int tfree = wmapf_search<NW, false>(L, s, free, sr, sc, gr, gc, T, tid, nt);
    if (tfree < 0) continue;                  // (cannot happen either)
    wmapf_backtrace<NW, false>(L, s, fcells, gr, gc, tfree, W, tid);
    if (tid == 0) nb[0] = seed;
    __syncthreads();
    // the neighbourhood: who is in the way of the free path, threads over agents
    int m = 1;
    for (int t = 0; t <= tfree && m < kk; ++t) {
      const int fc = fcells[t], fp = t >= 1 ? fcells[t - 1] : -1;
      for (int base = 0; base < N && m < kk; base += nt) {
        const int b = base + tid;
        bool in = false;
        if (b < N) {
          const int lb = len[b];
          const wlns_row pb{rows + (long long)b * T * 2};
          const int cb = pb(t < lb ? t : lb - 1);
          in = cb == fc;
          if (!in && t >= 1 && cb == fp) in = pb(t - 1 < lb ? t - 1 : lb - 1) == fc;
          for (int j = 0; j < m; ++j) in = in && nb[j] != b;
        }
        const u64 mask = __builtin_amdgcn_ballot_w64(in);
        wide_post(s, 0, __popcll(mask));
        const int p = wide_sync(s);      // every thread has read nb
        const int total = wide_sum(s, p, 0);
        if (total) {      // newcomers in index order: the waves in front, then the lanes below
          const u64 below = s.lane ? mask & (~0ull >> (64 - s.lane)) : 0ull;
          const int place = m + wide_sum_before(s, p, 0) + __popcll(below);
          if (in && place < kk) nb[place] = b;
          m = m + total < kk ? m + total : kk;
          __syncthreads();
        }
      }
    }
    for (int step = 1; m < kk && step < N; ++step) {      // fill up with seed + 1, seed + 2, ...
      const int b = (seed + step) % N;
      bool in = false;
      for (int j = 0; j < m; ++j) in = in || nb[j] == b;
      if (!in) {
        __syncthreads();
        if (tid == 0) nb[m] = b;
        ++m;
        __syncthreads();
      }
    }
    // un-reserve the old paths, read from their global rows
    int old_sum = 0;
    for (int j = 0; j < m; ++j) {
      const int a = nb[j], la = __builtin_amdgcn_readfirstlane(len[a]);
      wlns_mark<false>(L, wlns_row{rows + (long long)a * T * 2}, la, T, tid, nt);
      if (tid == 0) old_len[j] = la;
      old_sum += la;
    }
    __syncthreads();
    // re-plan in list order, each agent against everything reserved now
    int done = 0, new_sum = 0;
    for (; done < m; ++done) {
      const int la = old_len[done];
      const wlns_row row{rows + (long long)nb[done] * T * 2};
      const int st = __builtin_amdgcn_readfirstlane(row(0)), g = __builtin_amdgcn_readfirstlane(row(la - 1));
      const int tstar = wmapf_search<NW, true>(L, s, free, st >> 8, st & 255, g >> 8, g & 255, T, tid, nt);
      if (tstar < 0) break;
      wmapf_backtrace<NW, true>(L, s, new_cells[done], g >> 8, g & 255, tstar, W, tid);
      if (tid == 0) new_len[done] = tstar + 1;
      __syncthreads();
      wlns_mark<true>(L, wlns_staged{new_cells[done]}, tstar + 1, T, tid, nt);
      new_sum += tstar + 1;
      __syncthreads();      // the next agent loads these boards
    }
    if (done == m && new_sum < old_sum) {
      for (int j = 0; j < m; ++j) {
        const int a = nb[j], ln = new_len[j];
        int* p = rows + (long long)a * T * 2;
        for (int t = tid; t < T; t += nt) {
          const int cell = new_cells[j][t < ln ? t : ln - 1];
          p[2 * t] = cell >> 8;
          p[2 * t + 1] = cell & 255;
        }
        if (tid == 0) len[a] = ln;
      }
      ++taken;
    } else {
      for (int j = 0; j < done; ++j) wlns_mark<false>(L, wlns_staged{new_cells[j]}, new_len[j], T, tid, nt);
      __syncthreads();
      for (int j = 0; j < m; ++j) wlns_mark<true>(L, wlns_row{rows + (long long)nb[j] * T * 2}, old_len[j], T, tid, nt);
    }
  }
  __syncthreads();
  int total = 0, longest = 1;
  for (int base = 0; base < N; base += nt) {
    const int b = base + tid, lb = b < N ? len[b] : 1;
    total += lb - 1;
    longest = lb > longest ? lb : longest;
  }
  wide_post(s, 0, wave_all_sum(total));
  wide_post(s, 1, wave_all_max(longest));
  const int p = wide_sync(s);
  if (tid == 0) {
    makespan[cs] = wide_max(s, p, 1) - 1;
    flow_after[cs] = wide_sum(s, p, 0);
    accepted[cs] = taken;
    status[cs] = 0;
  }
}

}  // namespace

extern "C" size_t magat_sim_mapf_improve_wide_workspace_bytes(int C, int H, int W, int N, int T) {
  if (C <= 0 || H <= 0 || W <= 0 || N <= 0 || T <= 0 || H > WIDE_SIDE || W > WIDE_SIDE) return 0;
  return (size_t)C * (size_t)wlns_case_words(wide_rows(H), wide_words(W), N, T) * sizeof(u64);
}

extern "C" int magat_sim_mapf_improve_wide(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved, int32_t* paths,
                                           int32_t* lengths, int32_t* makespan, int32_t* flowtime_before, int32_t* flowtime_after,
                                           int32_t* accepted, int32_t* status, void* workspace, size_t workspace_bytes, int C, int N,
                                           int T, int iterations, int k, void* stream) {
  if (!map || !solved || !paths || !lengths || !makespan || !flowtime_before || !flowtime_after || !accepted || !status || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > WIDE_SIDE || W > WIDE_SIDE || T > WMAPF_MAX_T) return MAGAT_ERR_UNSUPPORTED;
  if (k < 1 || k > WLNS_MAX_K || iterations < 0 || iterations > WLNS_MAX_ITERATIONS) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
  magat_form_note(MAGAT_FORM_SIM_MAPF_LNS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_LNS, st);
  switch (wide_words(W)) {      // static LDS only: 8 + 32 KB of paths, the free rows (2, 4 or 8 KB) and the mail
    case 1:
      hipLaunchKernelGGL(wmapf_lns_kernel<1>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, makespan,
                         flowtime_before, flowtime_after, accepted, status, ws, N, T, iterations, k);
      break;
    case 2:
      hipLaunchKernelGGL(wmapf_lns_kernel<2>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, makespan,
                         flowtime_before, flowtime_after, accepted, status, ws, N, T, iterations, k);
      break;
    default:
      hipLaunchKernelGGL(wmapf_lns_kernel<4>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, makespan,
                         flowtime_before, flowtime_after, accepted, status, ws, N, T, iterations, k);
      break;
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}
