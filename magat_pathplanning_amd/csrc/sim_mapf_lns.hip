// Improves the schedules of the path-finding expert by neighbourhood re-planning (MAPF-LNS on top of prioritized planning;
// DESIGN 4.11, restated cell by cell in tests/lns_restatement.py).  It is still NOT ECBS: no bound on the flowtime - the only
// promises are that the flowtime never rises and that a valid schedule stays valid.
//   magat_sim_mapf_improve_workspace_bytes   per case: the reservation boards, 5 * T * 64 * 8 bytes, and d0, one int per agent
//   magat_sim_mapf_improve                   one wavefront per case runs every iteration; one launch, no host round trip
// The layout of mapf_plan_kernel (sim_mapf.hip): lane = map row, one 64-bit word per row, reservation boards in the workspace
// (zeroed here), R layers in dynamic LDS; search and backtrace are the solver's own (sim_mapf_parts.h).  Integer and bit
// arithmetic only, no random numbers.  Per case, on a solved schedule (an agent's cell at t: paths[a][min(t, length - 1)]):
//   screening      solved == 0: status 1; a length outside 1..T, one of the T cells of a row off the map or on an obstacle, a
//                  step that is none of the five moves: status 2.  Such a case is left as it came.
//   set-up         all N paths reserved; d0[a] = the length of a's free path (the search with the board loads compiled out).
//   iteration i    seed = the (i mod N)-th agent by (-delay, index), delay = length - d0: found by counting (a bisection over
//                  the delay, then the index inside the class), lanes over agents.  The seed's free path is searched and
//                  traced again; along it, lanes over agents in chunks of 64 and a ballot, the agents standing on its cell
//                  at t or swapping with it join the neighbourhood (index order, at most k), then seed + 1, seed + 2, ...
//                  Old cells of the neighbourhood are staged in LDS and un-reserved, its agents re-planned in list order and
//                  reserved, new cells staged in LDS; accepted iff everybody arrived and the lengths sum to strictly less -
//                  only then are the global paths and lengths overwritten - else the new paths are cleared and the old ones
//                  reserved again (exact: in a valid schedule no two agents share a V or an A_d bit).
// Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_parts.h"      // MAPF_*, board_row, mapf_search, mapf_backtrace

namespace {

constexpr int LNS_MAX_K = 8;
constexpr int LNS_MAX_ITERATIONS = 4096;

__host__ __device__ inline long long lns_case_words(int N, int T) {      // boards, then d0 padded to whole words
  return (long long)T * MAPF_BOARDS * MAPF_SIDE + ((long long)N + 1) / 2;
}

// Reserves (SET) or un-reserves one path given as LDS cells (row << 8 | col), lanes over t: layer t belongs to one lane, so
// no two lanes touch one word.  V[t] along the path and at its last cell behind it, A_d[t] at the entered cell of a real move.
template <bool SET>
__device__ void lns_mark(u64* boards, const int* cells, int len, int T, int lane) {
  for (int t = lane; t < T; t += 64) {
    const int cell = cells[t < len ? t : len - 1], cr = cell >> 8, cc = cell & 255;
    u64* v = boards + ((long long)t * MAPF_BOARDS) * MAPF_SIDE + cr;
    if (SET) *v |= 1ull << cc;
    else *v &= ~(1ull << cc);
    if (t >= 1 && t < len) {
      const int from = cells[t - 1], dr = cr - (from >> 8), dc = cc - (from & 255);
      const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : dc == 1 ? 3 : 4;
      if (d < 4) {
        u64* a = boards + ((long long)t * MAPF_BOARDS + 1 + d) * MAPF_SIDE + cr;
        if (SET) *a |= 1ull << cc;
        else *a &= ~(1ull << cc);
      }
    }
  }
}

// the first `len` cells of a global path row -> LDS
__device__ void lns_stage(int* cells, const int* p, int len, int lane) {
  for (int t = lane; t < len; t += 64) cells[t] = p[2 * t] << 8 | p[2 * t + 1];
}

// how many agents have delay = length - d0 >= x (wave-uniform)
__device__ int lns_count_ge(const int* len, const int* d0, int N, int x, int lane) {
  int cnt = 0;
  for (int base = 0; base < N; base += 64) {
    const int b = base + lane;
    cnt += __popcll(__builtin_amdgcn_ballot_w64(b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] >= x));
  }
  return cnt;
}

__global__ __launch_bounds__(64) void mapf_lns_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                      const uint8_t* __restrict__ solved, int* paths, int* lengths, int* makespan,
                                                      int* __restrict__ flow_before, int* __restrict__ flow_after,
                                                      int* __restrict__ accepted, int* __restrict__ status, u64* workspace, int N,
                                                      int T, int iterations, int K) {
  HIP_DYNAMIC_SHARED(u64, R)                      // [T][64]
  __shared__ u64 free_rows[MAPF_SIDE];            // the free cells, for the lanes that are not the cell's row
  __shared__ int cells[MAPF_MAX_T];               // set-up: the path being reserved
  __shared__ int fcells[MAPF_MAX_T];              // the seed's free path
  __shared__ int old_cells[LNS_MAX_K][MAPF_MAX_T], new_cells[LNS_MAX_K][MAPF_MAX_T];      // the stage
  __shared__ int nb[LNS_MAX_K], old_len[LNS_MAX_K], new_len[LNS_MAX_K];
  const int cs = blockIdx.x, lane = threadIdx.x;
  u64* boards = workspace + (long long)cs * lns_case_words(N, T);
  int* d0 = reinterpret_cast<int*>(boards + (long long)T * MAPF_BOARDS * MAPF_SIDE);
  const long long a0 = (long long)cs * N;
  int* len = lengths + a0;
  int* rows = paths + a0 * T * 2;      // agent a's row: rows + a * T * 2
  if (lane == 0) {
    flow_before[cs] = 0;
    flow_after[cs] = 0;
    accepted[cs] = 0;
  }
  if (solved[cs] == 0) {
    if (lane == 0) status[cs] = 1;
    return;
  }
  const uint8_t* mp = map + cs * map_stride;
  u64 free = 0ull;
  for (int r = 0; r < H; ++r) {
    const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] == 0);
    if (lane == r) free = word;
  }
  free_rows[lane] = free;
  __syncthreads();
  // screening, lanes over t
  bool bad = false;
  for (int a = 0; a < N; ++a) {
    const int la = len[a];
    bad |= la < 1 || la > T;
    const int* p = rows + (long long)a * T * 2;
    for (int t = lane; t < T; t += 64) {
      const int r = p[2 * t], c = p[2 * t + 1];
      const bool inside = r >= 0 && r < H && c >= 0 && c < W;
      bad |= !inside || !has_bit(free_rows[inside ? r : 0], inside ? c : 0);
      if (t >= 1 && inside) {
        const int pr = p[2 * t - 2], pc = p[2 * t - 1];
        const bool pin = pr >= 0 && pr < H && pc >= 0 && pc < W;      // (a cell outside is refused by its own lane)
        const int dr = pin ? r - pr : 0, dc = pin ? c - pc : 0;
        bad |= !((dr == 0 && dc >= -1 && dc <= 1) || (dc == 0 && dr >= -1 && dr <= 1));
      }
    }
  }
  if (wave_any(bad)) {
    if (lane == 0) status[cs] = 2;
    return;
  }
  // set-up: every path reserved, d0 of every agent, the flowtime
  for (int i = lane; i < T * MAPF_BOARDS * MAPF_SIDE; i += 64) boards[i] = 0ull;
  __syncthreads();
  int flow = 0;
  for (int a = 0; a < N; ++a) {
    const int la = __builtin_amdgcn_readfirstlane(len[a]);
    const int* p = rows + (long long)a * T * 2;
    lns_stage(cells, p, la, lane);
    __syncthreads();
    lns_mark<true>(boards, cells, la, T, lane);
    const int s = __builtin_amdgcn_readfirstlane(cells[0]), g = __builtin_amdgcn_readfirstlane(cells[la - 1]);
    const int tfree = mapf_search<false>(nullptr, R, free, s >> 8, s & 255, g >> 8, g & 255, T, lane);
    if (lane == 0) d0[a] = tfree < 0 ? la : tfree + 1;      // (the path itself is a witness: tfree <= la - 1)
    flow += la - 1;
    __syncthreads();      // `cells` is staged again
  }
  if (lane == 0) flow_before[cs] = flow;
  const int kk = K < N ? K : N;
  int taken = 0;
  for (int it = 0; it < iterations; ++it) {
    __syncthreads();      // d0, and the lengths and paths of an accepted iteration
    // the seed: the (it mod N)-th agent by (-delay, index); 0 <= delay < T
    const int rank = it % N;
    int lo = 0, hi = T, above = 0;      // count(delay >= lo) > rank >= count(delay >= hi) = above
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1, cnt = lns_count_ge(len, d0, N, mid, lane);
      if (cnt > rank) lo = mid;
      else hi = mid, above = cnt;
    }
    int seed = -1;
    for (int base = 0, seen = above; base < N; base += 64) {      // the (rank - above)-th agent, in index order, with delay == lo
      const int b = base + lane;
      const u64 m = __builtin_amdgcn_ballot_w64(b < N && len[b < N ? b : 0] - d0[b < N ? b : 0] == lo);
      const int pc = __popcll(m);
      if (seen + pc > rank) {
        const u64 below = lane ? m & (~0ull >> (64 - lane)) : 0ull;
        const u64 pick = __builtin_amdgcn_ballot_w64(has_bit(m, lane) && seen + __popcll(below) == rank);
        seed = base + __builtin_ctzll(pick);
        break;
      }
      seen += pc;
    }
    if (seed < 0 || seed >= N) continue;      // (cannot happen: every delay lies in 0 .. T - 1)
    // the seed's free path
    const int ls = __builtin_amdgcn_readfirstlane(len[seed]);
    const int* ps = rows + (long long)seed * T * 2;
    const int sr = __builtin_amdgcn_readfirstlane(ps[0]), sc = __builtin_amdgcn_readfirstlane(ps[1]);
    const int gr = __builtin_amdgcn_readfirstlane(ps[2 * ls - 2]), gc = __builtin_amdgcn_readfirstlane(ps[2 * ls - 1]);
    const int tfree = mapf_search<false>(nullptr, R, free, sr, sc, gr, gc, T, lane);
    if (tfree < 0) continue;                  // (cannot happen either)
    __syncthreads();
    mapf_backtrace<false>(nullptr, R, fcells, gr, gc, tfree, W, lane);
    if (lane == 0) nb[0] = seed;
    __syncthreads();
    // the neighbourhood: who is in the way of the free path, lanes over agents
    int m = 1;
    for (int t = 0; t <= tfree && m < kk; ++t) {
      const int fc = fcells[t], fp = t >= 1 ? fcells[t - 1] : -1;
      for (int base = 0; base < N && m < kk; base += 64) {
        const int b = base + lane;
        bool in = false;
        if (b < N) {
          const int lb = len[b];
          const int* pb = rows + (long long)b * T * 2;
          const int tb = t < lb ? t : lb - 1, cb = pb[2 * tb] << 8 | pb[2 * tb + 1];
          in = cb == fc;
          if (!in && t >= 1 && cb == fp) {
            const int tp = t - 1 < lb ? t - 1 : lb - 1;
            in = (pb[2 * tp] << 8 | pb[2 * tp + 1]) == fc;
          }
          for (int j = 0; j < m; ++j) in = in && nb[j] != b;
        }
        u64 mask = __builtin_amdgcn_ballot_w64(in);
        if (mask) {
          __syncthreads();      // every lane has read nb
          while (mask && m < kk) {
            if (lane == 0) nb[m] = base + __builtin_ctzll(mask);
            mask &= mask - 1;
            ++m;
          }
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
        if (lane == 0) nb[m] = b;
        ++m;
        __syncthreads();
      }
    }
    // stage and un-reserve the old paths
    int old_sum = 0;
    for (int j = 0; j < m; ++j) {
      const int a = nb[j], la = __builtin_amdgcn_readfirstlane(len[a]);
      lns_stage(old_cells[j], rows + (long long)a * T * 2, la, lane);
      if (lane == 0) old_len[j] = la;
      old_sum += la;
    }
    __syncthreads();
    for (int j = 0; j < m; ++j) lns_mark<false>(boards, old_cells[j], old_len[j], T, lane);
    __syncthreads();
    // re-plan in list order, each agent against everything reserved now
    int done = 0, new_sum = 0;
    for (; done < m; ++done) {
      const int la = old_len[done];
      const int s = __builtin_amdgcn_readfirstlane(old_cells[done][0]), g = __builtin_amdgcn_readfirstlane(old_cells[done][la - 1]);
      const int tstar = mapf_search<true>(boards, R, free, s >> 8, s & 255, g >> 8, g & 255, T, lane);
      if (tstar < 0) break;
      __syncthreads();
      mapf_backtrace<true>(boards, R, new_cells[done], g >> 8, g & 255, tstar, W, lane);
      if (lane == 0) new_len[done] = tstar + 1;
      __syncthreads();
      lns_mark<true>(boards, new_cells[done], tstar + 1, T, lane);
      new_sum += tstar + 1;
      __syncthreads();      // the next agent loads these boards
    }
    if (done == m && new_sum < old_sum) {
      for (int j = 0; j < m; ++j) {
        const int a = nb[j], ln = new_len[j];
        int* p = rows + (long long)a * T * 2;
        for (int t = lane; t < T; t += 64) {
          const int cell = new_cells[j][t < ln ? t : ln - 1];
          p[2 * t] = cell >> 8;
          p[2 * t + 1] = cell & 255;
        }
        if (lane == 0) len[a] = ln;
      }
      ++taken;
    } else {
      for (int j = 0; j < done; ++j) lns_mark<false>(boards, new_cells[j], new_len[j], T, lane);
      __syncthreads();
      for (int j = 0; j < m; ++j) lns_mark<true>(boards, old_cells[j], old_len[j], T, lane);
    }
  }
  __syncthreads();
  int total = 0, longest = 1;
  for (int base = 0; base < N; base += 64) {
    const int b = base + lane, lb = b < N ? len[b] : 1;
    total += lb - 1;
    longest = lb > longest ? lb : longest;
  }
  total = wave_all_sum(total);
  longest = wave_all_max(longest);
  if (lane == 0) {
    makespan[cs] = longest - 1;
    flow_after[cs] = total;
    accepted[cs] = taken;
    status[cs] = 0;
  }
}

}  // namespace

extern "C" size_t magat_sim_mapf_improve_workspace_bytes(int C, int N, int T) {
  if (C <= 0 || N <= 0 || T <= 0) return 0;
  return (size_t)C * (size_t)lns_case_words(N, T) * sizeof(u64);
}

extern "C" int magat_sim_mapf_improve(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved, int32_t* paths,
                                      int32_t* lengths, int32_t* makespan, int32_t* flowtime_before, int32_t* flowtime_after,
                                      int32_t* accepted, int32_t* status, void* workspace, size_t workspace_bytes, int C, int N,
                                      int T, int iterations, int k, void* stream) {
  if (!map || !solved || !paths || !lengths || !makespan || !flowtime_before || !flowtime_after || !accepted || !status || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > MAPF_SIDE || W > MAPF_SIDE || T > MAPF_MAX_T) return MAGAT_ERR_UNSUPPORTED;
  if (k < 1 || k > LNS_MAX_K || iterations < 0 || iterations > LNS_MAX_ITERATIONS) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_improve_workspace_bytes(C, N, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  // dynamic LDS: the R layers, <= 128 KB; + 19 KB static (the stage of 2 * 8 paths, two paths, the free rows)
  const size_t lds = (size_t)T * MAPF_SIDE * sizeof(u64);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (magat_ensure_dyn_lds(reinterpret_cast<const void*>(&mapf_lns_kernel), MAGAT_LDS_SIM_MAPF_LNS, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  magat_form_note(MAGAT_FORM_SIM_MAPF_LNS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_LNS, st);
  hipLaunchKernelGGL(mapf_lns_kernel, dim3((unsigned)C), dim3(64), lds, st, map, map_batched ? (long long)H * W : 0LL, H, W, solved,
                     paths, lengths, makespan, flowtime_before, flowtime_after, accepted, status, static_cast<u64*>(workspace), N, T,
                     iterations, k);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
