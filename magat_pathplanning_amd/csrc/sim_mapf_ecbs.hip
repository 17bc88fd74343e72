// A bounded-suboptimal multi-agent path-finding expert for C cases at once: enhanced conflict-based search (ECBS) on the device -
// conflict-based search with a focal search on both levels (the rule is in include/magat_hip.h, restated cell by cell
// in tests/ecbs_restatement.py).  A solved case promises 1000 * flowtime <= w_milli * lower_bound <= w_milli * optimum.
//   magat_sim_mapf_ecbs_workspace_bytes   per case: hard and soft boards, the planes, the root's paths, the node pool, five int rows
//   magat_sim_mapf_ecbs                   one wavefront per case runs the whole tree; one launch, no host round trip
// The tree is sim_mapf_tree.h's walk, under the focal rule (FOCAL = true).  This file brings its form.  The layout of
// mapf_cbs_kernel (sim_mapf_cbs.hip): lane = map row, one 64-bit word per row.  Per case:
//   hard boards    workspace [t][V, A_up, A_left, A_down, A_right][row]: the constraints of the agent that is searched, as in CBS.
//   soft boards    a second set: the planner's reservation of every OTHER agent of the schedule the search runs against, set
//                  before a search and cleared after it by lanes over t (a lane owns the words of its t).  None at K = 1.
//   planes         workspace [k][t][row], K = levels of them: plane K - 1 is the planner's R on the hard boards, plane k below it
//                  the cells reached with at most k steps that break a soft board.  A lane reads back only the rows it wrote.
//   focal search   ecbs_search / ecbs_backtrace below: t*, and the arrival (plane ka, step ta) that the trace starts from.
//   node pool      workspace: 32 bytes per node (sim_mapf_ecbs_parts.h) and its agent's new path, T cells of 16 bits; the root's N
//                  paths, lengths and t*, and `src`, beside it.
//   LDS            the two cell-owner grids of the conflict scan and the conflict count (32 KB) and the path just traced (1 KB).
// Integer and bit arithmetic only.  Every store is a per-lane (vector) store or an LDS atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_MAX_N, audit_stage2 - the walk's conflict scan
#include "sim_mapf_cbs_parts.h"        // cbs_wave
#include "sim_mapf_ecbs_parts.h"       // ECBS_*, ecbs_node
#include "sim_mapf_parts.h"            // MAPF_*, board_row
#include "sim_mapf_tree.h"             // mapf_tree_search, tree_entry_check

namespace {

constexpr int ECBS_GRID = MAPF_SIDE * MAPF_SIDE;

// per case, in 64-bit words: hard boards | soft boards | planes | root paths | node paths | nodes | rlen, rts, src, the two cell rows
struct ecbs_layout {
  long long soft, planes, root, npath, nodes, ints, words;
};
__host__ __device__ inline ecbs_layout ecbs_case_layout(int N, int T, int M, int K) {
  ecbs_layout l;
  l.soft = (long long)T * MAPF_BOARDS * MAPF_SIDE;
  l.planes = 2 * l.soft;
  l.root = l.planes + (long long)K * T * MAPF_SIDE;
  l.npath = l.root + ((long long)N * T + 3) / 4;
  l.nodes = l.npath + ((long long)M * T + 3) / 4;
  l.ints = l.nodes + (long long)M * 4;
  l.words = l.ints + (5LL * N + 1) / 2;
  return l;
}

// the planner's reservation of one row of the schedule (padded with its last cell) on the soft boards, or its removal: V[t] at the
// cell of every t < T, A_d[t] at the entered cell of a real move.  Lanes over t: a lane touches the words of its own t only.
template <bool SET>
__device__ __forceinline__ void ecbs_reserve(u64* soft, const int* p, int T, int lane) {
  for (int t = lane; t < T; t += 64) {
    const int r = p[2 * t], c = p[2 * t + 1];
    u64* layer = soft + (long long)t * MAPF_BOARDS * MAPF_SIDE;
    if (SET) layer[r] |= 1ull << c;
    else layer[r] &= ~(1ull << c);
    if (t >= 1) {
      const int dr = r - p[2 * t - 2], dc = c - p[2 * t - 1];
      if (dr != 0 || dc != 0) {
        const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : 3;
        if (SET) layer[(1 + d) * MAPF_SIDE + r] |= 1ull << c;
        else layer[(1 + d) * MAPF_SIDE + r] &= ~(1ull << c);
      }
    }
  }
}

// one layer of the planner's flood from the cells `cur` onto the boards of the layer it arrives in
__device__ __forceinline__ u64 ecbs_step(u64 cur, u64 free, u64 v, u64 a_up, u64 a_left, u64 a_down, u64 a_right) {
  const u64 moved = cells_up(cur & ~a_down) | ((cur & ~a_right) >> 1) | cells_down(cur & ~a_up) | ((cur & ~a_left) << 1);
  return (cur | moved) & free & ~v;
}

// The focal search of one agent.  P[k][t][row]: P^k_0 = {start}; P^(K-1)_(t+1) = hard(P^(K-1)_t); P^0_(t+1) = clean(P^0_t);
// P^k_(t+1) = clean(P^k_t) | hard(P^(k-1)_t) in between.  t* is mapf_search's on plane K - 1; the flood goes on to
// b = min(w_milli * t* / 1000, T - 1) and ends early once the goal is in plane 0.  Returns t* or -1, and the arrival: the smallest
// k with the goal in P^k_t for a t in [t*, b], then the smallest such t.  Wave-uniform.
template <int K>
__device__ int ecbs_search(const u64* hard, const u64* soft, u64* P, u64 free, int sr, int sc, int gr, int gc, int T, int w_milli,
                           int lane, int* k_out, int* t_out) {
  int last = -1;
  for (int base = (T - 1) & ~63; base >= 0; base -= 64) {      // lanes over t, highest 64 first
    const int t = base + lane;
    const u64 m = __builtin_amdgcn_ballot_w64(t < T && has_bit(*board_row(hard, t < T ? t : 0, 0, gr), gc));
    if (m) {
      last = base + 63 - __clzll(m);
      break;
    }
  }
  if (last >= T - 1) return -1;      // the goal is held for ever
  const long long plane = (long long)T * MAPF_SIDE;
  u64 cur[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cur[k] = lane == sr ? 1ull << sc : 0ull;
    P[k * plane + lane] = cur[k];
  }
  u64 hd[MAPF_AHEAD][MAPF_BOARDS], cl[MAPF_AHEAD][MAPF_BOARDS];      // the hard boards, and hard | soft
#pragma unroll
  for (int i = 0; i < MAPF_AHEAD; ++i)
#pragma unroll
    for (int b = 0; b < MAPF_BOARDS; ++b) {
      hd[i][b] = 1 + i < T ? *board_row(hard, 1 + i, b, lane) : 0ull;
      cl[i][b] = hd[i][b];
      if constexpr (K > 1) cl[i][b] |= 1 + i < T ? *board_row(soft, 1 + i, b, lane) : 0ull;
    }
  int tstar = -1, bound = T - 1, best_k = K, best_t = -1;
  for (int t0 = 0;; t0 += MAPF_AHEAD) {
#pragma unroll
    for (int i = 0; i < MAPF_AHEAD; ++i) {
      const int t = t0 + i;      // cur[k] = P^k_t; hd[i], cl[i] = the boards of layer t + 1
      if (tstar < 0) {
        if (t > last && wave_any(lane == gr && has_bit(cur[K - 1], gc))) {
          tstar = t;
          const long long b = (long long)w_milli * t / 1000;
          bound = b < T - 1 ? (int)b : T - 1;
        } else if (t == T - 1 || !wave_any(cur[K - 1] != 0ull)) {
          return -1;
        }
      }
      if (tstar >= 0) {
#pragma unroll
        for (int k = K - 1; k >= 0; --k)
          if (k < best_k && wave_any(lane == gr && has_bit(cur[k], gc))) best_k = k, best_t = t;
        if (best_k == 0 || t == bound) {
          *k_out = best_k, *t_out = best_t;
          return tstar;
        }
      }
      u64 h[MAPF_BOARDS], c[MAPF_BOARDS];
      const int tn = t + 1 + MAPF_AHEAD;
#pragma unroll
      for (int b = 0; b < MAPF_BOARDS; ++b) {
        h[b] = hd[i][b], c[b] = cl[i][b];
        hd[i][b] = tn < T ? *board_row(hard, tn, b, lane) : 0ull;
        cl[i][b] = hd[i][b];
        if constexpr (K > 1) cl[i][b] |= tn < T ? *board_row(soft, tn, b, lane) : 0ull;
      }
      u64 nxt[K];
      nxt[K - 1] = ecbs_step(cur[K - 1], free, h[0], h[1], h[2], h[3], h[4]);
#pragma unroll
      for (int k = 0; k + 1 < K; ++k) {
        nxt[k] = ecbs_step(cur[k], free, c[0], c[1], c[2], c[3], c[4]);
        if (k >= 1) nxt[k] |= ecbs_step(cur[k - 1], free, h[0], h[1], h[2], h[3], h[4]);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        cur[k] = nxt[k];
        P[k * plane + (long long)(t + 1) * MAPF_SIDE + lane] = cur[k];
      }
    }
  }
}

// the first of up, left, down, right, stop whose source cell is in `prev` and, for a real move, not in A_opp(d) - or -1.  Each
// candidate is tested by the lane of its row.
__device__ __forceinline__ int ecbs_source(u64 prev, u64 a_up, u64 a_left, u64 a_down, u64 a_right, int r, int c, int W, int lane) {
  const bool up = lane == r + 1 && has_bit(prev & ~a_down, c);                    // moved up: came from the row below
  const bool left = lane == r && c + 1 < W && has_bit(prev & ~a_right, c + 1 < W ? c + 1 : c);
  const bool down = lane == r - 1 && has_bit(prev & ~a_up, c);
  const bool right = lane == r && c >= 1 && has_bit(prev & ~a_left, c >= 1 ? c - 1 : c);
  const bool stop = lane == r && has_bit(prev, c);
  const bool any_up = wave_any(up), any_left = wave_any(left), any_down = wave_any(down), any_right = wave_any(right), any_stop = wave_any(stop);
  return any_up ? 0 : any_left ? 1 : any_down ? 2 : any_right ? 3 : any_stop ? 4 : -1;
}

// Walks from (goal, t, plane k) down to t = 1.  In plane K - 1: any hard-allowed source in P^(K-1)_(t-1).  In a plane below it:
// first a source in P^k_(t-1) whose step is clean - none when the cell is in soft V[t], where it can only have been reached by a
// drop - else a hard-allowed source in P^(k-1)_(t-1), and on in plane k - 1.  Lane 0 writes the cells.
template <int K>
__device__ void ecbs_backtrace(const u64* hard, const u64* soft, const u64* P, int* cells, int gr, int gc, int k, int t, int T, int W,
                               int lane) {
  const long long plane = (long long)T * MAPF_SIDE;
  int r = gr, c = gc;
  if (lane == 0) cells[t] = r << 8 | c;
  for (; t >= 1; --t) {
    u64 h[4], s[4], sv = 0ull;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      h[b] = *board_row(hard, t, 1 + b, lane);
      s[b] = 0ull;
      if constexpr (K > 1) s[b] = *board_row(soft, t, 1 + b, lane);
    }
    if constexpr (K > 1) sv = *board_row(soft, t, 0, lane);
    const u64 here = P[k * plane + (long long)(t - 1) * MAPF_SIDE + lane];
    const u64 below = k >= 1 ? P[(k - 1) * plane + (long long)(t - 1) * MAPF_SIDE + lane] : 0ull;
    int mv = -1;
    if (k == K - 1) {
      mv = ecbs_source(here, h[0], h[1], h[2], h[3], r, c, W, lane);
    } else {
      if (!wave_any(lane == r && has_bit(sv, c))) mv = ecbs_source(here, h[0] | s[0], h[1] | s[1], h[2] | s[2], h[3] | s[3], r, c, W, lane);
      if (mv < 0 && k >= 1) {
        mv = ecbs_source(below, h[0], h[1], h[2], h[3], r, c, W, lane);
        --k;
      }
    }
    if (mv == 0) r += 1;
    else if (mv == 1) c += 1;
    else if (mv == 2) r -= 1;
    else if (mv == 3) c -= 1;
    if (lane == 0) cells[t - 1] = r << 8 | c;
  }
}

template <int K>
struct ecbs_form : cbs_wave {
  static constexpr bool FOCAL = true, BORROWS_GRIDS = false;
  u64 *soft, *P;
  int *own0, *own1;
  int T, W, w_milli, ka, ta;
  template <bool SET>
  __device__ __forceinline__ void reserve(const int* p) const {
    if constexpr (K > 1) ecbs_reserve<SET>(soft, p, T, tid);
  }
  template <bool CHILD>
  __device__ __forceinline__ int search(int sr, int sc, int gr, int gc) {
    ka = 0, ta = 0;
    return ecbs_search<K>(hard, soft, P, free, sr, sc, gr, gc, T, w_milli, tid, &ka, &ta);
  }
  template <bool CHILD>
  __device__ __forceinline__ void trace(int* cells, int gr, int gc) const {
    ecbs_backtrace<K>(hard, soft, P, cells, gr, gc, ka, ta, T, W, tid);
  }
};

template <int K>
__global__ __launch_bounds__(64) void mapf_ecbs_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                       const int* __restrict__ start, const int* __restrict__ goal, int* paths,
                                                       int* lengths, int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                       int* __restrict__ status, int* __restrict__ flowtime,
                                                       int* __restrict__ lower_bound, int* __restrict__ nodes_out,
                                                       int* __restrict__ expanded_out, int* __restrict__ horizon_hit, u64* workspace,
                                                       int N, int T, int max_nodes, int w_milli) {
  __shared__ int own[2 * ECBS_GRID];
  __shared__ int cells[MAPF_MAX_T];
  const int cs = blockIdx.x, lane = threadIdx.x;
  const ecbs_layout lay = ecbs_case_layout(N, T, max_nodes, K);
  u64* hard = workspace + (long long)cs * lay.words;
  int* ints = reinterpret_cast<int*>(hard + lay.ints);      // rlen, rts, src, the two cell rows: N ints each
  const long long a0 = (long long)cs * N;
  const tree_case<ecbs_node> k{start + a0 * 2, goal + a0 * 2, paths + a0 * T * 2, lengths + a0,
                               reinterpret_cast<uint16_t*>(hard + lay.root), reinterpret_cast<uint16_t*>(hard + lay.npath),
                               reinterpret_cast<ecbs_node*>(hard + lay.nodes), ints, ints + N, ints + 2 * N, ints + 3 * N, cells,
                               N, T, H, W, max_nodes, w_milli};
  for (long long i = lane; i < lay.planes; i += 64) hard[i] = 0ull;      // both sets of boards
  ecbs_form<K> f{{{lane}, hard}, hard + lay.soft, hard + lay.planes, own, own + ECBS_GRID, T, W, w_milli, 0, 0};
  f.load_free(map + cs * map_stride, H, W);
  mapf_tree_search(f, k, tree_out{makespan, solved, status, flowtime, lower_bound, nodes_out, expanded_out, horizon_hit}, cs);
}

}  // namespace

extern "C" size_t magat_sim_mapf_ecbs_workspace_bytes(int C, int N, int T, int max_nodes, int levels) {
  if (C <= 0 || N <= 0 || T <= 0 || max_nodes <= 0 || levels <= 0 || N > AUDIT_MAX_N || T > MAPF_MAX_T || max_nodes > ECBS_MAX_NODES ||
      levels > ECBS_MAX_LEVELS)
    return 0;
  return (size_t)C * (size_t)ecbs_case_layout(N, T, max_nodes, levels).words * sizeof(u64);
}

extern "C" int magat_sim_mapf_ecbs(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                                   int32_t* paths, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                                   int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                                   void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, int w_milli, int levels,
                                   void* stream) {
  const int rc = tree_entry_check({map, start, goal, paths, lengths, makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit},
                                  H, W, C, N, T, max_nodes, levels > 0 && w_milli >= 1000, levels <= ECBS_MAX_LEVELS && w_milli <= ECBS_MAX_W_MILLI,
                                  MAPF_SIDE, MAPF_MAX_T, ECBS_MAX_NODES, workspace, workspace_bytes,
                                  magat_sim_mapf_ecbs_workspace_bytes(C, N, T, max_nodes, levels));
  if (rc != MAGAT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_MAPF_ECBS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_ECBS, st);
  const long long stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
#define ECBS_LAUNCH(K)                                                                                                              \
  hipLaunchKernelGGL((mapf_ecbs_kernel<K>), dim3((unsigned)C), dim3(64), 0, st, map, stride, H, W, start, goal, paths, lengths,     \
                     makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit, ws, N, T, max_nodes, w_milli)
  if (levels == 1) ECBS_LAUNCH(1);
  else if (levels == 2) ECBS_LAUNCH(2);
  else if (levels == 3) ECBS_LAUNCH(3);
  else ECBS_LAUNCH(4);
#undef ECBS_LAUNCH
  magat_prof_end(pid, st);
  return magat_check_launch();
}
