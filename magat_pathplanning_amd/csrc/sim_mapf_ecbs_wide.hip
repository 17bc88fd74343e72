// The wide form of the bounded-suboptimal expert of sim_mapf_ecbs.hip: the same ECBS rule, cell for cell and node for node (DESIGN
// 4.11; include/magat_hip.h; restated in tests/ecbs_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_ecbs_wide_workspace_bytes   per case: hard and soft boards, the planes, the root's paths, the node pool, five int
//                                              rows and the two cell-owner grids
//   magat_sim_mapf_ecbs_wide                   one workgroup per case runs the whole tree; one launch, no host round trip
// The tree is sim_mapf_tree.h's walk, the one the narrow form runs, under the focal rule.  This file brings its form.  The layout of
// wmapf_plan_kernel (sim_mapf_wide.hip): `rows` = 64 ceil(H / 64) threads, thread = map row, NW = 1, 2 or 4 64-bit words per row in
// registers, votes and minima across the wavefronts through the LDS mail (row_board.h).  Per case, in the workspace:
//   hard boards    [t][V, A_up, A_left, A_down, A_right][row][NW]: the constraints of the agent that is searched.
//   soft boards    a second set: the planner's reservation of every OTHER agent of the schedule the search runs against, set before
//                  a search and cleared after it by threads over t (a thread owns the words of its t).  None at K = 1.
//   planes         [k][t][row][NW], K = levels of them, as in the narrow form.  A thread reads back its own row, and in the
//                  backtrace the rows next to the cell it stands on, behind a barrier.
//   node pool      32 bytes per node (sim_mapf_ecbs_parts.h) and its agent's new path, T cells of 16 bits; the root's N paths, lengths
//                  and t*, and `src`, beside it.
//   grids          the two cell-owner grids of the conflict scan and the conflict count, 2 * H * W ints (512 KB at 256 x 256: not
//                  LDS), global atomicMin; the cell of every agent at two steps in the int rows.
//   LDS            seven copies of the mail - a step of the flood sends the boundary rows of up to seven boards in one round - and
//                  the path just traced (4 KB).  The walk's reductions go through copy 0.
// The flood takes ONE barrier per step: the boundary rows of every plane's hard- and clean-masked fronts and the votes (the goal is
// in plane k; plane K - 1 is not empty) travel together.  The backtrace takes one per step too: every candidate of both planes and
// the soft-V test are one posted word.  All control flow around a barrier is uniform over the workgroup: every condition on it
// comes out of the mail or is read from one address by all threads.
// Integer and bit arithmetic only.  Every store is a per-thread (vector) store or an LDS / global atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_group.h"                  // wide_group: the walk's reductions, the free board
#include "sim_mapf_audit_parts.h"      // AUDIT_MAX_N, audit_stage2 - the walk's conflict scan
#include "sim_mapf_cbs_parts.h"        // (the walk's cbs_mark_chain, cbs_place)
#include "sim_mapf_ecbs_parts.h"       // ECBS_*, ecbs_node
#include "sim_mapf_tree.h"             // mapf_tree_search, tree_entry_check
#include "sim_mapf_wide_parts.h"       // WMAPF_MAX_T, wide_rows / wide_words, wide_layers

namespace {

constexpr int WECBS_BOARDS = 5;                            // V, then A_d in the key order up, left, down, right
constexpr int WECBS_MAILS = 2 * ECBS_MAX_LEVELS - 1;       // hard fronts of the planes 0 .. K - 1, clean fronts of 0 .. K - 2

// Layers of hard and hard | soft boards in flight: 10 NW words a layer.  Chosen per instantiation so that none spills to scratch
// (the compiler's resource report; the table is in DESIGN 4.11).
template <int NW, int K>
constexpr int wecbs_ahead() {
  return NW == 1 ? (K <= 2 ? 4 : 2) : NW == 2 ? 2 : 1;
}

// per case, in 64-bit words: hard boards | soft boards | planes | root paths | node paths | nodes | rlen, rts, src, the two cell
// rows | the two grids
struct wecbs_layout {
  long long soft, planes, root, npath, nodes, ints, grids, words;
};
__host__ __device__ inline wecbs_layout wecbs_case_layout(int H, int W, int N, int T, int M, int K) {
  const long long board = (long long)wide_rows(H) * wide_words(W);
  wecbs_layout l;
  l.soft = (long long)T * WECBS_BOARDS * board;
  l.planes = 2 * l.soft;
  l.root = l.planes + (long long)K * T * board;
  l.npath = l.root + ((long long)N * T + 3) / 4;
  l.nodes = l.npath + ((long long)M * T + 3) / 4;
  l.ints = l.nodes + (long long)M * 4;
  l.grids = l.ints + (5LL * N + 1) / 2;
  l.words = l.grids + (long long)H * W;
  return l;
}

template <int NW>
using wecbs_set = wide_layers<NW, WECBS_BOARDS>;
template <int NW>
using wecbs_plane = wide_layers<NW, 1>;

// one constraint bit, by the thread of its row
template <bool SET, int NW>
__device__ __forceinline__ void wecbs_mark(const wecbs_set<NW>& L, int board, int t, int r, int c, int tid) {
  if (tid == r) {
    u64* w = L.at(t, board, r) + (c >> 6);
    if (SET) *w |= 1ull << (c & 63);
    else *w &= ~(1ull << (c & 63));
  }
}

// the planner's reservation of one row of the schedule (padded with its last cell) on the soft boards, or its removal: V[t] at the
// cell of every t < T, A_d[t] at the entered cell of a real move.  Threads over t: a thread touches the words of its own t only.
template <bool SET, int NW>
__device__ __forceinline__ void wecbs_reserve(const wecbs_set<NW>& L, const int* p, int T, int tid, int nt) {
  for (int t = tid; t < T; t += nt) {
    const int r = p[2 * t], c = p[2 * t + 1];
    u64* v = L.at(t, 0, r) + (c >> 6);
    if (SET) *v |= 1ull << (c & 63);
    else *v &= ~(1ull << (c & 63));
    if (t >= 1) {
      const int dr = r - p[2 * t - 2], dc = c - p[2 * t - 1];
      if (dr != 0 || dc != 0) {
        const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : 3;
        u64* a = L.at(t, 1 + d, r) + (c >> 6);
        if (SET) *a |= 1ull << (c & 63);
        else *a &= ~(1ull << (c & 63));
      }
    }
  }
}

// one layer of the planner's flood from the cells `cur` onto the boards b[] of the layer it arrives in; up / down: the fronts
// cur & ~A_down and cur & ~A_up, already shifted across the rows
template <int NW>
__device__ __forceinline__ wboard<NW> wecbs_step(const wboard<NW>& cur, const wboard<NW>& free, const wboard<NW>* b,
                                                 const wboard<NW>& up, const wboard<NW>& down) {
  return (cur | up | wb_left(cur & ~b[4]) | down | wb_right(cur & ~b[2])) & free & ~b[0];
}

// The focal search of one agent, the narrow form's (sim_mapf_ecbs.hip: ecbs_search) on wide boards.  P[k][t][row]: P^k_0 =
// {start}; P^(K-1)_(t+1) = hard(P^(K-1)_t); P^0_(t+1) = clean(P^0_t); P^k_(t+1) = clean(P^k_t) | hard(P^(k-1)_t) in between.  t*
// is wmapf_search's on plane K - 1; the flood goes on to b = min(w_milli * t* / 1000, T - 1) and ends early once the goal is in
// plane 0.  Returns t* or -1, and the arrival: the smallest k with the goal in P^k_t for a t in [t*, b], then the smallest such t.
// The same for every thread.  Mail copy j < K carries the hard front of plane j, copy K + j the clean front of plane j.
template <int NW, int K>
__device__ int wecbs_search(const wecbs_set<NW>& hard, const wecbs_set<NW>& soft, u64* planes, long long plane_words, wide_seat& s,
                            const wboard<NW>& free, int sr, int sc, int gr, int gc, int T, int w_milli, int tid, int nt, int* k_out,
                            int* t_out) {
  constexpr int AHEAD = wecbs_ahead<NW, K>();
  int hit = -1;      // threads over t, ascending: a thread's last hit is its largest
  for (int t = tid; t < T; t += nt)
    if (has_bit(hard.at(t, 0, gr)[gc >> 6], gc & 63)) hit = t;
  wide_post(s, 0, wave_all_max(hit));
  const int last = wide_max(s, wide_sync(s), 0);
  if (last >= T - 1) return -1;      // the goal is held for ever
  wboard<NW> cur[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cur[k] = tid == sr ? wb_bit<NW>(sc) : wb_zero<NW>();
    wecbs_plane<NW>{planes + k * plane_words, nt}.store(0, 0, tid, cur[k]);
  }
  wboard<NW> hd[AHEAD][WECBS_BOARDS], cl[AHEAD][WECBS_BOARDS];      // the hard boards, and hard | soft
#pragma unroll
  for (int i = 0; i < AHEAD; ++i)
#pragma unroll
    for (int b = 0; b < WECBS_BOARDS; ++b) {
      hd[i][b] = 1 + i < T ? hard.load(1 + i, b, tid) : wb_zero<NW>();
      cl[i][b] = hd[i][b];
      if constexpr (K > 1) cl[i][b] = cl[i][b] | (1 + i < T ? soft.load(1 + i, b, tid) : wb_zero<NW>());
    }
  int tstar = -1, bound = T - 1, best_k = K, best_t = -1;
  for (int t0 = 0;; t0 += AHEAD) {
#pragma unroll
    for (int i = 0; i < AHEAD; ++i) {
      const int t = t0 + i;      // cur[k] = P^k_t; hd[i], cl[i] = the boards of layer t + 1
      wboard<NW> h[WECBS_BOARDS], c[WECBS_BOARDS];
      const int tn = t + 1 + AHEAD;
#pragma unroll
      for (int b = 0; b < WECBS_BOARDS; ++b) {
        h[b] = hd[i][b], c[b] = cl[i][b];
        hd[i][b] = tn < T ? hard.load(tn, b, tid) : wb_zero<NW>();
        cl[i][b] = hd[i][b];
        if constexpr (K > 1) cl[i][b] = cl[i][b] | (tn < T ? soft.load(tn, b, tid) : wb_zero<NW>());
      }
      // one round: the fronts' boundary rows and the votes
      int mine = (int)wb_any(cur[K - 1]) << 4;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        mine |= (int)(tid == gr && wb_has(cur[k], gc)) << k;
        wide_seat sk = s;
        if (k != K - 2 || K == 1) {      // (plane K - 2 drops into plane K - 1, which takes no drops)
          sk.mail = s.mail + k;
          wide_post_rows(sk, cur[k] & ~h[3], cur[k] & ~h[1]);
        }
        if (k + 1 < K) {
          sk.mail = s.mail + K + k;
          wide_post_rows(sk, cur[k] & ~c[3], cur[k] & ~c[1]);
        }
      }
      wide_post(s, 0, wave_all_or(mine));
      const int p = wide_sync(s);
      const int votes = wide_or(s, p, 0);
      if (tstar < 0) {
        if (t > last && (votes >> (K - 1) & 1)) {
          tstar = t;
          const long long b = (long long)w_milli * t / 1000;
          bound = b < T - 1 ? (int)b : T - 1;
        } else if (t == T - 1 || !(votes & 16)) {
          return -1;
        }
      }
      if (tstar >= 0) {
        const int goal_in = votes & ((1 << K) - 1);
        if (goal_in) {
          const int k = __builtin_ctz(goal_in);
          if (k < best_k) best_k = k, best_t = t;
        }
        if (best_k == 0 || t == bound) {
          *k_out = best_k, *t_out = best_t;
          return tstar;
        }
      }
      wboard<NW> nxt[K];
      {
        wide_seat sk = s;
        sk.mail = s.mail + (K - 1);
        nxt[K - 1] = wecbs_step(cur[K - 1], free, h, wide_cells_up(sk, p, cur[K - 1] & ~h[3]), wide_cells_down(sk, p, cur[K - 1] & ~h[1]));
      }
#pragma unroll
      for (int k = 0; k + 1 < K; ++k) {
        wide_seat sk = s;
        sk.mail = s.mail + K + k;
        nxt[k] = wecbs_step(cur[k], free, c, wide_cells_up(sk, p, cur[k] & ~c[3]), wide_cells_down(sk, p, cur[k] & ~c[1]));
        if (k >= 1) {
          sk.mail = s.mail + (k - 1);
          nxt[k] = nxt[k] | wecbs_step(cur[k - 1], free, h, wide_cells_up(sk, p, cur[k - 1] & ~h[3]),
                                       wide_cells_down(sk, p, cur[k - 1] & ~h[1]));
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        cur[k] = nxt[k];
        wecbs_plane<NW>{planes + k * plane_words, nt}.store(t + 1, 0, tid, cur[k]);
      }
    }
  }
}

// this thread's candidates for the move INTO (r, c), bits up, left, down, right, stop: the source cell is in `prev` and, for a
// real move, not in A_opp(d).  Each candidate is tested by the thread of its row.
template <int NW>
__device__ __forceinline__ int wecbs_sources(const wboard<NW>& prev, const wboard<NW>& a_up, const wboard<NW>& a_left,
                                             const wboard<NW>& a_down, const wboard<NW>& a_right, int r, int c, int W, int tid) {
  const bool up = tid == r + 1 && wb_has(prev & ~a_down, c);                      // moved up: came from the row below
  const bool left = tid == r && c + 1 < W && wb_has(prev & ~a_right, c + 1 < W ? c + 1 : c);
  const bool down = tid == r - 1 && wb_has(prev & ~a_up, c);
  const bool right = tid == r && c >= 1 && wb_has(prev & ~a_left, c >= 1 ? c - 1 : c);
  const bool stop = tid == r && wb_has(prev, c);
  return (int)up | (int)left << 1 | (int)down << 2 | (int)right << 3 | (int)stop << 4;
}
__device__ __forceinline__ int wecbs_first(int bits) {      // the first of up, left, down, right, stop - or -1
  return bits & 1 ? 0 : bits & 2 ? 1 : bits & 4 ? 2 : bits & 8 ? 3 : bits & 16 ? 4 : -1;
}

// Walks from (goal, t, plane k) down to t = 1, by the narrow form's rule.  In plane K - 1: any hard-allowed source in
// P^(K-1)_(t-1).  In a plane below it: first a source in P^k_(t-1) whose step is clean - none when the cell is in soft V[t], where
// it can only have been reached by a drop - else a hard-allowed source in P^(k-1)_(t-1), and on in plane k - 1.  Only the threads
// of the rows r - 1, r, r + 1 load anything.  Thread 0 writes the cells.
template <int NW, int K>
__device__ void wecbs_backtrace(const wecbs_set<NW>& hard, const wecbs_set<NW>& soft, const u64* planes, long long plane_words,
                                wide_seat& s, int* cells, int gr, int gc, int k, int t, int W, int tid, int nt) {
  int r = gr, c = gc;
  if (tid == 0) cells[t] = r << 8 | c;
  for (; t >= 1; --t) {
    int mine = 0;
    if (tid >= r - 1 && tid <= r + 1) {
      wboard<NW> h[4], hs[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        h[b] = hard.load(t, 1 + b, tid);
        hs[b] = h[b];
        if constexpr (K > 1) hs[b] = hs[b] | soft.load(t, 1 + b, tid);
      }
      const wboard<NW> here = wecbs_plane<NW>{const_cast<u64*>(planes) + k * plane_words, nt}.load(t - 1, 0, tid);
      if (k == K - 1) {
        mine = wecbs_sources(here, h[0], h[1], h[2], h[3], r, c, W, tid);
      } else {
        mine = wecbs_sources(here, hs[0], hs[1], hs[2], hs[3], r, c, W, tid);
        if (k >= 1) {
          const wboard<NW> below = wecbs_plane<NW>{const_cast<u64*>(planes) + (k - 1) * plane_words, nt}.load(t - 1, 0, tid);
          mine |= wecbs_sources(below, h[0], h[1], h[2], h[3], r, c, W, tid) << 5;
        }
        if constexpr (K > 1) mine |= (int)(tid == r && wb_has(soft.load(t, 0, tid), c)) << 10;
      }
    }
    wide_post(s, 0, wave_all_or(mine));
    const int votes = wide_or(s, wide_sync(s), 0);
    int mv = -1;
    if (k == K - 1) {
      mv = wecbs_first(votes & 31);
    } else {
      if (!(votes >> 10 & 1)) mv = wecbs_first(votes & 31);
      if (mv < 0 && k >= 1) {
        mv = wecbs_first(votes >> 5 & 31);
        --k;
      }
    }
    if (mv == 0) r += 1;
    else if (mv == 1) c += 1;
    else if (mv == 2) r -= 1;
    else if (mv == 3) c -= 1;
    if (tid == 0) cells[t - 1] = r << 8 | c;
  }
}

template <int NW, int K>
struct wecbs_form : wide_group<NW> {
  static constexpr bool FOCAL = true, BORROWS_GRIDS = false;
  wecbs_set<NW> hard, soft;
  u64* planes;
  long long plane_words;
  int *own0, *own1;
  int T, W, w_milli, ka, ta;
  using wide_group<NW>::tid;
  using wide_group<NW>::nt;
  using wide_group<NW>::s;
  using wide_group<NW>::free;
  __device__ __forceinline__ bool screen(const int* st, const int* gl, int N, int H, int W) {      // one round per agent
    wboard<NW> starts = wb_zero<NW>(), goals = wb_zero<NW>();
    bool ok = true;
    for (int a = 0; a < N && ok; ++a) {
      const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
      const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
      const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
      const int scc = inside ? sc : 0, gcc = inside ? gc : 0;
      const bool s_ok = inside && tid == sr && wb_has(free & ~starts, scc), g_ok = inside && tid == gr && wb_has(free & ~goals, gcc);
      wide_post(s, 0, (int)wave_any(s_ok) | (int)wave_any(g_ok) << 1);
      ok = wide_or(s, wide_sync(s), 0) == 3;
      if (inside && tid == sr) starts = starts | wb_bit<NW>(scc);
      if (inside && tid == gr) goals = goals | wb_bit<NW>(gcc);
    }
    return ok;
  }
  template <bool SET>
  __device__ __forceinline__ void mark(int board, int t, int r, int c) const {
    wecbs_mark<SET>(hard, board, t, r, c, tid);
  }
  template <bool SET>
  __device__ __forceinline__ void reserve(const int* p) const {
    if constexpr (K > 1) wecbs_reserve<SET>(soft, p, T, tid, nt);
  }
  template <bool CHILD>
  __device__ __forceinline__ int search(int sr, int sc, int gr, int gc) {
    // (the seat and the arrival go in as locals of their own: the inliner weighs the call by what it can keep in registers, as it
    // did when they were the kernel's locals, and a member of the form counts for that only as long as every other member does)
    wide_seat seat = s;
    int k_arrival = 0, t_arrival = 0;
    const int tstar = wecbs_search<NW, K>(hard, soft, planes, plane_words, seat, free, sr, sc, gr, gc, T, w_milli, tid, nt, &k_arrival, &t_arrival);
    s = seat, ka = k_arrival, ta = t_arrival;
    return tstar;
  }
  template <bool CHILD>
  __device__ __forceinline__ void trace(int* cells, int gr, int gc) {
    wecbs_backtrace<NW, K>(hard, soft, planes, plane_words, s, cells, gr, gc, ka, ta, W, tid, nt);
  }
};

template <int NW, int K>
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_ecbs_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                               const int* __restrict__ start, const int* __restrict__ goal, int* paths,
                                                               int* lengths, int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                               int* __restrict__ status, int* __restrict__ flowtime,
                                                               int* __restrict__ lower_bound, int* __restrict__ nodes_out,
                                                               int* __restrict__ expanded_out, int* __restrict__ horizon_hit,
                                                               u64* workspace, int N, int T, int max_nodes, int w_milli) {
  __shared__ wide_mail mails[WECBS_MAILS];
  __shared__ int cells[WMAPF_MAX_T];
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const wecbs_layout lay = wecbs_case_layout(H, W, N, T, max_nodes, K);
  u64* mine = workspace + (long long)cs * lay.words;
  int* ints = reinterpret_cast<int*>(mine + lay.ints);      // rlen, rts, src, the two cell rows: N ints each
  int* own = reinterpret_cast<int*>(mine + lay.grids);
  const long long a0 = (long long)cs * N;
  const tree_case<ecbs_node> k{start + a0 * 2, goal + a0 * 2, paths + a0 * T * 2, lengths + a0,
                               reinterpret_cast<uint16_t*>(mine + lay.root), reinterpret_cast<uint16_t*>(mine + lay.npath),
                               reinterpret_cast<ecbs_node*>(mine + lay.nodes), ints, ints + N, ints + 2 * N, ints + 3 * N, cells,
                               N, T, H, W, max_nodes, w_milli};
  for (long long i = tid; i < lay.planes; i += nt) mine[i] = 0ull;      // both sets of boards
  wecbs_form<NW, K> f{wide_group_of<NW>(mails, tid, nt), wecbs_set<NW>{mine, nt}, wecbs_set<NW>{mine + lay.soft, nt},
                      mine + lay.planes, (long long)T * nt * NW, own, own + H * W, T, W, w_milli, 0, 0};
  f.load_free(map + cs * map_stride, H, W);
  mapf_tree_search(f, k, tree_out{makespan, solved, status, flowtime, lower_bound, nodes_out, expanded_out, horizon_hit}, cs);
}

}  // namespace

extern "C" size_t magat_sim_mapf_ecbs_wide_workspace_bytes(int C, int H, int W, int N, int T, int max_nodes, int levels) {
  if (C <= 0 || H <= 0 || W <= 0 || N <= 0 || T <= 0 || max_nodes <= 0 || levels <= 0 || H > WIDE_SIDE || W > WIDE_SIDE ||
      N > AUDIT_MAX_N || T > WMAPF_MAX_T || max_nodes > ECBS_MAX_NODES || levels > ECBS_MAX_LEVELS)
    return 0;
  return (size_t)C * (size_t)wecbs_case_layout(H, W, N, T, max_nodes, levels).words * sizeof(u64);
}

extern "C" int magat_sim_mapf_ecbs_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                                        int32_t* paths, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                                        int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                                        void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, int w_milli,
                                        int levels, void* stream) {
  const int rc = tree_entry_check({map, start, goal, paths, lengths, makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit},
                                  H, W, C, N, T, max_nodes, levels > 0 && w_milli >= 1000, levels <= ECBS_MAX_LEVELS && w_milli <= ECBS_MAX_W_MILLI,
                                  WIDE_SIDE, WMAPF_MAX_T, ECBS_MAX_NODES, workspace, workspace_bytes,
                                  magat_sim_mapf_ecbs_wide_workspace_bytes(C, H, W, N, T, max_nodes, levels));
  if (rc != MAGAT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_MAPF_ECBS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_ECBS, st);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
#define WECBS_LAUNCH(NW, K)                                                                                                          \
  hipLaunchKernelGGL((wmapf_ecbs_kernel<NW, K>), grid, block, 0, st, map, stride, H, W, start, goal, paths, lengths, makespan, solved, \
                     status, flowtime, lower_bound, nodes, expanded, horizon_hit, ws, N, T, max_nodes, w_milli)
#define WECBS_LEVELS(NW)             \
  if (levels == 1) WECBS_LAUNCH(NW, 1);      \
  else if (levels == 2) WECBS_LAUNCH(NW, 2); \
  else if (levels == 3) WECBS_LAUNCH(NW, 3); \
  else WECBS_LAUNCH(NW, 4)
  switch (wide_words(W)) {      // static LDS only: the mails and the traced path
    case 1:
      WECBS_LEVELS(1);
      break;
    case 2:
      WECBS_LEVELS(2);
      break;
    default:
      WECBS_LEVELS(4);
      break;
  }
#undef WECBS_LEVELS
#undef WECBS_LAUNCH
  magat_prof_end(pid, st);
  return magat_check_launch();
}
