// A bounded-suboptimal multi-agent path-finding expert for C cases at once: enhanced conflict-based search (ECBS) on the device -
// conflict-based search with a focal search on both levels (the rule is in include/magat_hip.h, restated cell by cell
// in tests/ecbs_restatement.py).  A solved case promises 1000 * flowtime <= w_milli * lower_bound <= w_milli * optimum.
//   magat_sim_mapf_ecbs_workspace_bytes   per case: hard and soft boards, the planes, the root's paths, the node pool, five int rows
//   magat_sim_mapf_ecbs                   one wavefront per case runs the whole tree; one launch, no host round trip
// The layout of mapf_cbs_kernel (sim_mapf_cbs.hip): lane = map row, one 64-bit word per row.  Per case:
//   hard boards    workspace [t][V, A_up, A_left, A_down, A_right][row]: the constraints of the agent that is searched, as in CBS.
//   soft boards    a second set: the planner's reservation of every OTHER agent of the schedule the search runs against, set
//                  before a search and cleared after it by lanes over t (a lane owns the words of its t).
//   planes         workspace [k][t][row], K = levels of them: plane K - 1 is the planner's R on the hard boards, plane k below it
//                  the cells reached with at most k steps that break a soft board.  A lane reads back only the rows it wrote.
//   node pool      workspace: 32 bytes per node (parent, cost, lb, hc, agent | board | open | length, t | cell, t*) and its agent's
//                  new path, T cells of 16 bits; the root's N paths, lengths and t* beside it.
//   schedule       assembled into `paths` / `lengths` themselves, as in CBS; `src` remembers which node gave an agent its path.
//   LDS            the two cell-owner grids of the conflict scan and the conflict count (32 KB) and the path just traced (1 KB).
//   open list      two linear scans by the wave: the smallest lb, then the smallest (hc, cost, index) inside the focal bound.
// Integer and bit arithmetic only.  Every store is a per-lane (vector) store or an LDS atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_MAX_N, AUDIT_NONE, audit_stage2
#include "sim_mapf_cbs_parts.h"        // cbs_wave_min / _max, cbs_mark, cbs_mark_chain, cbs_place
#include "sim_mapf_ecbs_parts.h"       // ECBS_*, ecbs_node, ecbs_wave_sum, ecbs_count
#include "sim_mapf_parts.h"            // MAPF_*, board_row

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
__global__ __launch_bounds__(64) void mapf_ecbs_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                       const int* __restrict__ start, const int* __restrict__ goal, int* paths,
                                                       int* lengths, int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                       int* __restrict__ status, int* __restrict__ flowtime,
                                                       int* __restrict__ lower_bound, int* __restrict__ nodes_out,
                                                       int* __restrict__ expanded_out, int* __restrict__ horizon_hit, u64* workspace,
                                                       int N, int T, int max_nodes, int w_milli) {
  __shared__ int own[2 * ECBS_GRID];              // the owner grids of the conflict scan and the conflict count
  __shared__ int cells[MAPF_MAX_T];               // the path just traced
  const int cs = blockIdx.x, lane = threadIdx.x;
  const ecbs_layout lay = ecbs_case_layout(N, T, max_nodes, K);
  u64* hard = workspace + (long long)cs * lay.words;
  u64* soft = hard + lay.soft;
  u64* P = hard + lay.planes;
  uint16_t* root = reinterpret_cast<uint16_t*>(hard + lay.root);
  uint16_t* npath = reinterpret_cast<uint16_t*>(hard + lay.npath);
  ecbs_node* nodes = reinterpret_cast<ecbs_node*>(hard + lay.nodes);
  int* rlen = reinterpret_cast<int*>(hard + lay.ints);      // the root's lengths
  int* rts = rlen + N;                                       // the root's t*
  int* src = rts + N;                                        // the node an agent's row of the schedule came from; 0: the root
  int* at = src + N;
  const long long a0 = (long long)cs * N;
  int* len = lengths + a0;
  int* rows = paths + a0 * T * 2;
  const int *st = start + a0 * 2, *gl = goal + a0 * 2;
  for (long long i = lane; i < lay.planes; i += 64) hard[i] = 0ull;      // both sets of boards
  for (int i = lane; i < 2 * ECBS_GRID; i += 64) own[i] = AUDIT_NONE;
  const uint8_t* mp = map + cs * map_stride;
  u64 free = 0ull;
  for (int r = 0; r < H; ++r) {
    const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] == 0);
    if (lane == r) free = word;
  }
  int state = -1, count = 0, expanded = 0, hit = 0;      // state: the status once it is known
  // screening: every start and goal on a free cell of its own, before any cell indexes anything
  u64 starts = 0ull, goals = 0ull;
  for (int a = 0; a < N && state < 0; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
    const u64 sbit = inside ? 1ull << sc : 0ull, gbit = inside ? 1ull << gc : 0ull;
    const bool ok = wave_any(lane == sr && (free & ~starts & sbit)) && wave_any(lane == gr && (free & ~goals & gbit));
    if (!ok) state = 3;
    if (lane == sr) starts |= sbit;
    if (lane == gr) goals |= gbit;
  }
  __syncthreads();      // the cleared boards
  // the root: the agents in index order, each against the soft boards of those before it
  int cost = 0, lb = 0;
  for (int a = 0; a < N && state < 0; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    int ka = 0, ta = 0;
    const int tstar = ecbs_search<K>(hard, soft, P, free, sr, sc, gr, gc, T, w_milli, lane, &ka, &ta);
    if (tstar < 0) {
      state = 2, hit = 1;
      break;
    }
    __syncthreads();
    ecbs_backtrace<K>(hard, soft, P, cells, gr, gc, ka, ta, T, W, lane);
    __syncthreads();
    for (int t = lane; t <= ta; t += 64) root[(long long)a * T + t] = (uint16_t)cells[t];
    if (lane == 0) rlen[a] = len[a] = ta + 1, rts[a] = tstar;
    cost += ta, lb += tstar;
    __syncthreads();      // the path is read by other lanes; `cells` is traced again
    cbs_place(rows + (long long)a * T * 2, root + (long long)a * T, ta + 1, T, lane);
    __syncthreads();
    if constexpr (K > 1) {
      ecbs_reserve<true>(soft, rows + (long long)a * T * 2, T, lane);
      __syncthreads();
    }
  }
  if (state < 0) {
    if constexpr (K > 1) {
      for (int a = 0; a < N; ++a) ecbs_reserve<false>(soft, rows + (long long)a * T * 2, T, lane);
    }
    int span = 0;
    for (int base = 0; base < N; base += 64) {
      const int b = base + lane, l = b < N ? len[b] : 1;
      span = l > span ? l : span;
    }
    span = cbs_wave_max(span);
    const int hc = ecbs_count(rows, N, T, W, span, own, own + ECBS_GRID, at, at + N, lane, 64, ecbs_wave_sum);
    if (lane == 0) nodes[0] = ecbs_node{-1, cost, lb, hc, ECBS_OPEN, 0, 0, 0};
    count = 1;
  }
  int best_cost = 0, lbmin = -1;
  while (state < 0) {
    __syncthreads();      // the nodes, their paths, the cleared boards
    // the smallest lb of the open list, then the smallest (hc, cost, index) among the open nodes inside w * that
    int lo = AUDIT_NONE;
    for (int i = lane; i < count; i += 64) {
      const ecbs_node nd = nodes[i];
      if ((nd.who & ECBS_OPEN) && nd.lb < lo) lo = nd.lb;
    }
    lo = cbs_wave_min(lo);
    if (lo == AUDIT_NONE) {
      state = 2;
      break;
    }
    lbmin = lo;
    int bh = AUDIT_NONE, bc = AUDIT_NONE, bi = AUDIT_NONE;
    for (int i = lane; i < count; i += 64) {
      const ecbs_node nd = nodes[i];
      if (!(nd.who & ECBS_OPEN) || 1000LL * nd.cost > (long long)w_milli * lo) continue;
      if (nd.hc < bh || (nd.hc == bh && nd.cost < bc)) bh = nd.hc, bc = nd.cost, bi = i;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const int oh = __shfl_xor(bh, off, 64), oc = __shfl_xor(bc, off, 64), oi = __shfl_xor(bi, off, 64);
      if (oh < bh || (oh == bh && (oc < bc || (oc == bc && oi < bi)))) bh = oh, bc = oc, bi = oi;
    }
    if (bi == AUDIT_NONE) {      // (the node that gives the smallest lb is inside the bound: not reached)
      state = 2;
      break;
    }
    best_cost = bc;
    const int blb = __builtin_amdgcn_readfirstlane(nodes[bi].lb);
    __syncthreads();      // everybody has read the node before it is closed
    if (lane == 0) nodes[bi].who &= ~ECBS_OPEN;
    // its schedule: the first node of the chain that names an agent holds its path, the root the others'
    u64 named = 0ull;      // agents 64 * lane .. 64 * lane + 63
    for (int i = bi; i > 0; i = __builtin_amdgcn_readfirstlane(nodes[i].parent)) {
      const int who = __builtin_amdgcn_readfirstlane(nodes[i].who), x = who & 4095;
      if (wave_any(lane == (x >> 6) && has_bit(named, x & 63))) continue;
      if (lane == (x >> 6)) named |= 1ull << (x & 63);
      const int lx = (who >> 16 & 255) + 1;
      cbs_place(rows + (long long)x * T * 2, npath + (long long)i * T, lx, T, lane);
      if (lane == 0) len[x] = lx, src[x] = i;
    }
    for (int a = 0; a < N; ++a) {
      if (wave_any(lane == (a >> 6) && has_bit(named, a & 63))) continue;
      const int la = __builtin_amdgcn_readfirstlane(rlen[a]);
      cbs_place(rows + (long long)a * T * 2, root + (long long)a * T, la, T, lane);
      if (lane == 0) len[a] = la, src[a] = 0;
    }
    __syncthreads();
    int t2 = -1;
    const int key2 = audit_stage2(rows, N, T, W, own, own + ECBS_GRID, at, at + N, lane, 64, [](int key) {
      key = cbs_wave_min(key);
      __syncthreads();
      return key;
    }, &t2);
    if (key2 == AUDIT_NONE) {
      state = 0;
      break;
    }
    if (count + 2 > max_nodes) {
      state = 1;
      break;
    }
    ++expanded;
    __syncthreads();      // the scan's reads of the grids lie behind
    for (int i = lane; i < H * W; i += 64) own[i] = own[ECBS_GRID + i] = AUDIT_NONE;
    const int kind = key2 & 1;
    for (int k = 0; k < 2; ++k) {
      const int x = k ? key2 >> 1 & 4095 : key2 >> 13, child = count + k;
      const int lx = __builtin_amdgcn_readfirstlane(len[x]), from = __builtin_amdgcn_readfirstlane(src[x]);
      const int tx = from ? __builtin_amdgcn_readfirstlane(nodes[from].tstar) : __builtin_amdgcn_readfirstlane(rts[x]);
      int* px = rows + (long long)x * T * 2;
      const int th = t2 < lx ? t2 : lx - 1;
      int cr = __builtin_amdgcn_readfirstlane(px[2 * th]), cc = __builtin_amdgcn_readfirstlane(px[2 * th + 1]), board = 0;
      if (kind) {      // its own step at t2: from (fr, fc) in direction d - closed by bit (fr, fc) of A_opp(d)[t2]
        const int fr = __builtin_amdgcn_readfirstlane(px[2 * t2 - 2]), fc = __builtin_amdgcn_readfirstlane(px[2 * t2 - 1]);
        const int dr = cr - fr, dc = cc - fc, d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : 3;
        board = 1 + ((d + 2) & 3), cr = fr, cc = fc;
      }
      cbs_mark<true>(hard, board, t2, cr, cc, lane);
      cbs_mark_chain<true>(hard, nodes, bi, x, lane);
      if constexpr (K > 1) {
        for (int o = 0; o < N; ++o)
          if (o != x) ecbs_reserve<true>(soft, rows + (long long)o * T * 2, T, lane);
      }
      __syncthreads();
      const int sr = __builtin_amdgcn_readfirstlane(st[2 * x]), sc = __builtin_amdgcn_readfirstlane(st[2 * x + 1]);
      const int gr = __builtin_amdgcn_readfirstlane(gl[2 * x]), gc = __builtin_amdgcn_readfirstlane(gl[2 * x + 1]);
      int ka = 0, ta = 0;
      const int tstar = ecbs_search<K>(hard, soft, P, free, sr, sc, gr, gc, T, w_milli, lane, &ka, &ta);
      __syncthreads();
      if (tstar >= 0) {
        ecbs_backtrace<K>(hard, soft, P, cells, gr, gc, ka, ta, T, W, lane);
        __syncthreads();
        for (int t = lane; t <= ta; t += 64) npath[(long long)child * T + t] = (uint16_t)cells[t];
      } else {
        hit = 1;
      }
      __syncthreads();      // every load of the boards lies behind; the child's path is read by other lanes
      cbs_mark<false>(hard, board, t2, cr, cc, lane);
      cbs_mark_chain<false>(hard, nodes, bi, x, lane);
      if constexpr (K > 1) {
        for (int o = 0; o < N; ++o)
          if (o != x) ecbs_reserve<false>(soft, rows + (long long)o * T * 2, T, lane);
      }
      int hc = 0;
      if (tstar >= 0) {      // the child's own schedule: the agent's row replaced, counted, put back
        cbs_place(px, npath + (long long)child * T, ta + 1, T, lane);
        if (lane == 0) len[x] = ta + 1;
        __syncthreads();
        int span = 0;
        for (int base = 0; base < N; base += 64) {
          const int b = base + lane, l = b < N ? len[b] : 1;
          span = l > span ? l : span;
        }
        span = cbs_wave_max(span);
        hc = ecbs_count(rows, N, T, W, span, own, own + ECBS_GRID, at, at + N, lane, 64, ecbs_wave_sum);
        cbs_place(px, from ? npath + (long long)from * T : root + (long long)x * T, lx, T, lane);
        if (lane == 0) len[x] = lx;
      }
      if (lane == 0)
        nodes[child] = ecbs_node{bi, tstar >= 0 ? bc - (lx - 1) + ta : -1, tstar >= 0 ? blb - tx + tstar : -1, hc,
                                 x | board << 12 | (tstar >= 0 ? ECBS_OPEN | ta << 16 : 0), t2 | cr << 16 | cc << 24,
                                 tstar >= 0 ? tstar : 0, 0};
      __syncthreads();
    }
    count += 2;
  }
  // the answer stands in paths / lengths already; every other case gets the start cells
  int longest = 0;
  if (state == 0) {
    __syncthreads();
    for (int base = 0; base < N; base += 64) {
      const int b = base + lane, l = b < N ? len[b] : 1;
      longest = l - 1 > longest ? l - 1 : longest;
    }
    longest = cbs_wave_max(longest);
  } else {
    __syncthreads();      // the conflict scan has read the rows
    for (int a = 0; a < N; ++a) {
      const int sr = st[2 * a], sc = st[2 * a + 1];
      int* p = rows + (long long)a * T * 2;
      for (int t = lane; t < T; t += 64) {
        p[2 * t] = sr;
        p[2 * t + 1] = sc;
      }
      if (lane == 0) len[a] = 1;
    }
  }
  if (lane == 0) {
    makespan[cs] = longest;
    solved[cs] = state == 0 ? 1 : 0;
    status[cs] = state;
    flowtime[cs] = state == 0 ? best_cost : -1;
    lower_bound[cs] = state <= 1 ? lbmin : -1;
    nodes_out[cs] = count;
    expanded_out[cs] = expanded;
    horizon_hit[cs] = hit;
  }
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
  if (!map || !start || !goal || !paths || !lengths || !makespan || !solved || !status || !flowtime || !lower_bound || !nodes ||
      !expanded || !horizon_hit || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0 || max_nodes <= 0 || levels <= 0 || w_milli < 1000) return MAGAT_ERR_BAD_SHAPE;
  if (H > MAPF_SIDE || W > MAPF_SIDE || T > MAPF_MAX_T || N > AUDIT_MAX_N || max_nodes > ECBS_MAX_NODES || levels > ECBS_MAX_LEVELS ||
      w_milli > ECBS_MAX_W_MILLI)
    return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_ecbs_workspace_bytes(C, N, T, max_nodes, levels)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
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
