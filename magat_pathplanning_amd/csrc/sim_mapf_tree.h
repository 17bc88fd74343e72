// The high-level search of the three tree experts - CBS (sim_mapf_cbs.hip), ECBS (sim_mapf_ecbs.hip) and wide ECBS
// (sim_mapf_ecbs_wide.hip) - once: screen, root, then pick / close / rebuild the schedule / find the first conflict / branch into two
// children, and the results (the rules are in include/magat_hip.h, restated in tests/cbs_restatement.py and
// tests/ecbs_restatement.py).  One workgroup per case runs mapf_tree_search; the kernel carves the workspace, zeroes its boards and
// hands in a form, which brings what differs between the three:
//   tid, nt, own0, own1     the workgroup (nt = 64: one wavefront) and the two cell-owner grids of the conflict scan, where the form
//                           keeps them: dynamic LDS (CBS), static LDS (ECBS), the workspace (wide ECBS)
//   group_min / _max / _sum (from the form's group, sim_group.h: wave_group or wide_group<NW>) a reduction over the workgroup
//                           BEHIND A BARRIER of the whole workgroup, the same value in every thread;
//   group_min3              the lexicographically smallest int triple.  One wave: the butterfly.  Wide: the LDS mail - every thread
//                           goes through the same sequence of wide_sync, so the walk calls them under uniform conditions only
//   screen                  every start and goal on a free cell of its own, before any cell indexes anything
//   mark<SET>               one constraint bit;  reserve<SET>: a schedule row on the soft boards (nothing where there are none)
//   search<CHILD>, trace    the low-level search of one agent under the boards as they stand; it leaves the arrival step in `ta`
//                           (and what else the trace needs in the form) and returns t*, or -1
//   FOCAL                   the rule.  false: the open node with the smallest (cost, index); no lb / hc / t*; the bound of a spent
//                           budget is that cost; 16-byte nodes with length - 1 packed into `who`.  true: the smallest lb first, then
//                           the smallest (hc, cost, index) inside 1000 cost <= w_milli lb; the bound is that lb; every node's schedule
//                           is counted (ecbs_count); 32-byte nodes with length - 1 in `len1`
//   BORROWS_GRIDS           the search overwrites the memory of the owner grids (CBS: its R layers)
// The owner grids are all AUDIT_NONE between two uses: the walk clears them at the start, after a conflict scan that stopped early,
// and after every search of a form that borrows them.  ecbs_count leaves them clean itself.
// The barriers (the union of what the three kernels had; one on a single wavefront costs next to nothing), and what each protects:
//   after screening         the boards the kernel zeroed, the cleared grids
//   search | trace          the planes are read across rows;  trace | copy: `cells` is read by other threads
//   after a root path       the path is placed by other threads, `cells` is traced again;  placed | reserved | next search
//   top of the loop         the nodes, their paths, the cleared boards and grids
//   pick | close | rebuild  everybody has read the node before it is closed, and sees it closed
//   rebuild | scan          the schedule rows and lengths;  scan | clearing the grids: the scan's reads lie behind
//   marks, reservations | search | (trace | copy) | unmark, unreserve: every load of the boards lies behind, the child's path is read
//   unreserve | the child's row replaced: the reservations were read from the row;  replaced | counted;  node written | next child
// Every branch around a barrier is uniform over the workgroup: its condition comes out of a group reduction or is read from one
// address by all threads.  Every store is a per-thread (vector) store or an atomic from plain C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_NONE, audit_stage2
#include "sim_mapf_cbs_parts.h"        // cbs_mark_chain, cbs_place
#include "sim_mapf_ecbs_parts.h"       // ecbs_node, ecbs_count

constexpr int TREE_OPEN = 1 << 15;      // in a node's `who`: agent | board << 12 | open << 15

struct cbs_node {
  int parent;
  int cost;      // the flowtime of the node's schedule; -1: the child found no arrival
  int who;       // agent | board << 12 | open << 15 | (length - 1) << 16
  int what;      // the constraint: t | row << 16 | col << 24
};

// one case: its slices of the inputs and outputs, and of the workspace what the walk itself reads and writes
template <class Node>
struct tree_case {
  const int *st, *gl;          // start and goal cells
  int *rows, *len;             // `paths` and `lengths`: the schedule of the node at hand is assembled here (the outputs are the scratch)
  uint16_t *root, *npath;      // the root's N paths and every node's new path, T cells of 16 bits (row << 8 | col)
  Node* nodes;
  int *rlen, *rts, *src;       // the root's lengths; focal: the root's t*, and the node an agent's row came from (0: the root)
  int* at;                     // the cell of every agent at two steps, 2 N ints
  int* cells;                  // LDS: the path just traced
  int N, T, H, W, max_nodes, w_milli;
};
struct tree_out {
  int* makespan;
  uint8_t* solved;
  int *status, *flowtime, *lower_bound, *nodes, *expanded, *horizon_hit;
};

template <class Form>
__device__ __forceinline__ void tree_clear_grids(Form& f, int cells) {
  for (int i = f.tid; i < cells; i += f.nt) f.own0[i] = f.own1[i] = AUDIT_NONE;
}
// max over the agents of len, at least 1
template <class Form>
__device__ __forceinline__ int tree_span(Form& f, const int* len, int N) {
  int span = 1;
  for (int b = f.tid; b < N; b += f.nt) span = len[b] > span ? len[b] : span;
  return f.group_max(span);
}
// ---- the rule: everything FOCAL decides, but the root's soft boards ----------------------------------------------------------------
__device__ __forceinline__ int tree_len1(const cbs_node& nd) { return nd.who >> 16 & 255; }
__device__ __forceinline__ int tree_len1(const ecbs_node& nd) { return nd.len1; }
// The open node to expand: its index or AUDIT_NONE, its cost, and the bound the open list gives.  Uniform.
template <class Form, class Node>
__device__ __forceinline__ int tree_pick(Form& f, const Node* nodes, int count, int w_milli, int* cost, int* bound) {
  int lo = 0;
  if constexpr (Form::FOCAL) {
    lo = AUDIT_NONE;
    for (int i = f.tid; i < count; i += f.nt) {
      const Node nd = nodes[i];
      if ((nd.who & TREE_OPEN) && nd.lb < lo) lo = nd.lb;
    }
    lo = f.group_min(lo);
    if (lo == AUDIT_NONE) return AUDIT_NONE;
  }
  int bh = AUDIT_NONE, bc = AUDIT_NONE, bi = AUDIT_NONE;
  for (int i = f.tid; i < count; i += f.nt) {
    const Node nd = nodes[i];
    if (!(nd.who & TREE_OPEN)) continue;
    int hc = 0;
    if constexpr (Form::FOCAL) {
      if (1000LL * nd.cost > (long long)w_milli * lo) continue;
      hc = nd.hc;
    }
    if (hc < bh || (hc == bh && nd.cost < bc)) bh = hc, bc = nd.cost, bi = i;
  }
  f.group_min3(bh, bc, bi);      // (focal: the node that gives the smallest lb is inside the bound, so there is one)
  *cost = bc, *bound = Form::FOCAL ? lo : bc;
  return bi;
}
// hc of the schedule in k.rows with agent x's row replaced by `path` (ta + 1 cells); the row and its length are put back (`from`,
// lx).  Behind a barrier: the reservations were read from the row.
template <class Form, class Node>
__device__ __forceinline__ int tree_count_with(Form& f, const tree_case<Node>& k, int x, const uint16_t* path, int ta,
                                               const uint16_t* from, int lx) {
  int* px = k.rows + (long long)x * k.T * 2;
  __syncthreads();
  cbs_place(px, path, ta + 1, k.T, f.tid, f.nt);
  if (f.tid == 0) k.len[x] = ta + 1;
  __syncthreads();
  const int span = tree_span(f, k.len, k.N);
  const int hc = ecbs_count(k.rows, k.N, k.T, k.W, span, f.own0, f.own1, k.at, k.at + k.N, f.tid, f.nt, [&](int n) { return f.group_sum(n); });
  cbs_place(px, from, lx, k.T, f.tid, f.nt);
  if (f.tid == 0) k.len[x] = lx;
  return hc;
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------
// (always inlined: the form is then the kernel's own local and dissolves into registers)
template <class Form, class Node>
__device__ __forceinline__ void mapf_tree_search(Form& f, const tree_case<Node>& k, const tree_out& out, int cs) {
  constexpr bool FOCAL = Form::FOCAL;
  const int tid = f.tid, nt = f.nt, N = k.N, T = k.T, W = k.W, grid = k.H * k.W;
  const int *st = k.st, *gl = k.gl;
  int *rows = k.rows, *len = k.len, *cells = k.cells;
  Node* nodes = k.nodes;
  tree_clear_grids(f, grid);
  int state = f.screen(st, gl, N, k.H, W) ? -1 : 3;      // state: the status once it is known
  int count = 0, expanded = 0, hit = 0;
  __syncthreads();
  // the root: every agent's path - focal: in index order, each against the soft boards of those before it
  int cost = 0, lb = 0;
  for (int a = 0; a < N && state < 0; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const int tstar = f.template search<false>(sr, sc, gr, gc);
    __syncthreads();
    if (tstar < 0) {
      state = 2, hit = 1;
      break;
    }
    const int ta = f.ta;
    f.template trace<false>(cells, gr, gc);
    __syncthreads();
    for (int t = tid; t <= ta; t += nt) k.root[(long long)a * T + t] = (uint16_t)cells[t];
    if (tid == 0) {
      k.rlen[a] = len[a] = ta + 1;
      if constexpr (FOCAL) k.rts[a] = tstar;
    }
    cost += ta, lb += tstar;
    __syncthreads();
    if constexpr (Form::BORROWS_GRIDS) tree_clear_grids(f, grid);
    if constexpr (FOCAL) {
      cbs_place(rows + (long long)a * T * 2, k.root + (long long)a * T, ta + 1, T, tid, nt);
      __syncthreads();
      f.template reserve<true>(rows + (long long)a * T * 2);
      __syncthreads();
    }
  }
  if (state < 0) {
    int hc = 0;
    if constexpr (FOCAL) {
      for (int a = 0; a < N; ++a) f.template reserve<false>(rows + (long long)a * T * 2);
      const int span = tree_span(f, len, N);
      hc = ecbs_count(rows, N, T, W, span, f.own0, f.own1, k.at, k.at + N, tid, nt, [&](int n) { return f.group_sum(n); });
      if (tid == 0) nodes[0] = Node{-1, cost, lb, hc, TREE_OPEN, 0, 0, 0};
    } else {
      if (tid == 0) nodes[0] = Node{-1, cost, TREE_OPEN, 0};
    }
    count = 1;
  }
  int best_cost = 0, bound = -1;
  while (state < 0) {
    __syncthreads();
    int bc = 0;
    const int bi = tree_pick(f, nodes, count, k.w_milli, &bc, &bound);
    if (bi == AUDIT_NONE) {
      state = 2;
      break;
    }
    best_cost = bc;
    int blb = 0;
    if constexpr (FOCAL) blb = __builtin_amdgcn_readfirstlane(nodes[bi].lb);
    __syncthreads();
    if (tid == 0) nodes[bi].who &= ~TREE_OPEN;
    __syncthreads();
    // its schedule: the first node of the chain that names an agent holds its path, the root the others'.  Every wave keeps the
    // set of the named agents for itself: lane l holds the agents 64 l .. 64 l + 63
    u64 named = 0ull;
    const int lane = tid & 63;
    for (int i = bi; i > 0; i = __builtin_amdgcn_readfirstlane(nodes[i].parent)) {
      const int x = __builtin_amdgcn_readfirstlane(nodes[i].who) & 4095;
      if (wave_any(lane == (x >> 6) && has_bit(named, x & 63))) continue;
      if (lane == (x >> 6)) named |= 1ull << (x & 63);
      const int lx = __builtin_amdgcn_readfirstlane(tree_len1(nodes[i])) + 1;
      cbs_place(rows + (long long)x * T * 2, k.npath + (long long)i * T, lx, T, tid, nt);
      if (tid == 0) {
        len[x] = lx;
        if constexpr (FOCAL) k.src[x] = i;
      }
    }
    for (int a = 0; a < N; ++a) {
      if (wave_any(lane == (a >> 6) && has_bit(named, a & 63))) continue;
      const int la = __builtin_amdgcn_readfirstlane(k.rlen[a]);
      cbs_place(rows + (long long)a * T * 2, k.root + (long long)a * T, la, T, tid, nt);
      if (tid == 0) {
        len[a] = la;
        if constexpr (FOCAL) k.src[a] = 0;
      }
    }
    __syncthreads();
    int t2 = -1;
    const int key2 = audit_stage2(rows, N, T, W, f.own0, f.own1, k.at, k.at + N, tid, nt, [&](int key) { return f.group_min(key); }, &t2);
    if (key2 == AUDIT_NONE) {
      state = 0;
      break;
    }
    if (count + 2 > k.max_nodes) {
      state = 1;
      break;
    }
    ++expanded;
    __syncthreads();
    tree_clear_grids(f, grid);
    const int kind = key2 & 1;
    for (int c = 0; c < 2; ++c) {
      const int x = c ? key2 >> 1 & 4095 : key2 >> 13, child = count + c;
      const int lx = __builtin_amdgcn_readfirstlane(len[x]);
      int from = 0, tx = 0;      // focal: where x's row came from, and its t* there
      if constexpr (FOCAL) {
        from = __builtin_amdgcn_readfirstlane(k.src[x]);
        tx = from ? __builtin_amdgcn_readfirstlane(nodes[from].tstar) : __builtin_amdgcn_readfirstlane(k.rts[x]);
      }
      const int* px = rows + (long long)x * T * 2;
      const int th = t2 < lx ? t2 : lx - 1;
      int cr = __builtin_amdgcn_readfirstlane(px[2 * th]), cc = __builtin_amdgcn_readfirstlane(px[2 * th + 1]), board = 0;
      if (kind) {      // its own step at t2: from (fr, fc) in direction d - closed by bit (fr, fc) of A_opp(d)[t2]
        const int fr = __builtin_amdgcn_readfirstlane(px[2 * t2 - 2]), fc = __builtin_amdgcn_readfirstlane(px[2 * t2 - 1]);
        const int dr = cr - fr, dc = cc - fc, d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : 3;
        board = 1 + ((d + 2) & 3), cr = fr, cc = fc;
      }
      f.template mark<true>(board, t2, cr, cc);
      cbs_mark_chain<true>(f, nodes, bi, x);
      for (int o = 0; o < N; ++o)
        if (o != x) f.template reserve<true>(rows + (long long)o * T * 2);
      __syncthreads();
      const int sr = __builtin_amdgcn_readfirstlane(st[2 * x]), sc = __builtin_amdgcn_readfirstlane(st[2 * x + 1]);
      const int gr = __builtin_amdgcn_readfirstlane(gl[2 * x]), gc = __builtin_amdgcn_readfirstlane(gl[2 * x + 1]);
      const int tstar = f.template search<true>(sr, sc, gr, gc);
      const int ta = f.ta;
      __syncthreads();
      if (tstar >= 0) {
        f.template trace<true>(cells, gr, gc);
        __syncthreads();
        for (int t = tid; t <= ta; t += nt) k.npath[(long long)child * T + t] = (uint16_t)cells[t];
      } else {
        hit = 1;
      }
      __syncthreads();
      f.template mark<false>(board, t2, cr, cc);
      cbs_mark_chain<false>(f, nodes, bi, x);
      for (int o = 0; o < N; ++o)
        if (o != x) f.template reserve<false>(rows + (long long)o * T * 2);
      if constexpr (Form::BORROWS_GRIDS) tree_clear_grids(f, grid);
      const int who = x | board << 12, what = t2 | cr << 16 | cc << 24, ccost = bc - (lx - 1) + ta;
      if constexpr (FOCAL) {
        int hc = 0;
        if (tstar >= 0)
          hc = tree_count_with(f, k, x, k.npath + (long long)child * T, ta, from ? k.npath + (long long)from * T : k.root + (long long)x * T, lx);
        if (tid == 0)
          nodes[child] = tstar >= 0 ? Node{bi, ccost, blb - tx + tstar, hc, who | TREE_OPEN, what, tstar, ta} : Node{bi, -1, -1, 0, who, what, 0, 0};
      } else {
        if (tid == 0) nodes[child] = tstar >= 0 ? Node{bi, ccost, who | TREE_OPEN | ta << 16, what} : Node{bi, -1, who, what};
      }
      __syncthreads();
    }
    count += 2;
  }
  // the answer stands in paths / lengths already; every other case gets the start cells
  int longest = 0;
  __syncthreads();      // the conflict scan has read the rows and lengths
  if (state == 0) {
    longest = tree_span(f, len, N) - 1;
  } else {
    for (int a = 0; a < N; ++a) {
      const int sr = st[2 * a], sc = st[2 * a + 1];
      int* p = rows + (long long)a * T * 2;
      for (int t = tid; t < T; t += nt) {
        p[2 * t] = sr;
        p[2 * t + 1] = sc;
      }
      if (tid == 0) len[a] = 1;
    }
  }
  if (tid == 0) {
    out.makespan[cs] = longest;
    out.solved[cs] = state == 0 ? 1 : 0;
    out.status[cs] = state;
    out.flowtime[cs] = state == 0 ? best_cost : -1;
    out.lower_bound[cs] = state <= 1 ? bound : -1;
    out.nodes[cs] = count;
    out.expanded[cs] = expanded;
    out.horizon_hit[cs] = hit;
  }
}

// ---- the entries ------------------------------------------------------------------------------------------------------------------
// The refusal ladder the three entries share, in its order: a null pointer, a non-positive shape, a limit, the workspace's size, its
// alignment.  An entry brings its own shape and limit conditions (levels, w_milli, its map side and horizon) and the bytes it needs.
inline int tree_entry_check(std::initializer_list<const void*> pointers, int H, int W, int C, int N, int T, int max_nodes,
                            bool own_shape_ok, bool own_limits_ok, int side, int max_t, int node_cap, const void* workspace,
                            size_t workspace_bytes, size_t need) {
  for (const void* p : pointers)
    if (!p) return MAGAT_ERR_NULL;
  if (!workspace) return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0 || max_nodes <= 0 || !own_shape_ok) return MAGAT_ERR_BAD_SHAPE;
  if (H > side || W > side || T > max_t || N > AUDIT_MAX_N || max_nodes > node_cap || !own_limits_ok) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < need) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  return MAGAT_OK;
}
