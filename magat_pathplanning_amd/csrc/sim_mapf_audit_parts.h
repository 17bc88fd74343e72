// What the two forms of the schedule audit (sim_mapf_audit.hip, sim_mapf_audit_wide.hip) share: the packed keys of a fault, the
// per-agent checks of stage 1, the conflict search of stage 2, and audit_walk, the body of both kernels around them.  The rule is
// in include/magat_hip.h and DESIGN 4.11, restated cell by cell in tests/audit_restatement.py.  The forms differ in how a map is
// held (one wave with a word per row, or a workgroup with up to four), so the stages take: is_free(r, c) for a cell ON the map,
// and group_min(key) - the minimum over the workgroup, the same value for every thread, behind a barrier of the whole workgroup
// (sim_group.h; the tree walk of sim_mapf_tree.h runs stage 2 on its own form).
// Every store is a per-lane (vector) store or an atomic from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "sim_entry.h"      // sim_entry_check
#include "sim_group.h"      // u64; the groups

constexpr int AUDIT_MAX_N = 4096;             // agents per case: an agent index takes 12 bits of a key
constexpr int AUDIT_NONE = 0x7fffffff;        // no fault; no owner of a cell

// Stage 1, the key of a fault of agent a: a << 12 | sub, sub in the order in which the agent's checks run - 0: kind 1; 1: kind 2;
// 2: kind 3; 3 + 3 t + (kind - 4) for kinds 4, 5, 6 at t (t < 1024: sub < 3075).  The smallest key is the first fault.
__device__ __forceinline__ int audit_key1(int a, int sub) { return a << 12 | sub; }
__device__ __forceinline__ int audit_min(int a, int b) { return b < a ? b : a; }

// Threads over t for every agent in turn; returns this thread's smallest key.  Every cell is screened before it indexes the
// map; differences are taken in 64 bits, so cells such as (2^30, -2^30) are just cells off the map.
template <typename IsFree>
__device__ int audit_stage1(const int* __restrict__ rows, const int* __restrict__ len, const int* __restrict__ start,
                            const int* __restrict__ goal, int N, int T, int H, int W, int tid, int nt, IsFree is_free) {
  int key = AUDIT_NONE;
  for (int a = 0; a < N; ++a) {
    const int L = len[a];
    if (L < 1 || L > T) {      // kind 1: the agent's other checks are skipped
      key = audit_min(key, audit_key1(a, 0));
      continue;
    }
    const int* p = rows + (long long)a * T * 2;
    const int lr = p[2 * L - 2], lc = p[2 * L - 1];      // the last cell: what the padding has to repeat
    for (int t = tid; t < T; t += nt) {
      const int r = p[2 * t], c = p[2 * t + 1];
      int sub = AUDIT_NONE;
      if (t >= 1) {
        const long long dr = (long long)r - p[2 * t - 2], dc = (long long)c - p[2 * t - 1];
        if (!((dr == 0 && dc >= -1 && dc <= 1) || (dc == 0 && dr >= -1 && dr <= 1))) sub = 3 + 3 * t + 2;      // kind 6
      }
      if (t >= L && (r != lr || c != lc)) sub = 3 + 3 * t + 1;                                                   // kind 5
      const bool inside = r >= 0 && r < H && c >= 0 && c < W;
      if (!inside || !is_free(inside ? r : 0, inside ? c : 0)) sub = 3 + 3 * t;                                  // kind 4
      if (t == L - 1 && (r != goal[2 * a] || c != goal[2 * a + 1])) sub = 2;                                     // kind 3
      if (t == 0 && (r != start[2 * a] || c != start[2 * a + 1])) sub = 1;                                       // kind 2
      if (sub != AUDIT_NONE) key = audit_min(key, audit_key1(a, sub));
    }
  }
  return key;
}

// (kind, t, a, b) of a stage-1 key
__device__ __forceinline__ void audit_fault1(int key, const int* __restrict__ len, int* __restrict__ fault) {
  const int a = key >> 12, sub = key & 4095;
  fault[0] = sub < 3 ? 1 + sub : 4 + (sub - 3) % 3;
  fault[1] = sub == 0 ? -1 : sub == 1 ? 0 : sub == 2 ? len[a] - 1 : (sub - 3) / 3;
  fault[2] = a;
  fault[3] = -1;
}

// Stage 2, on a case that passed stage 1 (every one of the T cells of every agent is on the map): the smallest (t, a, b), a < b,
// with a vertex conflict (kind 7) or a swap (kind 8), as the key a << 13 | b << 1 | (kind - 7) - or AUDIT_NONE - and its t.
// own[0], own[1]: two grids of H * W ints, all AUDIT_NONE going in, for the steps t - 1 and t in turn; at[0], at[1]: the cell
// (r * W + c) of every agent at those steps, N ints each.  Per step, threads over agents: everybody takes
// atomicMin(own[cell], a); a cell's owner is then its smallest agent, and (owner, b) for every b above its owner holds the
// first vertex pair of the step.  No vertex conflict at t - 1 makes that grid one agent per cell, so who stood on a's new cell
// is one lookup, and it swaps with a when it stands on a's old cell now.  Only the cells that were set are cleared.
template <typename GroupMin>
__device__ int audit_stage2(const int* __restrict__ rows, int N, int T, int W, int* own0, int* own1, int* at0, int* at1, int tid,
                            int nt, GroupMin group_min, int* t_out) {
  int *own_cur = own0, *own_prv = own1, *at_cur = at0, *at_prv = at1;
  for (int t = 0; t < T; ++t) {
    for (int a = tid; a < N; a += nt) {
      const int* p = rows + ((long long)a * T + t) * 2;
      const int cell = p[0] * W + p[1];
      at_cur[a] = cell;
      atomicMin(&own_cur[cell], a);
    }
    __syncthreads();
    int key = AUDIT_NONE;
    for (int a = tid; a < N; a += nt) {
      const int cell = at_cur[a], first = own_cur[cell];
      if (first < a) key = audit_min(key, first << 13 | a << 1);
      if (t >= 1) {
        const int from = at_prv[a], b = own_prv[cell];      // b: who stood on a's new cell
        if (from != cell && b != AUDIT_NONE && b > a && at_cur[b] == from) key = audit_min(key, a << 13 | b << 1 | 1);
      }
    }
    key = group_min(key);      // (a barrier: every read of own_prv lies before it)
    if (key != AUDIT_NONE) {
      *t_out = t;
      return key;
    }
    if (t >= 1)
      for (int a = tid; a < N; a += nt) own_prv[at_prv[a]] = AUDIT_NONE;
    __syncthreads();
    int* g = own_cur;
    own_cur = own_prv, own_prv = g;
    g = at_cur;
    at_cur = at_prv, at_prv = g;
  }
  *t_out = -1;
  return AUDIT_NONE;
}

// what thread 0 writes for a case behind its `dist` row; the bounds go out for every case
__device__ __forceinline__ void audit_write(int cs, int* __restrict__ status, int* __restrict__ fault, int* __restrict__ flowtime,
                                            int* __restrict__ makespan, int st, int kind, int t, int a, int b, int flow, int longest) {
  status[cs] = st;
  fault[4 * cs] = kind, fault[4 * cs + 1] = t, fault[4 * cs + 2] = a, fault[4 * cs + 3] = b;
  flowtime[cs] = st == 0 ? flow : -1;
  makespan[cs] = st == 0 ? longest : -1;
}

// ---- the walk: one case, from the free rows to the final write -----------------------------------------------------------------------
// One workgroup per case runs audit_walk.  The kernel hands in a form, which brings what differs between the two: the group
// (sim_group.h), flood(sr, sc, gr, gc) - the steps between two free cells, or -1, the same for every thread - and the two cell-owner
// grids own0, own1 where the form keeps them (LDS, or the workspace).  Every branch around a barrier or a group_* call is uniform.
struct audit_case {
  const uint8_t* map;
  int H, W;
  const uint8_t* solved;      // of the batch, or null
  const int *rows, *len, *st, *gl;
  int* at;                    // the cell of every agent at two steps, 2 N ints
  u64* free_rows;             // LDS, for publish_free
  int N, T;
};
struct audit_out {
  int *status, *fault, *dist, *flow_bound, *span_bound, *flowtime, *makespan;
};

template <class Form>
__device__ __forceinline__ void audit_walk(Form& f, const audit_case& k, const audit_out& out, int cs) {
  const int tid = f.tid, nt = f.nt, N = k.N, T = k.T, H = k.H, W = k.W;
  const int *st = k.st, *gl = k.gl, *len = k.len;
  f.load_free(k.map, H, W);
  f.publish_free(k.free_rows);
  for (int i = tid; i < H * W; i += nt) f.own0[i] = f.own1[i] = AUDIT_NONE;
  __syncthreads();
  const auto is_free = [&](int r, int c) { return f.is_free(r, c); };
  // the bounds: they depend on map, start and goal alone
  int bound = 0, longest = 0;
  bool apart = false;
  for (int a = 0; a < N; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const bool s_in = sr >= 0 && sr < H && sc >= 0 && sc < W, g_in = gr >= 0 && gr < H && gc >= 0 && gc < W;
    int d = -1;
    if (s_in && g_in && is_free(sr, sc) && is_free(gr, gc)) d = f.flood(sr, sc, gr, gc);
    if (tid == 0) out.dist[(long long)cs * N + a] = d;
    apart |= d < 0;
    bound += d;
    longest = d > longest ? d : longest;
  }
  if (tid == 0) {
    out.flow_bound[cs] = apart ? -1 : bound;
    out.span_bound[cs] = apart ? -1 : longest;
  }
  if (k.solved && k.solved[cs] == 0) {
    if (tid == 0) audit_write(cs, out.status, out.fault, out.flowtime, out.makespan, 1, 0, -1, -1, -1, 0, 0);
    return;
  }
  const int key1 = f.group_min(audit_stage1(k.rows, len, st, gl, N, T, H, W, tid, nt, is_free));
  if (key1 != AUDIT_NONE) {
    if (tid == 0) {
      audit_write(cs, out.status, out.fault, out.flowtime, out.makespan, 2, 0, -1, -1, -1, 0, 0);
      audit_fault1(key1, len, out.fault + 4 * cs);
    }
    return;
  }
  int t2 = -1;
  const int key2 = audit_stage2(k.rows, N, T, W, f.own0, f.own1, k.at, k.at + N, tid, nt, [&](int key) { return f.group_min(key); }, &t2);
  int flow = 0, last = 0;
  for (int base = 0; base < N; base += nt) {
    const int b = base + tid, lb = b < N ? len[b] : 1;
    flow += lb - 1;
    last = lb - 1 > last ? lb - 1 : last;
  }
  f.group_sum_max(flow, last);
  if (tid == 0) {
    if (key2 == AUDIT_NONE) audit_write(cs, out.status, out.fault, out.flowtime, out.makespan, 0, 0, -1, -1, -1, flow, last);
    else audit_write(cs, out.status, out.fault, out.flowtime, out.makespan, 2, 7 + (key2 & 1), t2, key2 >> 13, key2 >> 1 & 4095, 0, 0);
  }
}

// what the two entries refuse alike, in the ladder's order (sim_entry.h); an entry brings its map side, horizon and bytes
inline int audit_entry_check(std::initializer_list<const void*> pointers, int H, int W, int C, int N, int T, int side, int max_t,
                             const void* workspace, size_t workspace_bytes, size_t need) {
  return sim_entry_check(pointers, H > 0 && W > 0 && C > 0 && N > 0 && T > 0, H <= side && W <= side && T <= max_t && N <= AUDIT_MAX_N,
                         workspace, workspace_bytes, need);
}
