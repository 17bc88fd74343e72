// What the two forms of the schedule audit (sim_mapf_audit.hip, sim_mapf_audit_wide.hip) share: the packed keys of a fault, the
// per-agent checks of stage 1 and the conflict search of stage 2.  The rule is in include/magat_hip.h and DESIGN 4.11, restated
// cell by cell in tests/audit_restatement.py.  The forms differ in how a map is held (one wave with a word per row, or a
// workgroup with up to four), so they bring: is_free(r, c) for a cell ON the map, and group_min(key) - the minimum over the
// workgroup, the same value for every thread, behind a barrier of the whole workgroup.
// Every store is a per-lane (vector) store or an atomic from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"

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
