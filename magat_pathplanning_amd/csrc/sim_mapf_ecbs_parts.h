// What the two forms of ECBS (sim_mapf_ecbs.hip, sim_mapf_ecbs_wide.hip) share below the tree walk (sim_mapf_tree.h): the limits, the
// node of the tree and the conflict count hc of a schedule.  The rule is in include/magat_hip.h and DESIGN 4.11, restated cell by cell
// in tests/ecbs_restatement.py.  The forms differ in how a map is held (one wave with a word per row, or a workgroup with up to four)
// and so bring group_sum(n): the sum over the workgroup (row_board.h: wave_all_sum, then the mail), the same value for every thread.
// Every store is a per-lane (vector) store or an atomic from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_NONE

constexpr int ECBS_MAX_NODES = 4096;
constexpr int ECBS_MAX_LEVELS = 4;
constexpr int ECBS_MAX_W_MILLI = 1 << 20;

struct ecbs_node {
  int parent;
  int cost;      // the flowtime of the node's schedule; -1: the child found no arrival
  int lb;        // the sum of the agents' t*
  int hc;        // the conflicts of the node's schedule
  int who;       // agent | board << 12 | open << 15
  int what;      // the constraint: t | row << 16 | col << 24
  int tstar;     // the re-planned agent's bound
  int len1;      // the length of its new path - 1 (up to 1023 in the wide form: a word of its own in both)
};

// hc of the schedule in `rows`, over t < span: own_t[cell] is the smallest agent on a cell at t (audit_stage2's grids, all
// AUDIT_NONE going in and coming out).  Counted: the agents a with own_t[cell_a(t)] < a, and for t >= 1 the agents a that moved,
// with b = own_(t-1)[cell_a(t)] existing, b > a and cell_b(t) == cell_a(t-1).  Threads over agents; the same value for every
// thread.
template <typename GroupSum>
__device__ int ecbs_count(const int* rows, int N, int T, int W, int span, int* own0, int* own1, int* at0, int* at1, int tid, int nt,
                          GroupSum group_sum) {
  int *own_cur = own0, *own_prv = own1, *at_cur = at0, *at_prv = at1;
  int n = 0;
  for (int t = 0; t < span; ++t) {
    for (int a = tid; a < N; a += nt) {
      const int* p = rows + ((long long)a * T + t) * 2;
      const int cell = p[0] * W + p[1];
      at_cur[a] = cell;
      atomicMin(&own_cur[cell], a);
    }
    __syncthreads();
    for (int a = tid; a < N; a += nt) {
      const int cell = at_cur[a];
      if (own_cur[cell] < a) ++n;
      if (t >= 1) {
        const int from = at_prv[a], b = own_prv[cell];
        if (from != cell && b != AUDIT_NONE && b > a && at_cur[b] == from) ++n;
      }
    }
    __syncthreads();      // every read of own_prv lies behind
    if (t >= 1)
      for (int a = tid; a < N; a += nt) own_prv[at_prv[a]] = AUDIT_NONE;
    __syncthreads();
    int* g = own_cur;
    own_cur = own_prv, own_prv = g;
    g = at_cur;
    at_cur = at_prv, at_prv = g;
  }
  if (span >= 1)
    for (int a = tid; a < N; a += nt) own_prv[at_prv[a]] = AUDIT_NONE;
  __syncthreads();
  return group_sum(n);
}
