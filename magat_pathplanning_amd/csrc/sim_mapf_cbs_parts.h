// What conflict-based search (sim_mapf_cbs.hip) and its bounded-suboptimal form (sim_mapf_ecbs.hip) share: the reductions over the
// wavefront, the constraint bits of an agent's chain on the hard boards, and a node's path laid into a row of the schedule.
// One wavefront per case, lane = map row.  Every store is a per-lane (vector) store from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_parts.h"      // MAPF_BOARDS, MAPF_SIDE

__device__ __forceinline__ int cbs_wave_min(int v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ int cbs_wave_max(int v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// one constraint bit, by the lane of its row
template <bool SET>
__device__ __forceinline__ void cbs_mark(u64* boards, int board, int t, int r, int c, int lane) {
  if (lane == r) {
    u64* w = boards + ((long long)t * MAPF_BOARDS + board) * MAPF_SIDE + r;
    if (SET) *w |= 1ull << c;
    else *w &= ~(1ull << c);
  }
}
// the constraints of agent x on the chain from node i to the root: mark(board, t, row, col) for each
// (Node: parent, who = agent | board << 12 | ..., what = t | row << 16 | col << 24)
template <typename Node, typename Mark>
__device__ __forceinline__ void cbs_for_chain(const Node* nodes, int i, int x, Mark mark) {
  while (i > 0) {
    const int who = __builtin_amdgcn_readfirstlane(nodes[i].who), what = __builtin_amdgcn_readfirstlane(nodes[i].what);
    if ((who & 4095) == x) mark(who >> 12 & 7, what & 0xffff, what >> 16 & 255, what >> 24 & 255);
    i = __builtin_amdgcn_readfirstlane(nodes[i].parent);
  }
}
template <bool SET, typename Node>
__device__ void cbs_mark_chain(u64* boards, const Node* nodes, int i, int x, int lane) {
  cbs_for_chain(nodes, i, x, [&](int board, int t, int r, int c) { cbs_mark<SET>(boards, board, t, r, c, lane); });
}

// a path of `len` 16-bit cells, padded with its last one, into a row of the schedule; the nt threads of the workgroup over t
__device__ __forceinline__ void cbs_place(int* p, const uint16_t* src, int len, int T, int lane, int nt = 64) {
  for (int t = lane; t < T; t += nt) {
    const int cell = src[t < len ? t : len - 1];
    p[2 * t] = cell >> 8;
    p[2 * t + 1] = cell & 255;
  }
}
