// What the tree walk (sim_mapf_tree.h) takes from below: the constraint bits of an agent's chain and a node's path laid into a row
// of the schedule, for any form - and cbs_wave, what the two one-wavefront forms (sim_mapf_cbs.hip, sim_mapf_ecbs.hip: lane = map row,
// one 64-bit word per row) bring alike: the one-wave group (sim_group.h: the reductions, the free board), the screening and a bit of
// the hard boards.
// Every store is a per-lane (vector) store from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"           // wave_any
#include "sim_group.h"           // wave_group
#include "sim_mapf_parts.h"      // MAPF_BOARDS, MAPF_SIDE

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
template <bool SET, typename Form, typename Node>
__device__ __forceinline__ void cbs_mark_chain(Form& f, const Node* nodes, int i, int x) {
  cbs_for_chain(nodes, i, x, [&](int board, int t, int r, int c) { f.template mark<SET>(board, t, r, c); });
}

// a path of `len` 16-bit cells, padded with its last one, into a row of the schedule; the nt threads of the workgroup over t
__device__ __forceinline__ void cbs_place(int* p, const uint16_t* src, int len, int T, int lane, int nt = 64) {
  for (int t = lane; t < T; t += nt) {
    const int cell = src[t < len ? t : len - 1];
    p[2 * t] = cell >> 8;
    p[2 * t + 1] = cell & 255;
  }
}

struct cbs_wave : wave_group {
  u64* hard;      // [t][V, A_up, A_left, A_down, A_right][row]: the constraints of the agent that is searched
  __device__ __forceinline__ bool screen(const int* st, const int* gl, int N, int H, int W) const {
    u64 starts = 0ull, goals = 0ull;
    bool ok = true;
    for (int a = 0; a < N && ok; ++a) {
      const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
      const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
      const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
      const u64 sbit = inside ? 1ull << sc : 0ull, gbit = inside ? 1ull << gc : 0ull;
      ok = wave_any(tid == sr && (free & ~starts & sbit)) && wave_any(tid == gr && (free & ~goals & gbit));
      if (tid == sr) starts |= sbit;
      if (tid == gr) goals |= gbit;
    }
    return ok;
  }
  template <bool SET>
  __device__ __forceinline__ void mark(int board, int t, int r, int c) const {
    cbs_mark<SET>(hard, board, t, r, c, tid);
  }
};
