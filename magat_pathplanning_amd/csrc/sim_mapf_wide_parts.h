// What the wide solver (sim_mapf_wide.hip) and the wide schedule improver (sim_mapf_lns_wide.hip) share: the layout of the layers
// in the workspace, the space-time search of one agent and its backtrace.  One workgroup per case, thread = map row, NW 64-bit
// words per row (row_board.h: wide boards).  BOARDS = false compiles the loads of the reservation boards out - the same search
// on empty boards: an agent's FREE path; the R layers are still written to the workspace, since the backtrace reads them.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"

constexpr int WMAPF_MAX_T = 1024;
constexpr int WMAPF_BOARDS = 6;      // V, then A_d in the key order up, left, down, right, then R
constexpr int WMAPF_R = 5;
constexpr int WMAPF_AHEAD = 4;       // layers of boards in flight

__host__ __device__ constexpr int wide_rows(int H) { return 64 * ((H + 63) / 64); }
__host__ __device__ constexpr int wide_words(int W) { return W <= 64 ? 1 : W <= 128 ? 2 : 4; }

// the layers of one case, NB boards each (the wide ECBS keeps sets of 5, and its planes as layers of one board): every thread
// touches its own row of a board, but for the reservations of a path
template <int NW, int NB = WMAPF_BOARDS>
struct wide_layers {
  u64* base;
  int rows;
  __device__ __forceinline__ u64* at(int t, int b, int row) const { return base + (((long long)t * NB + b) * rows + row) * NW; }
  __device__ __forceinline__ wboard<NW> load(int t, int b, int row) const {
    wboard<NW> r;
    const u64* p = at(t, b, row);
#pragma unroll
    for (int k = 0; k < NW; ++k) r.w[k] = p[k];
    return r;
  }
  // a reservation board (b < WMAPF_R): empty when the boards are compiled out
  template <bool BOARDS>
  __device__ __forceinline__ wboard<NW> board(int t, int b, int row) const {
    if constexpr (BOARDS) return load(t, b, row);
    return wb_zero<NW>();
  }
  __device__ __forceinline__ void store(int t, int b, int row, const wboard<NW>& v) const {
    u64* p = at(t, b, row);
#pragma unroll
    for (int k = 0; k < NW; ++k) p[k] = v.w[k];
  }
};

// R_0 = {start}; R_{t+1} = free & ~V[t+1] & (R_t | U_d shift_d(R_t & ~A_opp(d)[t+1])).  Returns t* = the first t > last with the
// goal in R_t (last: the largest t with the goal in V[t]), or -1: R_t ran empty or t reached T - 1.  The same for every thread.
template <int NW, bool BOARDS>
__device__ int wmapf_search(const wide_layers<NW>& L, wide_seat& s, const wboard<NW>& free, int sr, int sc, int gr, int gc, int T,
                            int tid, int nt) {
  int last = -1;
  if constexpr (BOARDS) {
    int hit = -1;      // threads over t, ascending: the last hit of the wave is its largest
    for (int base = 0; base < T; base += nt) {
      const int t = base + tid;
      const u64 m = __builtin_amdgcn_ballot_w64(t < T && has_bit(L.at(t < T ? t : 0, 0, gr)[gc >> 6], gc & 63));
      if (m) hit = base + 64 * s.wave + 63 - __clzll(m);
    }
    wide_post(s, 0, hit);
    last = wide_max(s, wide_sync(s), 0);
  }
  if (last >= T - 1) return -1;      // the goal is held for ever
  wboard<NW> cur = tid == sr ? wb_bit<NW>(sc) : wb_zero<NW>();
  L.store(0, WMAPF_R, tid, cur);
  wboard<NW> ahead[WMAPF_AHEAD][5];
#pragma unroll
  for (int k = 0; k < WMAPF_AHEAD; ++k)
#pragma unroll
    for (int b = 0; b < 5; ++b) ahead[k][b] = 1 + k < T ? L.template board<BOARDS>(1 + k, b, tid) : wb_zero<NW>();
  for (int t0 = 0;; t0 += WMAPF_AHEAD) {
#pragma unroll
    for (int k = 0; k < WMAPF_AHEAD; ++k) {
      const int t = t0 + k;      // cur = R_t, ahead[k] = the boards of layer t + 1
      const wboard<NW> v = ahead[k][0], a_up = ahead[k][1], a_left = ahead[k][2], a_down = ahead[k][3], a_right = ahead[k][4];
      const int tn = t + 1 + WMAPF_AHEAD;
#pragma unroll
      for (int b = 0; b < 5; ++b) ahead[k][b] = tn < T ? L.template board<BOARDS>(tn, b, tid) : wb_zero<NW>();
      // the swap rule: u -> u + d is closed when a planned agent enters u in the direction opposite to d in the same step
      const wboard<NW> going_up = cur & ~a_down, going_down = cur & ~a_up;
      wide_post_rows(s, going_up, going_down);
      wide_post(s, 0, (int)wave_any(tid == gr && wb_has(cur, gc)) | (int)wave_any(wb_any(cur)) << 1);
      const int p = wide_sync(s);
      const int votes = wide_or(s, p, 0);
      if (t > last && (votes & 1)) return t;
      if (t == T - 1 || !(votes & 2)) return -1;
      const wboard<NW> moved = wide_cells_up(s, p, going_up) | wb_left(cur & ~a_right) | wide_cells_down(s, p, going_down) |
                               wb_right(cur & ~a_left);
      cur = (cur | moved) & free & ~v;
      L.store(t + 1, WMAPF_R, tid, cur);
    }
  }
}

// Walks from (goal, t*) down to t = 1: the move INTO (r, c) is the first of up, left, down, right, stop whose source cell is in
// R_{t-1} and, for a real move, not in A_opp(d)[t].  Each candidate is tested by the thread of its row (a row off the map has
// no thread or an empty row), the workgroup votes.  Thread 0 writes the cells.
template <int NW, bool BOARDS>
__device__ void wmapf_backtrace(const wide_layers<NW>& L, wide_seat& s, int* cells, int gr, int gc, int tstar, int W, int tid) {
  int r = gr, c = gc;
  if (tid == 0) cells[tstar] = r << 8 | c;
  wboard<NW> ahead[WMAPF_AHEAD][5];      // A_up, A_left, A_down, A_right of layer t, and R_{t-1}
#pragma unroll
  for (int k = 0; k < WMAPF_AHEAD; ++k)
#pragma unroll
    for (int b = 0; b < 5; ++b)
      ahead[k][b] = tstar - k >= 1 ? (b < 4 ? L.template board<BOARDS>(tstar - k, 1 + b, tid) : L.load(tstar - k - 1, WMAPF_R, tid))
                                   : wb_zero<NW>();
  for (int t0 = tstar; t0 >= 1; t0 -= WMAPF_AHEAD) {
#pragma unroll
    for (int k = 0; k < WMAPF_AHEAD; ++k) {
      const int t = t0 - k;
      if (t < 1) break;
      const wboard<NW> a_up = ahead[k][0], a_left = ahead[k][1], a_down = ahead[k][2], a_right = ahead[k][3], prev = ahead[k][4];
      const int tn = t - WMAPF_AHEAD;
#pragma unroll
      for (int b = 0; b < 5; ++b)
        ahead[k][b] = tn >= 1 ? (b < 4 ? L.template board<BOARDS>(tn, 1 + b, tid) : L.load(tn - 1, WMAPF_R, tid)) : wb_zero<NW>();
      const bool up = tid == r + 1 && wb_has(prev & ~a_down, c);                      // moved up: came from the row below
      const bool left = tid == r && c + 1 < W && wb_has(prev & ~a_right, c + 1 < W ? c + 1 : c);
      const bool down = tid == r - 1 && wb_has(prev & ~a_up, c);
      const bool right = tid == r && c >= 1 && wb_has(prev & ~a_left, c >= 1 ? c - 1 : c);
      wide_post(s, 0, (int)wave_any(up) | (int)wave_any(left) << 1 | (int)wave_any(down) << 2 | (int)wave_any(right) << 3);
      const int votes = wide_or(s, wide_sync(s), 0);
      if (votes & 1) r += 1;
      else if (votes & 2) c += 1;
      else if (votes & 4) r -= 1;
      else if (votes & 8) c -= 1;      // else stop: (r, c) is in R_{t-1}
      if (tid == 0) cells[t - 1] = r << 8 | c;
    }
  }
}
