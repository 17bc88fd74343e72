// What the solver (sim_mapf.hip) and the schedule improver (sim_mapf_lns.hip) share: the layout of the reservation boards, the
// space-time search of one agent and its backtrace.  One wavefront per case, lane = map row, one 64-bit word per row
// (row_board.h).  BOARDS = false compiles the loads of the reservation boards out - the same search on empty boards: an agent's
// FREE path - and `boards` is not read.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"      // u64, wave_shift, cells_up / cells_down, wave_any, has_bit

constexpr int MAPF_SIDE = 64;       // rows = lanes, columns = bits
constexpr int MAPF_MAX_T = 256;
constexpr int MAPF_BOARDS = 5;      // V, then A_d in the key order up, left, down, right
constexpr int MAPF_AHEAD = 4;       // layers of reservation boards in flight

__device__ __forceinline__ const u64* board_row(const u64* boards, int t, int b, int row) {
  return boards + ((long long)t * MAPF_BOARDS + b) * MAPF_SIDE + row;
}
template <bool BOARDS>
__device__ __forceinline__ u64 board_word(const u64* boards, int t, int b, int row) {
  if constexpr (BOARDS) return *board_row(boards, t, b, row);
  return 0ull;
}

// R_0 = {start}; R_{t+1} = free & ~V[t+1] & (R_t | U_d shift_d(R_t & ~A_opp(d)[t+1])).  Returns t* = the first t > last with the
// goal in R_t (last: the largest t with the goal in V[t]), or -1: R_t ran empty or t reached T - 1.  Wave-uniform.
template <bool BOARDS>
__device__ int mapf_search(const u64* boards, u64* R, u64 free, int sr, int sc, int gr, int gc, int T, int lane) {
  int last = -1;
  for (int base = (T - 1) & ~63; BOARDS && base >= 0; base -= 64) {      // lanes over t, highest 64 first
    const int t = base + lane;
    const u64 m = __builtin_amdgcn_ballot_w64(t < T && has_bit(*board_row(boards, t < T ? t : 0, 0, gr), gc));
    if (m) {
      last = base + 63 - __clzll(m);
      break;
    }
  }
  if (last >= T - 1) return -1;      // the goal is held for ever
  u64 cur = lane == sr ? 1ull << sc : 0ull;
  R[lane] = cur;
  u64 ahead[MAPF_AHEAD][MAPF_BOARDS];
#pragma unroll
  for (int k = 0; k < MAPF_AHEAD; ++k)
#pragma unroll
    for (int b = 0; b < MAPF_BOARDS; ++b) ahead[k][b] = 1 + k < T ? board_word<BOARDS>(boards, 1 + k, b, lane) : 0ull;
  for (int t0 = 0;; t0 += MAPF_AHEAD) {
#pragma unroll
    for (int k = 0; k < MAPF_AHEAD; ++k) {
      const int t = t0 + k;      // cur = R_t, ahead[k] = the boards of layer t + 1
      if (t > last && wave_any(lane == gr && has_bit(cur, gc))) return t;
      if (t == T - 1 || !wave_any(cur != 0ull)) return -1;
      const u64 v = ahead[k][0], a_up = ahead[k][1], a_left = ahead[k][2], a_down = ahead[k][3], a_right = ahead[k][4];
      const int tn = t + 1 + MAPF_AHEAD;
#pragma unroll
      for (int b = 0; b < MAPF_BOARDS; ++b) ahead[k][b] = tn < T ? board_word<BOARDS>(boards, tn, b, lane) : 0ull;
      // the swap rule: u -> u + d is closed when a planned agent enters u in the direction opposite to d in the same step
      const u64 moved = cells_up(cur & ~a_down) | ((cur & ~a_right) >> 1) | cells_down(cur & ~a_up) | ((cur & ~a_left) << 1);
      cur = (cur | moved) & free & ~v;
      R[(t + 1) * MAPF_SIDE + lane] = cur;
    }
  }
}

// Walks from (goal, t*) down to t = 1: the move INTO (r, c) is the first of up, left, down, right, stop whose source cell is in
// R_{t-1} and, for a real move, not in A_opp(d)[t].  Each candidate is tested by the lane of its row (a row off the map has
// no lane or an empty word).  Lane 0 writes the cells.
template <bool BOARDS>
__device__ void mapf_backtrace(const u64* boards, const u64* R, int* cells, int gr, int gc, int tstar, int W, int lane) {
  int r = gr, c = gc;
  if (lane == 0) cells[tstar] = r << 8 | c;
  u64 ahead[MAPF_AHEAD][4];
#pragma unroll
  for (int k = 0; k < MAPF_AHEAD; ++k)
#pragma unroll
    for (int b = 0; b < 4; ++b) ahead[k][b] = tstar - k >= 1 ? board_word<BOARDS>(boards, tstar - k, 1 + b, lane) : 0ull;
  for (int t0 = tstar; t0 >= 1; t0 -= MAPF_AHEAD) {
#pragma unroll
    for (int k = 0; k < MAPF_AHEAD; ++k) {
      const int t = t0 - k;
      if (t < 1) break;
      const u64 a_up = ahead[k][0], a_left = ahead[k][1], a_down = ahead[k][2], a_right = ahead[k][3];
      const int tn = t - MAPF_AHEAD;
#pragma unroll
      for (int b = 0; b < 4; ++b) ahead[k][b] = tn >= 1 ? board_word<BOARDS>(boards, tn, 1 + b, lane) : 0ull;
      const u64 prev = R[(t - 1) * MAPF_SIDE + lane];
      const bool up = lane == r + 1 && has_bit(prev & ~a_down, c);                    // moved up: came from the row below
      const bool left = lane == r && c + 1 < W && has_bit(prev & ~a_right, c + 1 < W ? c + 1 : c);
      const bool down = lane == r - 1 && has_bit(prev & ~a_up, c);
      const bool right = lane == r && c >= 1 && has_bit(prev & ~a_left, c >= 1 ? c - 1 : c);
      if (wave_any(up)) r += 1;
      else if (wave_any(left)) c += 1;
      else if (wave_any(down)) r -= 1;
      else if (wave_any(right)) c -= 1;      // else stop: (r, c) is in R_{t-1}
      if (lane == 0) cells[t - 1] = r << 8 | c;
    }
  }
}
