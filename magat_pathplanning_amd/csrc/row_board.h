// Row boards: a map of up to 64 x 64 cells held by one wavefront, lane = map row, one 64-bit word per row (bit c = column c).
// A whole board - obstacles, a reachable set, a flood front - is one register pair across the wave: moving it left / right is
// a 64-bit shift, up / down a DPP wave shift.  Shared by sim_mapf.hip (the solver) and sim_cases.hip (the case generator).
#pragma once
#include "magat_common.h"

typedef unsigned long long u64;

// DPP wave shifts of both halves of a board word; the lane without a source gets zero
template <int CTRL>
__device__ __forceinline__ u64 wave_shift(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, true);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 cells_up(u64 v) { return wave_shift<0x130>(v); }        // wave_shl:1 - row r takes row r + 1
__device__ __forceinline__ u64 cells_down(u64 v) { return wave_shift<0x138>(v); }      // wave_shr:1 - row r takes row r - 1
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
__device__ __forceinline__ bool has_bit(u64 w, int c) { return (w >> c) & 1ull; }
