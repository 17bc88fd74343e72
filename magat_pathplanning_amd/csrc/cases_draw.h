// The case generator's random stream and lane scans, shared by sim_cases.hip (maps up to 64 x 64) and sim_cases_wide.hip (up to
// 256 x 256): a case is a function of (seed, global case index, stream, index) in both, so the two forms draw the same numbers.
#pragma once
#include "row_board.h"

constexpr int CASES_ROUNDS = 64;                  // goal tuples drawn before a case is given up
constexpr int CASES_MAX_AISLES = 4096;            // bounds on the sequential maze walk: aisles * walk steps per case
constexpr int CASES_MAX_WALK = 1024;
constexpr u64 CASES_M = 0x9E3779B97F4A7C15ull;
enum { STREAM_AISLE_X = 0, STREAM_AISLE_Y = 1, STREAM_WALK = 2, STREAM_CELL = 3, STREAM_START = 4, STREAM_GOAL = 5 };

__device__ __forceinline__ u64 mix64(u64 z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// the upper 32 bits of draw(seed, case, stream, i); key = mix(seed + M * (case + 1))
__device__ __forceinline__ unsigned draw32(u64 key, int stream, u64 i) {
  return (unsigned)(mix64(key + CASES_M * ((((u64)stream << 40) | i) + 1)) >> 32);
}
__device__ __forceinline__ int below(unsigned u, int n) { return (int)(((u64)u * (unsigned)n) >> 32); }

template <int CTRL>
__device__ __forceinline__ int dpp_int(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ int wave_sum_int(int v) {      // wave-uniform
  v += dpp_int<0x128>(v);      // row_ror 8, 4, 2, 1: all-reduce of each 16-lane row
  v += dpp_int<0x124>(v);
  v += dpp_int<0x122>(v);
  v += dpp_int<0x121>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
__device__ __forceinline__ int wave_scan_int(int v, int lane) {      // inclusive prefix sum over the lanes
  v += dpp_int<0x111>(v);      // row_shr 1, 2, 4, 8 with zero fill: the scan of each 16-lane row
  v += dpp_int<0x112>(v);
  v += dpp_int<0x114>(v);
  v += dpp_int<0x118>(v);
  const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
  const int row = lane >> 4;
  return v + (row >= 1 ? t0 : 0) + (row >= 2 ? t1 : 0) + (row >= 3 ? t2 : 0);
}
