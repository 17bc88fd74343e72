// The workgroup of a row-board kernel, once per width: wave_group - one wavefront, lane = map row, one 64-bit word per row - and
// wide_group<NW> - up to four wavefronts, thread = map row, NW words per row, the LDS mail between the waves (row_board.h).  Both
// carry tid, nt and this thread's row of the free cells, and offer the same members, so a walk written against one runs on the other
// (sim_mapf_tree.h, sim_mapf_lns_walk.h, sim_mapf_audit_parts.h):
//   group_min / _max / _sum / _or   a reduction over the workgroup BEHIND A BARRIER of the whole workgroup, the same value in every
//   group_min3                      thread; min3: the lexicographically smallest int triple.  One wave: the butterfly.  Wide: the
//                                   butterfly, then one round of the mail - every thread passes the same sequence of wide_sync, so
//                                   they are called under conditions that are uniform over the workgroup only
//   group_sum_max(sum, max)         a sum and a maximum in ONE round: the closing figures of a case
//   group_sum_waves(v)              the sum over the waves of a value that is the same in every lane of a wave (a ballot's popcount)
//   group_count(pred, &before)      how many threads have pred, and how many of those sit in front of this one in thread order: the
//                                   ballot, its popcount and the bits below - wide: plus the waves in front, out of the same round
//   load_free(mp, H, W)             the free cells of the map into `free`;  publish_free(rows in LDS) / is_free(r, c): every row for
//                                   the threads that are not the cell's row (the caller's barrier stands between the two)
// Every store is a per-lane (vector) store from plain C++.
#pragma once
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"

__device__ __forceinline__ int lanes_below(u64 m, int lane) { return __popcll(lane ? m & (~0ull >> (64 - lane)) : 0ull); }

// free cells: row r of the map read by the lanes over its columns, one ballot per row; lanes >= H and bits >= W stay zero
__device__ __forceinline__ u64 load_free(const uint8_t* mp, int H, int W, int lane) {
  u64 free = 0ull;
  for (int r = 0; r < H; ++r) {
    const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] == 0);
    if (lane == r) free = word;
  }
  return free;
}
// wide: the rows of this wave, each read by the lanes over its columns, one ballot per word; rows >= H and bits >= W stay zero
template <int NW>
__device__ __forceinline__ wboard<NW> load_free(const uint8_t* mp, int H, int W, const wide_seat& s, int tid) {
  wboard<NW> free = wb_zero<NW>();
  for (int r = 64 * s.wave; r < H && r < 64 * s.wave + 64; ++r) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int col = 64 * k + s.lane;
      const u64 word = __builtin_amdgcn_ballot_w64(col < W && mp[r * W + (col < W ? col : 0)] == 0);
      if (tid == r) free.w[k] = word;
    }
  }
  return free;
}

struct wave_group {
  static constexpr int nt = 64;
  int tid;
  u64 free = 0ull;
  const u64* free_rows = nullptr;      // LDS, [row]
  __device__ __forceinline__ int group_min(int v) {
    v = wave_all_min(v);
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ int group_max(int v) {
    v = wave_all_max(v);
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ int group_sum(int v) {
    v = wave_all_sum(v);
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ int group_or(int v) {
    v = wave_all_or(v);
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ void group_sum_max(int& sum, int& max) {
    sum = wave_all_sum(sum), max = wave_all_max(max);
    __syncthreads();
  }
  __device__ __forceinline__ int group_sum_waves(int v) {      // v: the same in every lane of a wave
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ void group_min3(int& a, int& b, int& c) {
    wave_all_min3(a, b, c);
    __syncthreads();
  }
  __device__ __forceinline__ int group_count(bool pred, int* before) {
    const u64 m = __builtin_amdgcn_ballot_w64(pred);
    *before = m ? lanes_below(m, tid) : 0;      // (a scan's rounds mostly count nobody)
    __syncthreads();
    return __popcll(m);
  }
  __device__ __forceinline__ void load_free(const uint8_t* mp, int H, int W) { free = ::load_free(mp, H, W, tid); }
  __device__ __forceinline__ void publish_free(u64* rows) {
    rows[tid] = free;
    free_rows = rows;
  }
  __device__ __forceinline__ bool is_free(int r, int c) const { return has_bit(free_rows[r], c); }
};

template <int NW>
struct wide_group {
  int tid, nt;      // nt = rows
  wide_seat s;
  wboard<NW> free;
  const u64* free_rows;      // LDS, [row][NW]
  __device__ __forceinline__ int group_min(int v) {
    wide_post(s, 0, wave_all_min(v));
    return wide_min(s, wide_sync(s), 0);
  }
  __device__ __forceinline__ int group_max(int v) {
    wide_post(s, 0, wave_all_max(v));
    return wide_max(s, wide_sync(s), 0);
  }
  __device__ __forceinline__ int group_sum(int v) {
    wide_post(s, 0, wave_all_sum(v));
    return wide_sum(s, wide_sync(s), 0);
  }
  __device__ __forceinline__ int group_or(int v) {
    wide_post(s, 0, wave_all_or(v));
    return wide_or(s, wide_sync(s), 0);
  }
  __device__ __forceinline__ void group_sum_max(int& sum, int& max) {
    wide_post(s, 0, wave_all_sum(sum));
    wide_post(s, 1, wave_all_max(max));
    const int p = wide_sync(s);
    sum = wide_sum(s, p, 0), max = wide_max(s, p, 1);
  }
  __device__ __forceinline__ int group_sum_waves(int v) {      // v: the same in every lane of a wave
    wide_post(s, 0, v);
    return wide_sum(s, wide_sync(s), 0);
  }
  __device__ __forceinline__ void group_min3(int& a, int& b, int& c) {      // the butterfly, then the waves' three ints through the mail
    wave_all_min3(a, b, c);
    wide_post(s, 0, a);
    wide_post(s, 1, b);
    wide_post(s, 2, c);
    const int p = wide_sync(s);
    for (int w = 0; w < s.nwaves; ++w) {
      const int oa = s.mail->num[p][w][0], ob = s.mail->num[p][w][1], oc = s.mail->num[p][w][2];
      if (oa < a || (oa == a && (ob < b || (ob == b && oc < c)))) a = oa, b = ob, c = oc;
    }
  }
  __device__ __forceinline__ int group_count(bool pred, int* before) {
    const u64 m = __builtin_amdgcn_ballot_w64(pred);
    wide_post(s, 0, __popcll(m));
    const int p = wide_sync(s), total = wide_sum(s, p, 0);
    *before = total ? wide_sum_before(s, p, 0) + lanes_below(m, s.lane) : 0;      // (a scan's rounds mostly count nobody)
    return total;
  }
  __device__ __forceinline__ void load_free(const uint8_t* mp, int H, int W) { free = ::load_free<NW>(mp, H, W, s, tid); }
  __device__ __forceinline__ void publish_free(u64* rows) {
#pragma unroll
    for (int k = 0; k < NW; ++k) rows[tid * NW + k] = free.w[k];
    free_rows = rows;
  }
  __device__ __forceinline__ bool is_free(int r, int c) const { return has_bit(free_rows[r * NW + (c >> 6)], c & 63); }
};
template <int NW>
__device__ __forceinline__ wide_group<NW> wide_group_of(wide_mail* mail, int tid, int nt) {
  return wide_group<NW>{tid, nt, wide_seat{mail, tid & 63, tid >> 6, nt >> 6, 0}, wb_zero<NW>(), nullptr};
}
