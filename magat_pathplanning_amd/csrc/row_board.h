// Row boards: a map of up to 64 x 64 cells held by one wavefront, lane = map row, one 64-bit word per row (bit c = column c).
// A whole board - obstacles, a reachable set, a flood front - is one register pair across the wave: moving it left / right is
// a 64-bit shift, up / down a DPP wave shift.  Shared by sim_mapf.hip (the solver) and sim_cases.hip (the case generator).
// Wide boards (below): maps up to 256 x 256 held by one workgroup of up to four wavefronts, thread = map row, NW words per
// row - sim_mapf_wide.hip and sim_cases_wide.hip.
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
// the butterfly over the 64 lanes: op(a, b) of an int from every lane, the same value in every lane afterwards
template <typename Op>
__device__ __forceinline__ int wave_all(int v, Op op) {
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_all_min(int v) { return wave_all(v, [](int a, int b) { return b < a ? b : a; }); }
__device__ __forceinline__ int wave_all_max(int v) { return wave_all(v, [](int a, int b) { return b > a ? b : a; }); }
__device__ __forceinline__ int wave_all_sum(int v) { return wave_all(v, [](int a, int b) { return a + b; }); }
__device__ __forceinline__ int wave_all_or(int v) { return wave_all(v, [](int a, int b) { return a | b; }); }
// the lexicographically smallest (a, b, c) of the lanes
__device__ __forceinline__ void wave_all_min3(int& a, int& b, int& c) {
  for (int off = 32; off >= 1; off >>= 1) {
    const int oa = __shfl_xor(a, off, 64), ob = __shfl_xor(b, off, 64), oc = __shfl_xor(c, off, 64);
    if (oa < a || (oa == a && (ob < b || (ob == b && oc < c)))) a = oa, b = ob, c = oc;
  }
}

// ---- wide boards -------------------------------------------------------------------------------------------------------------
// One workgroup of 64 * ceil(H / 64) threads, thread = map row, NW = 1, 2 or 4 words per row in registers (word k holds columns
// 64 k .. 64 k + 63).  Threads at rows >= H hold zero and bits >= W are never set, so no shift wraps.  The words are only ever
// indexed by constants (unrolled loops, selects for a run-time column), so a board stays in registers.
constexpr int WIDE_SIDE = 256;
constexpr int WIDE_WAVES = WIDE_SIDE / 64;
constexpr int WIDE_MAX_WORDS = WIDE_SIDE / 64;

template <int NW>
struct wboard {
  u64 w[NW];
};
template <int NW>
__device__ __forceinline__ wboard<NW> wb_zero() {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = 0ull;
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> operator&(const wboard<NW>& a, const wboard<NW>& b) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = a.w[k] & b.w[k];
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> operator|(const wboard<NW>& a, const wboard<NW>& b) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = a.w[k] | b.w[k];
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> operator^(const wboard<NW>& a, const wboard<NW>& b) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = a.w[k] ^ b.w[k];
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> operator~(const wboard<NW>& a) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = ~a.w[k];
  return r;
}
template <int NW>
__device__ __forceinline__ bool wb_any(const wboard<NW>& a) {
  u64 v = 0ull;
#pragma unroll
  for (int k = 0; k < NW; ++k) v |= a.w[k];
  return v != 0ull;
}
template <int NW>
__device__ __forceinline__ int wb_count(const wboard<NW>& a) {
  int n = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) n += __popcll(a.w[k]);
  return n;
}
// the board of this row with column c alone (0 <= c < 64 NW)
template <int NW>
__device__ __forceinline__ wboard<NW> wb_bit(int c) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = (c >> 6) == k ? 1ull << (c & 63) : 0ull;
  return r;
}
template <int NW>
__device__ __forceinline__ bool wb_has(const wboard<NW>& a, int c) {      // 0 <= c < 64 NW
  u64 word = 0ull;
#pragma unroll
  for (int k = 0; k < NW; ++k) word = (c >> 6) == k ? a.w[k] : word;
  return has_bit(word, c & 63);
}
// columns 0 .. W - 1 of a row
template <int NW>
__device__ __forceinline__ wboard<NW> wb_columns(int W) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = W >= 64 * k + 64 ? ~0ull : W > 64 * k ? (1ull << (W - 64 * k)) - 1ull : 0ull;
  return r;
}
// left: column c takes column c + 1; right: column c takes column c - 1 - multi-word shifts, the carry bit goes between words
template <int NW>
__device__ __forceinline__ wboard<NW> wb_left(const wboard<NW>& a) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = (a.w[k] >> 1) | (k + 1 < NW ? a.w[k + 1 < NW ? k + 1 : k] << 63 : 0ull);
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> wb_right(const wboard<NW>& a) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = (a.w[k] << 1) | (k >= 1 ? a.w[k >= 1 ? k - 1 : k] >> 63 : 0ull);
  return r;
}
// a + b as one 64 NW-bit number (the carry out of the last word is dropped), and the row with its columns reversed
template <int NW>
__device__ __forceinline__ wboard<NW> wb_add(const wboard<NW>& a, const wboard<NW>& b) {
  wboard<NW> r;
  u64 carry = 0ull;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const u64 t = a.w[k] + b.w[k], s = t + carry;
    carry = (u64)(t < a.w[k]) | (u64)(s < t);
    r.w[k] = s;
  }
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> wb_reverse(const wboard<NW>& a) {
  wboard<NW> r;
#pragma unroll
  for (int k = 0; k < NW; ++k) r.w[k] = __brevll(a.w[NW - 1 - k]);
  return r;
}

// What crosses the wavefronts of the workgroup, in LDS: the boundary rows of a vertical shift (lane 0 of a wave is what lane 63
// of the wave above takes on the way up, lane 63 what lane 0 of the wave below takes on the way down) and up to three ints per
// wave (votes, counts).  Two copies used in turn: a wave posts into copy `parity`, ONE __syncthreads, everybody reads that copy
// and the next round posts into the other one - a copy is written again only behind the barrier of the round between, which
// every reader of it has passed.  Every round of a kernel goes through wide_sync, so all threads agree on the parity.
struct wide_mail {
  u64 up[2][WIDE_WAVES][WIDE_MAX_WORDS];
  u64 down[2][WIDE_WAVES][WIDE_MAX_WORDS];
  int num[2][WIDE_WAVES][3];
};
struct wide_seat {
  wide_mail* mail;
  int lane, wave, nwaves, parity;
};
__device__ __forceinline__ void wide_post(const wide_seat& s, int i, int v) {      // v: wave-uniform
  if (s.lane == 0) s.mail->num[s.parity][s.wave][i] = v;
}
template <int NW>
__device__ __forceinline__ void wide_post_rows(const wide_seat& s, const wboard<NW>& going_up, const wboard<NW>& going_down) {
  if (s.lane == 0) {
#pragma unroll
    for (int k = 0; k < NW; ++k) s.mail->up[s.parity][s.wave][k] = going_up.w[k];
  }
  if (s.lane == 63) {
#pragma unroll
    for (int k = 0; k < NW; ++k) s.mail->down[s.parity][s.wave][k] = going_down.w[k];
  }
}
// the barrier of a round; returns the copy to read
__device__ __forceinline__ int wide_sync(wide_seat& s) {
  __syncthreads();
  const int p = s.parity;
  s.parity ^= 1;
  return p;
}
__device__ __forceinline__ int wide_or(const wide_seat& s, int p, int i) {
  int v = 0;
  for (int w = 0; w < s.nwaves; ++w) v |= s.mail->num[p][w][i];
  return v;
}
__device__ __forceinline__ int wide_sum(const wide_seat& s, int p, int i) {
  int v = 0;
  for (int w = 0; w < s.nwaves; ++w) v += s.mail->num[p][w][i];
  return v;
}
__device__ __forceinline__ int wide_sum_before(const wide_seat& s, int p, int i) {      // over the waves in front of this one
  int v = 0;
  for (int w = 0; w < s.nwaves; ++w) v += w < s.wave ? s.mail->num[p][w][i] : 0;
  return v;
}
__device__ __forceinline__ int wide_max(const wide_seat& s, int p, int i) {
  int v = s.mail->num[p][0][i];
  for (int w = 1; w < s.nwaves; ++w) v = s.mail->num[p][w][i] > v ? s.mail->num[p][w][i] : v;
  return v;
}
__device__ __forceinline__ int wide_min(const wide_seat& s, int p, int i) {
  int v = s.mail->num[p][0][i];
  for (int w = 1; w < s.nwaves; ++w) v = s.mail->num[p][w][i] < v ? s.mail->num[p][w][i] : v;
  return v;
}
// the vertical shifts of the rows posted in copy p (call with every lane active: DPP)
template <int NW>
__device__ __forceinline__ wboard<NW> wide_cells_up(const wide_seat& s, int p, const wboard<NW>& v) {      // row r takes row r + 1
  wboard<NW> r;
  const bool edge = s.lane == 63 && s.wave + 1 < s.nwaves;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    r.w[k] = cells_up(v.w[k]);
    if (edge) r.w[k] = s.mail->up[p][s.wave + 1][k];
  }
  return r;
}
template <int NW>
__device__ __forceinline__ wboard<NW> wide_cells_down(const wide_seat& s, int p, const wboard<NW>& v) {      // row r takes row r - 1
  wboard<NW> r;
  const bool edge = s.lane == 0 && s.wave >= 1;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    r.w[k] = cells_down(v.w[k]);
    if (edge) r.w[k] = s.mail->down[p][s.wave - 1][k];
  }
  return r;
}
