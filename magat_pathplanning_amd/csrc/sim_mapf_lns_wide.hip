// The wide form of the schedule improver of sim_mapf_lns.hip: the same neighbourhood re-planning rule, cell for cell (DESIGN
// 4.11; restated in tests/lns_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_improve_wide_workspace_bytes   per case: the layers, T * 6 * rows * words * 8 bytes, and d0, one int per agent
//   magat_sim_mapf_improve_wide                   one workgroup per case runs every iteration; one launch, no host round trip
// The rule is sim_mapf_lns_walk.h's walk, the one the narrow form runs.  This file brings its form, in the layout of
// wmapf_plan_kernel (sim_mapf_wide.hip): `rows` threads, thread = map row, `words` 64-bit words per row in registers, the five
// reservation boards and the R layer of every t in the workspace, votes and counts across the wavefronts through the LDS mail
// (row_board.h, sim_group.h); search and backtrace are the wide solver's own (sim_mapf_wide_parts.h).  LDS: the walk's stage (the
// free path and 8 re-planned paths of 1024 cells), the free rows and the mail.
// Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_entry.h"      // wide_launch
#include "sim_group.h"                // wide_group
#include "sim_mapf_lns_walk.h"        // mapf_lns_walk, lns_entry_check
#include "sim_mapf_wide_parts.h"      // WMAPF_*, wide_rows / wide_words, wide_layers, wmapf_search, wmapf_backtrace

namespace {

__host__ __device__ inline long long wlns_layer_words(int rows, int words) { return (long long)WMAPF_BOARDS * rows * words; }
__host__ __device__ inline long long wlns_case_words(int rows, int words, int N, int T) {      // layers, then d0 padded to whole words
  return (long long)T * wlns_layer_words(rows, words) + ((long long)N + 1) / 2;
}

template <int NW>
struct wlns_form : wide_group<NW> {
  wide_layers<NW> L;
  int T, W;
  __device__ __forceinline__ void clear_boards() const {      // the reservation boards; an R layer is written before it is read
    const int nt = this->nt;
    for (int t = 0; t < T; ++t)
      for (int i = this->tid; i < 5 * nt * NW; i += nt) L.base[t * wlns_layer_words(nt, NW) + i] = 0ull;
  }
  __device__ __forceinline__ u64* board_word(int t, int b, int r, int c) const { return L.at(t, b, r) + (c >> 6); }
  __device__ __forceinline__ void stage_old(const int*, int, const int*, const int*, int) const {}      // the old paths are read from their global rows
  __device__ __forceinline__ lns_row old(int, lns_row row) const { return row; }
  // (the seat goes in as a local of its own: the inliner weighs the call by what it can keep in registers - sim_mapf_ecbs_wide.hip)
  template <bool BOARDS>
  __device__ __forceinline__ int search(int sr, int sc, int gr, int gc) {
    wide_seat seat = this->s;
    const int tstar = wmapf_search<NW, BOARDS>(L, seat, this->free, sr, sc, gr, gc, T, this->tid, this->nt);
    this->s = seat;
    return tstar;
  }
  template <bool BOARDS>
  __device__ __forceinline__ void trace(int* cells, int gr, int gc, int tstar) {
    wide_seat seat = this->s;
    wmapf_backtrace<NW, BOARDS>(L, seat, cells, gr, gc, tstar, W, this->tid);
    this->s = seat;
  }
};

template <int NW>
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_lns_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                              const uint8_t* __restrict__ solved, int* paths, int* lengths,
                                                              int* makespan, int* __restrict__ flow_before,
                                                              int* __restrict__ flow_after, int* __restrict__ accepted,
                                                              int* __restrict__ status, u64* workspace, int N, int T, int iterations,
                                                              int K) {
  __shared__ wide_mail mail;
  __shared__ u64 free_rows[WIDE_SIDE * NW];      // the free cells, for the threads that are not the cell's row
  __shared__ lns_stage<WMAPF_MAX_T> stage;
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = rows
  u64* mine = workspace + (long long)cs * wlns_case_words(nt, NW, N, T);
  const long long a0 = (long long)cs * N;
  const lns_case k{map + cs * map_stride, H, W, solved[cs], paths + a0 * T * 2, lengths + a0,
                   reinterpret_cast<int*>(mine + (long long)T * wlns_layer_words(nt, NW)), free_rows, N, T};
  wlns_form<NW> f{wide_group_of<NW>(&mail, tid, nt), wide_layers<NW>{mine, nt}, T, W};
  mapf_lns_walk(f, k, stage, lns_out{makespan, flow_before, flow_after, accepted, status}, cs, iterations, K);
}

}  // namespace

extern "C" size_t magat_sim_mapf_improve_wide_workspace_bytes(int C, int H, int W, int N, int T) {
  if (C <= 0 || H <= 0 || W <= 0 || N <= 0 || T <= 0 || H > WIDE_SIDE || W > WIDE_SIDE) return 0;
  return (size_t)C * (size_t)wlns_case_words(wide_rows(H), wide_words(W), N, T) * sizeof(u64);
}

extern "C" int magat_sim_mapf_improve_wide(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved, int32_t* paths,
                                           int32_t* lengths, int32_t* makespan, int32_t* flowtime_before, int32_t* flowtime_after,
                                           int32_t* accepted, int32_t* status, void* workspace, size_t workspace_bytes, int C, int N,
                                           int T, int iterations, int k, void* stream) {
  const int rc = lns_entry_check({map, solved, paths, lengths, makespan, flowtime_before, flowtime_after, accepted, status}, H, W, C, N, T,
                                 iterations, k, WIDE_SIDE, WMAPF_MAX_T, workspace, workspace_bytes,
                                 magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T));
  if (rc != MAGAT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
  magat_form_note(MAGAT_FORM_SIM_MAPF_LNS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_LNS, st);
  wide_launch(wide_words(W), [&](auto nw) {      // static LDS only: 4 + 32 KB of paths, the free rows (2, 4 or 8 KB) and the mail
    hipLaunchKernelGGL(wmapf_lns_kernel<decltype(nw)::value>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, makespan,
                       flowtime_before, flowtime_after, accepted, status, ws, N, T, iterations, k);
  });
  magat_prof_end(pid, st);
  return magat_check_launch();
}
