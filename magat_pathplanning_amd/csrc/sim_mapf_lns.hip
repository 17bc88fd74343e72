// Improves the schedules of the path-finding expert by neighbourhood re-planning (MAPF-LNS on top of prioritized planning;
// DESIGN 4.11, restated cell by cell in tests/lns_restatement.py): the form of maps up to 64 x 64.
//   magat_sim_mapf_improve_workspace_bytes   per case: the reservation boards, 5 * T * 64 * 8 bytes, and d0, one int per agent
//   magat_sim_mapf_improve                   one wavefront per case runs every iteration; one launch, no host round trip
// The rule is sim_mapf_lns_walk.h's walk, the one the wide form runs.  This file brings its form, in the layout of mapf_plan_kernel
// (sim_mapf.hip): lane = map row, one 64-bit word per row, reservation boards in the workspace, R layers in dynamic LDS; search
// and backtrace are the solver's own (sim_mapf_parts.h).  Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_group.h"              // wave_group
#include "sim_mapf_lns_walk.h"      // mapf_lns_walk, lns_entry_check
#include "sim_mapf_parts.h"         // MAPF_*, board_row, mapf_search, mapf_backtrace

namespace {

__host__ __device__ inline long long lns_case_words(int N, int T) {      // boards, then d0 padded to whole words
  return (long long)T * MAPF_BOARDS * MAPF_SIDE + ((long long)N + 1) / 2;
}

struct lns_form : wave_group {
  u64 *boards, *R;      // [t][V, A_up, A_left, A_down, A_right][row] in the workspace; [T][64] in LDS
  int (*old_cells)[MAPF_MAX_T];      // LDS: the old paths of the neighbourhood (from global rows the un-reserve and the roll-back cost time)
  int T, W;
  __device__ __forceinline__ void stage_old(const int* nb, int m, const int* rows, const int* len, int T) const {
    for (int j = 0; j < m; ++j) {
      const lns_row row{rows + (long long)nb[j] * T * 2};
      for (int t = tid; t < len[nb[j]]; t += 64) old_cells[j][t] = row(t);
    }
    __syncthreads();      // the staged cells are read by other lanes
  }
  __device__ __forceinline__ lns_staged old(int j, lns_row) const { return lns_staged{old_cells[j]}; }
  __device__ __forceinline__ void clear_boards() const {
    for (int i = tid; i < T * MAPF_BOARDS * MAPF_SIDE; i += 64) boards[i] = 0ull;
  }
  __device__ __forceinline__ u64* board_word(int t, int b, int r, int) const { return boards + ((long long)t * MAPF_BOARDS + b) * MAPF_SIDE + r; }
  template <bool BOARDS>
  __device__ __forceinline__ int search(int sr, int sc, int gr, int gc) const {
    return mapf_search<BOARDS>(BOARDS ? boards : nullptr, R, free, sr, sc, gr, gc, T, tid);
  }
  template <bool BOARDS>
  __device__ __forceinline__ void trace(int* cells, int gr, int gc, int tstar) const {
    __syncthreads();      // the R layers are read behind the search's stores
    mapf_backtrace<BOARDS>(BOARDS ? boards : nullptr, R, cells, gr, gc, tstar, W, tid);
  }
};

__global__ __launch_bounds__(64) void mapf_lns_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                      const uint8_t* __restrict__ solved, int* paths, int* lengths, int* makespan,
                                                      int* __restrict__ flow_before, int* __restrict__ flow_after,
                                                      int* __restrict__ accepted, int* __restrict__ status, u64* workspace, int N,
                                                      int T, int iterations, int K) {
  HIP_DYNAMIC_SHARED(u64, R)                      // [T][64]
  __shared__ u64 free_rows[MAPF_SIDE];            // the free cells, for the lanes that are not the cell's row
  __shared__ lns_stage<MAPF_MAX_T> stage;
  __shared__ int old_cells[LNS_MAX_K][MAPF_MAX_T];
  const int cs = blockIdx.x, lane = threadIdx.x;
  u64* boards = workspace + (long long)cs * lns_case_words(N, T);
  const long long a0 = (long long)cs * N;
  const lns_case k{map + cs * map_stride, H, W, solved[cs], paths + a0 * T * 2, lengths + a0,
                   reinterpret_cast<int*>(boards + (long long)T * MAPF_BOARDS * MAPF_SIDE), free_rows, N, T};
  lns_form f{{lane}, boards, R, old_cells, T, W};
  mapf_lns_walk(f, k, stage, lns_out{makespan, flow_before, flow_after, accepted, status}, cs, iterations, K);
}

}  // namespace

extern "C" size_t magat_sim_mapf_improve_workspace_bytes(int C, int N, int T) {
  if (C <= 0 || N <= 0 || T <= 0) return 0;
  return (size_t)C * (size_t)lns_case_words(N, T) * sizeof(u64);
}

extern "C" int magat_sim_mapf_improve(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved, int32_t* paths,
                                      int32_t* lengths, int32_t* makespan, int32_t* flowtime_before, int32_t* flowtime_after,
                                      int32_t* accepted, int32_t* status, void* workspace, size_t workspace_bytes, int C, int N,
                                      int T, int iterations, int k, void* stream) {
  const int rc = lns_entry_check({map, solved, paths, lengths, makespan, flowtime_before, flowtime_after, accepted, status}, H, W, C, N, T,
                                 iterations, k, MAPF_SIDE, MAPF_MAX_T, workspace, workspace_bytes,
                                 magat_sim_mapf_improve_workspace_bytes(C, N, T));
  if (rc != MAGAT_OK) return rc;
  // dynamic LDS: the R layers, <= 128 KB; + 18 KB static (the stage of 2 * 8 paths, the free path, the free rows)
  const size_t lds = (size_t)T * MAPF_SIDE * sizeof(u64);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (magat_ensure_dyn_lds(reinterpret_cast<const void*>(&mapf_lns_kernel), MAGAT_LDS_SIM_MAPF_LNS, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  magat_form_note(MAGAT_FORM_SIM_MAPF_LNS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_LNS, st);
  hipLaunchKernelGGL(mapf_lns_kernel, dim3((unsigned)C), dim3(64), lds, st, map, map_batched ? (long long)H * W : 0LL, H, W, solved,
                     paths, lengths, makespan, flowtime_before, flowtime_after, accepted, status, static_cast<u64*>(workspace), N, T,
                     iterations, k);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
