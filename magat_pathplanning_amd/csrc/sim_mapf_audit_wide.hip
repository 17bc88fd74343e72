// The wide form of the schedule audit of sim_mapf_audit.hip: the same rule, cell for cell (include/magat_hip.h;
// restated in tests/audit_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_audit_wide_workspace_bytes   per case: the two cell-owner grids, 2 * H * W ints, and the cell of every agent
//                                               at the steps t - 1 and t, 2 * N ints
//   magat_sim_mapf_audit_wide                   one workgroup per case; one launch, no host round trip; nothing is modified
// The body, the stages and the keys are sim_mapf_audit_parts.h's (audit_walk), the ones the narrow form runs.  This file brings its
// form, in the layout of wmapf_plan_kernel (sim_mapf_wide.hip): `rows` threads, thread = map row, `words` 64-bit words per row in
// registers, votes and minima across the wavefronts through the LDS mail (row_board.h, sim_group.h).
//   dist        per agent a flood on the free board, one barrier per step as in the wide planner's layer loop: the boundary rows
//               and the votes (the goal is reached; the board still grows) travel in one round of the mail.
//   stage 2     the two cell-owner grids in the caller's workspace (set to "nobody" by the walk, then only the cells that were set
//               are cleared), global atomicMin.
// All control flow around a barrier is uniform over the workgroup.  Every store is a per-lane (vector) store or a global atomic
// from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_entry.h"      // wide_launch
#include "sim_group.h"      // wide_group
#include "sim_mapf_audit_parts.h"
#include "sim_mapf_wide_parts.h"      // WMAPF_MAX_T, wide_rows / wide_words

namespace {

__host__ __device__ inline long long waudit_case_ints(int H, int W, int N) { return 2LL * H * W + 2LL * N; }

// steps from (sr, sc) to a free cell (gr, gc), or -1 (the same for every thread); one round of the mail per step
template <int NW>
__device__ int waudit_flood(wide_seat& s, const wboard<NW>& free, int sr, int sc, int gr, int gc, int tid) {
  wboard<NW> reach = tid == sr ? wb_bit<NW>(sc) : wb_zero<NW>();
  bool grew = true;
  for (int steps = 0;; ++steps) {
    wide_post_rows(s, reach, reach);
    wide_post(s, 0, (int)wave_any(tid == gr && wb_has(reach, gc)) | (int)wave_any(grew) << 1);
    const int p = wide_sync(s);
    const int votes = wide_or(s, p, 0);
    if (votes & 1) return steps;
    if (!(votes & 2)) return -1;
    const wboard<NW> next = free & (reach | wide_cells_up(s, p, reach) | wide_cells_down(s, p, reach) | wb_left(reach) | wb_right(reach));
    grew = wb_any(next ^ reach);
    reach = next;
  }
}

template <int NW>
struct waudit_form : wide_group<NW> {
  int *own0, *own1;      // stage 2: the smallest agent on a cell at t - 1 and at t
  __device__ __forceinline__ int flood(int sr, int sc, int gr, int gc) { return waudit_flood<NW>(this->s, this->free, sr, sc, gr, gc, this->tid); }
};

template <int NW>
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_audit_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                                const uint8_t* __restrict__ solved, const int* __restrict__ paths,
                                                                const int* __restrict__ lengths, const int* __restrict__ start,
                                                                const int* __restrict__ goal, int* __restrict__ status,
                                                                int* __restrict__ fault, int* __restrict__ dist,
                                                                int* __restrict__ flow_bound, int* __restrict__ span_bound,
                                                                int* __restrict__ flowtime, int* __restrict__ makespan,
                                                                int* workspace, int N, int T) {
  __shared__ wide_mail mail;
  __shared__ u64 free_rows[WIDE_SIDE * NW];      // the free cells, for the threads that are not the cell's row
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = rows
  const long long a0 = (long long)cs * N;
  int* own = workspace + cs * waudit_case_ints(H, W, N);
  const audit_case k{map + cs * map_stride, H, W, solved, paths + a0 * T * 2, lengths + a0, start + a0 * 2, goal + a0 * 2,
                     own + 2LL * H * W, free_rows, N, T};
  waudit_form<NW> f{wide_group_of<NW>(&mail, tid, nt), own, own + H * W};
  audit_walk(f, k, audit_out{status, fault, dist, flow_bound, span_bound, flowtime, makespan}, cs);
}

}  // namespace

extern "C" size_t magat_sim_mapf_audit_wide_workspace_bytes(int C, int H, int W, int N, int T) {
  if (C <= 0 || H <= 0 || W <= 0 || N <= 0 || T <= 0 || H > WIDE_SIDE || W > WIDE_SIDE || N > AUDIT_MAX_N || T > WMAPF_MAX_T) return 0;
  return (size_t)C * (size_t)waudit_case_ints(H, W, N) * sizeof(int);
}

extern "C" int magat_sim_mapf_audit_wide(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved,
                                         const int32_t* paths, const int32_t* lengths, const int32_t* start, const int32_t* goal,
                                         int32_t* status, int32_t* fault, int32_t* dist, int32_t* flowtime_bound,
                                         int32_t* makespan_bound, int32_t* flowtime, int32_t* makespan, void* workspace,
                                         size_t workspace_bytes, int C, int N, int T, void* stream) {
  const int rc = audit_entry_check({map, paths, lengths, start, goal, status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan},
                                   H, W, C, N, T, WIDE_SIDE, WMAPF_MAX_T, workspace, workspace_bytes,
                                   magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T));
  if (rc != MAGAT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  int* ws = static_cast<int*>(workspace);
  magat_form_note(MAGAT_FORM_SIM_MAPF_AUDIT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_AUDIT, st);
  wide_launch(wide_words(W), [&](auto nw) {      // static LDS only: the free rows (2, 4 or 8 KB) and the mail
    hipLaunchKernelGGL(wmapf_audit_kernel<decltype(nw)::value>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, start,
                       goal, status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan, ws, N, T);
  });
  magat_prof_end(pid, st);
  return magat_check_launch();
}
