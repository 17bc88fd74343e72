// Audits schedules of the path-finding expert on the device (the rule is in include/magat_hip.h, restated cell by
// cell in tests/audit_restatement.py): is a schedule a valid MAPF solution, where is its first fault, and how far is its
// flowtime from the classic lower bound, the sum of the agents' obstacle-avoiding shortest distances.
//   magat_sim_mapf_audit_workspace_bytes   per case: the cell of every agent at the steps t - 1 and t, 2 * N ints
//   magat_sim_mapf_audit                   one wavefront per case; one launch, no host round trip; nothing is modified
// The body, the stages and the keys are sim_mapf_audit_parts.h's (audit_walk), the ones the wide form runs.  This file brings its
// form, in the layout of mapf_plan_kernel (sim_mapf.hip): lane = map row, one 64-bit word per row (row_board.h).
//   dist        per agent a flood on the free board in registers, reach |= free & (reach and its four shifts), counted until
//               the goal's bit is set; the board standing still first: -1.  For every case, skipped and faulty ones too.
//   stage 2     two cell-owner grids in LDS (2 * 64 * 64 ints = 32 KB) for t - 1 and t.
// Integer arithmetic only; every store is a per-lane (vector) store or an LDS atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_group.h"      // wave_group
#include "sim_mapf_audit_parts.h"
#include "sim_mapf_parts.h"      // MAPF_SIDE, MAPF_MAX_T

namespace {

// steps from (sr, sc) to another free cell (gr, gc), or -1 (wave-uniform)
__device__ int audit_flood(u64 free, int sr, int sc, int gr, int gc, int lane) {
  u64 reach = lane == sr ? 1ull << sc : 0ull;
  for (int steps = 1;; ++steps) {
    const u64 next = free & (reach | cells_up(reach) | cells_down(reach) | reach << 1 | reach >> 1);
    if (wave_any(lane == gr && has_bit(next, gc))) return steps;
    if (!wave_any(next != reach)) return -1;
    reach = next;
  }
}

struct audit_form : wave_group {
  int *own0, *own1;      // stage 2: the smallest agent on a cell at t - 1 and at t
  __device__ __forceinline__ int flood(int sr, int sc, int gr, int gc) const {
    return sr == gr && sc == gc ? 0 : audit_flood(free, sr, sc, gr, gc, tid);
  }
};

__global__ __launch_bounds__(64) void mapf_audit_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                        const uint8_t* __restrict__ solved, const int* __restrict__ paths,
                                                        const int* __restrict__ lengths, const int* __restrict__ start,
                                                        const int* __restrict__ goal, int* __restrict__ status,
                                                        int* __restrict__ fault, int* __restrict__ dist,
                                                        int* __restrict__ flow_bound, int* __restrict__ span_bound,
                                                        int* __restrict__ flowtime, int* __restrict__ makespan, int* workspace,
                                                        int N, int T) {
  __shared__ u64 free_rows[MAPF_SIDE];                 // the free cells, for the lanes that are not the cell's row
  __shared__ int own[2][MAPF_SIDE * MAPF_SIDE];
  const int cs = blockIdx.x, lane = threadIdx.x;
  const long long a0 = (long long)cs * N;
  const audit_case k{map + cs * map_stride, H, W, solved, paths + a0 * T * 2, lengths + a0, start + a0 * 2, goal + a0 * 2,
                     workspace + a0 * 2, free_rows, N, T};
  audit_form f{{lane}, own[0], own[1]};
  audit_walk(f, k, audit_out{status, fault, dist, flow_bound, span_bound, flowtime, makespan}, cs);
}

}  // namespace

extern "C" size_t magat_sim_mapf_audit_workspace_bytes(int C, int N, int T) {
  if (C <= 0 || N <= 0 || T <= 0 || N > AUDIT_MAX_N || T > MAPF_MAX_T) return 0;
  return (size_t)C * 2 * (size_t)N * sizeof(int);
}

extern "C" int magat_sim_mapf_audit(const uint8_t* map, int map_batched, int H, int W, const uint8_t* solved, const int32_t* paths,
                                    const int32_t* lengths, const int32_t* start, const int32_t* goal, int32_t* status,
                                    int32_t* fault, int32_t* dist, int32_t* flowtime_bound, int32_t* makespan_bound,
                                    int32_t* flowtime, int32_t* makespan, void* workspace, size_t workspace_bytes, int C, int N,
                                    int T, void* stream) {
  const int rc = audit_entry_check({map, paths, lengths, start, goal, status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan},
                                   H, W, C, N, T, MAPF_SIDE, MAPF_MAX_T, workspace, workspace_bytes,
                                   magat_sim_mapf_audit_workspace_bytes(C, N, T));
  if (rc != MAGAT_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_MAPF_AUDIT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_AUDIT, st);
  hipLaunchKernelGGL(mapf_audit_kernel, dim3((unsigned)C), dim3(64), 0, st, map, map_batched ? (long long)H * W : 0LL, H, W, solved,
                     paths, lengths, start, goal, status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan,
                     static_cast<int*>(workspace), N, T);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
