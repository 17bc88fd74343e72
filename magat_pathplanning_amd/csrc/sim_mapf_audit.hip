// Audits schedules of the path-finding expert on the device (the rule is in include/magat_hip.h, restated cell by
// cell in tests/audit_restatement.py): is a schedule a valid MAPF solution, where is its first fault, and how far is its
// flowtime from the classic lower bound, the sum of the agents' obstacle-avoiding shortest distances.
//   magat_sim_mapf_audit_workspace_bytes   per case: the cell of every agent at the steps t - 1 and t, 2 * N ints
//   magat_sim_mapf_audit                   one wavefront per case; one launch, no host round trip; nothing is modified
// The layout of mapf_plan_kernel (sim_mapf.hip): lane = map row, one 64-bit word per row (row_board.h).  Per case:
//   dist        per agent a flood on the free board in registers, reach |= free & (reach and its four shifts), counted until
//               the goal's bit is set; the board standing still first: -1.  For every case, skipped and faulty ones too.
//   stage 1     lanes over t, agent after agent; every lane keeps its smallest fault key, one wave minimum at the end.
//   stage 2     two cell-owner grids in LDS (2 * 64 * 64 ints = 32 KB) for t - 1 and t, lanes over agents: O(N T) per case.
// Stages and keys are sim_mapf_audit_parts.h's.  Integer arithmetic only; every store is a per-lane (vector) store or an LDS
// atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
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

__global__ __launch_bounds__(64) void mapf_audit_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                        const uint8_t* __restrict__ solved, const int* __restrict__ paths,
                                                        const int* __restrict__ lengths, const int* __restrict__ start,
                                                        const int* __restrict__ goal, int* __restrict__ status,
                                                        int* __restrict__ fault, int* __restrict__ dist,
                                                        int* __restrict__ flow_bound, int* __restrict__ span_bound,
                                                        int* __restrict__ flowtime, int* __restrict__ makespan, int* workspace,
                                                        int N, int T) {
  __shared__ u64 free_rows[MAPF_SIDE];                 // the free cells, for the lanes that are not the cell's row
  __shared__ int own[2][MAPF_SIDE * MAPF_SIDE];        // stage 2: the smallest agent on a cell at t - 1 and at t
  const int cs = blockIdx.x, lane = threadIdx.x;
  const long long a0 = (long long)cs * N;
  const int* len = lengths + a0;
  const int* rows = paths + a0 * T * 2;
  const int *st = start + a0 * 2, *gl = goal + a0 * 2;
  const uint8_t* mp = map + cs * map_stride;
  u64 free = 0ull;
  for (int r = 0; r < H; ++r) {
    const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] == 0);
    if (lane == r) free = word;
  }
  free_rows[lane] = free;
  for (int i = lane; i < H * W; i += 64) own[0][i] = own[1][i] = AUDIT_NONE;
  __syncthreads();
  const auto is_free = [&](int r, int c) { return has_bit(free_rows[r], c); };
  // the bounds: they depend on map, start and goal alone
  int bound = 0, longest = 0;
  bool apart = false;
  for (int a = 0; a < N; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const bool s_in = sr >= 0 && sr < H && sc >= 0 && sc < W, g_in = gr >= 0 && gr < H && gc >= 0 && gc < W;
    int d = -1;
    if (s_in && g_in && is_free(sr, sc) && is_free(gr, gc)) d = sr == gr && sc == gc ? 0 : audit_flood(free, sr, sc, gr, gc, lane);
    if (lane == 0) dist[a0 + a] = d;
    apart |= d < 0;
    bound += d;
    longest = d > longest ? d : longest;
  }
  if (lane == 0) {
    flow_bound[cs] = apart ? -1 : bound;
    span_bound[cs] = apart ? -1 : longest;
  }
  if (solved && solved[cs] == 0) {
    if (lane == 0) audit_write(cs, status, fault, flowtime, makespan, 1, 0, -1, -1, -1, 0, 0);
    return;
  }
  const int key1 = wave_all_min(audit_stage1(rows, len, st, gl, N, T, H, W, lane, 64, is_free));
  if (key1 != AUDIT_NONE) {
    if (lane == 0) {
      audit_write(cs, status, fault, flowtime, makespan, 2, 0, -1, -1, -1, 0, 0);
      audit_fault1(key1, len, fault + 4 * cs);
    }
    return;
  }
  int* at = workspace + a0 * 2;
  int t2 = -1;
  const int key2 = audit_stage2(rows, N, T, W, own[0], own[1], at, at + N, lane, 64, [](int key) {
    key = wave_all_min(key);
    __syncthreads();
    return key;
  }, &t2);
  int flow = 0, last = 0;
  for (int base = 0; base < N; base += 64) {
    const int b = base + lane, lb = b < N ? len[b] : 1;
    flow += lb - 1;
    last = lb - 1 > last ? lb - 1 : last;
  }
  flow = wave_all_sum(flow);
  last = wave_all_max(last);
  if (lane == 0) {
    if (key2 == AUDIT_NONE) audit_write(cs, status, fault, flowtime, makespan, 0, 0, -1, -1, -1, flow, last);
    else audit_write(cs, status, fault, flowtime, makespan, 2, 7 + (key2 & 1), t2, key2 >> 13, key2 >> 1 & 4095, 0, 0);
  }
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
  if (!map || !paths || !lengths || !start || !goal || !status || !fault || !dist || !flowtime_bound || !makespan_bound || !flowtime ||
      !makespan || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > MAPF_SIDE || W > MAPF_SIDE || T > MAPF_MAX_T || N > AUDIT_MAX_N) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_audit_workspace_bytes(C, N, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_MAPF_AUDIT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_AUDIT, st);
  hipLaunchKernelGGL(mapf_audit_kernel, dim3((unsigned)C), dim3(64), 0, st, map, map_batched ? (long long)H * W : 0LL, H, W, solved,
                     paths, lengths, start, goal, status, fault, dist, flowtime_bound, makespan_bound, flowtime, makespan,
                     static_cast<int*>(workspace), N, T);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
