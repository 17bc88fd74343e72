// The wide form of the schedule audit of sim_mapf_audit.hip: the same rule, cell for cell (include/magat_hip.h;
// restated in tests/audit_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_audit_wide_workspace_bytes   per case: the two cell-owner grids, 2 * H * W ints, and the cell of every agent
//                                               at the steps t - 1 and t, 2 * N ints
//   magat_sim_mapf_audit_wide                   one workgroup per case; one launch, no host round trip; nothing is modified
// The layout of wmapf_plan_kernel (sim_mapf_wide.hip): `rows` threads, thread = map row, `words` 64-bit words per row in
// registers, votes and minima across the wavefronts through the LDS mail (row_board.h).  Per case:
//   dist        per agent a flood on the free board, one barrier per step as in the wide planner's layer loop: the boundary rows
//               and the votes (the goal is reached; the board still grows) travel in one round of the mail.
//   stage 1     threads over t, agent after agent; the free rows of the map in LDS for the threads that are not the cell's row.
//   stage 2     the two cell-owner grids in the caller's workspace (set to "nobody" here, then only the cells that were set are
//               cleared), threads over agents, global atomicMin.
// Stages and keys are sim_mapf_audit_parts.h's.  All control flow around a barrier is uniform over the workgroup.  Every store
// is a per-lane (vector) store or a global atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
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
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_audit_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                                const uint8_t* __restrict__ solved, const int* __restrict__ paths,
                                                                const int* __restrict__ lengths, const int* __restrict__ start,
                                                                const int* __restrict__ goal, int* __restrict__ status,
                                                                int* __restrict__ fault, int* __restrict__ dist,
                                                                int* __restrict__ flow_bound, int* __restrict__ span_bound,
                                                                int* __restrict__ flowtime, int* __restrict__ makespan,
                                                                int* workspace, int N, int T) {
  __shared__ wide_mail mail;
  __shared__ u64 free_rows[WIDE_SIDE][NW];      // the free cells, for the threads that are not the cell's row
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = rows
  wide_seat s{&mail, tid & 63, tid >> 6, nt >> 6, 0};
  const long long a0 = (long long)cs * N;
  const int* len = lengths + a0;
  const int* rows = paths + a0 * T * 2;
  const int *st = start + a0 * 2, *gl = goal + a0 * 2;
  int* own = workspace + cs * waudit_case_ints(H, W, N);
  int* at = own + 2LL * H * W;
  // free cells: the rows of this wave, each read by the lanes over its columns, one ballot per word; rows >= H and bits >= W
  // stay zero
  const uint8_t* mp = map + cs * map_stride;
  wboard<NW> free = wb_zero<NW>();
  for (int r = 64 * s.wave; r < H && r < 64 * s.wave + 64; ++r) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const int col = 64 * k + s.lane;
      const u64 word = __builtin_amdgcn_ballot_w64(col < W && mp[r * W + (col < W ? col : 0)] == 0);
      if (tid == r) free.w[k] = word;
    }
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) free_rows[tid][k] = free.w[k];
  for (int i = tid; i < 2 * H * W; i += nt) own[i] = AUDIT_NONE;
  __syncthreads();
  const auto is_free = [&](int r, int c) { return has_bit(free_rows[r][c >> 6], c & 63); };
  // the bounds: they depend on map, start and goal alone
  int bound = 0, longest = 0;
  bool apart = false;
  for (int a = 0; a < N; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const bool s_in = sr >= 0 && sr < H && sc >= 0 && sc < W, g_in = gr >= 0 && gr < H && gc >= 0 && gc < W;
    int d = -1;
    if (s_in && g_in && is_free(sr, sc) && is_free(gr, gc)) d = waudit_flood<NW>(s, free, sr, sc, gr, gc, tid);
    if (tid == 0) dist[a0 + a] = d;
    apart |= d < 0;
    bound += d;
    longest = d > longest ? d : longest;
  }
  if (tid == 0) {
    flow_bound[cs] = apart ? -1 : bound;
    span_bound[cs] = apart ? -1 : longest;
  }
  if (solved && solved[cs] == 0) {
    if (tid == 0) audit_write(cs, status, fault, flowtime, makespan, 1, 0, -1, -1, -1, 0, 0);
    return;
  }
  const auto group_min = [&](int key) {
    wide_post(s, 0, wave_all_min(key));
    return wide_min(s, wide_sync(s), 0);
  };
  const int key1 = group_min(audit_stage1(rows, len, st, gl, N, T, H, W, tid, nt, is_free));
  if (key1 != AUDIT_NONE) {
    if (tid == 0) {
      audit_write(cs, status, fault, flowtime, makespan, 2, 0, -1, -1, -1, 0, 0);
      audit_fault1(key1, len, fault + 4 * cs);
    }
    return;
  }
  int t2 = -1;
  const int key2 = audit_stage2(rows, N, T, W, own, own + H * W, at, at + N, tid, nt, group_min, &t2);
  int flow = 0, last = 0;
  for (int base = 0; base < N; base += nt) {
    const int b = base + tid, lb = b < N ? len[b] : 1;
    flow += lb - 1;
    last = lb - 1 > last ? lb - 1 : last;
  }
  wide_post(s, 0, wave_all_sum(flow));
  wide_post(s, 1, wave_all_max(last));
  const int p = wide_sync(s);
  if (tid == 0) {
    if (key2 == AUDIT_NONE)
      audit_write(cs, status, fault, flowtime, makespan, 0, 0, -1, -1, -1, wide_sum(s, p, 0), wide_max(s, p, 1));
    else audit_write(cs, status, fault, flowtime, makespan, 2, 7 + (key2 & 1), t2, key2 >> 13, key2 >> 1 & 4095, 0, 0);
  }
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
  if (!map || !paths || !lengths || !start || !goal || !status || !fault || !dist || !flowtime_bound || !makespan_bound || !flowtime ||
      !makespan || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > WIDE_SIDE || W > WIDE_SIDE || T > WMAPF_MAX_T || N > AUDIT_MAX_N) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  int* ws = static_cast<int*>(workspace);
  magat_form_note(MAGAT_FORM_SIM_MAPF_AUDIT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_AUDIT, st);
  switch (wide_words(W)) {      // static LDS only: the free rows (2, 4 or 8 KB) and the mail
    case 1:
      hipLaunchKernelGGL(wmapf_audit_kernel<1>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, start, goal, status,
                         fault, dist, flowtime_bound, makespan_bound, flowtime, makespan, ws, N, T);
      break;
    case 2:
      hipLaunchKernelGGL(wmapf_audit_kernel<2>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, start, goal, status,
                         fault, dist, flowtime_bound, makespan_bound, flowtime, makespan, ws, N, T);
      break;
    default:
      hipLaunchKernelGGL(wmapf_audit_kernel<4>, grid, block, 0, st, map, map_stride, H, W, solved, paths, lengths, start, goal, status,
                         fault, dist, flowtime_bound, makespan_bound, flowtime, makespan, ws, N, T);
      break;
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}
