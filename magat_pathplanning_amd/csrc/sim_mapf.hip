// A multi-agent path-finding expert for C cases at once: prioritized planning with an exact space-time search per agent
// (restated cell by cell in tests/mapf_restatement.py).  It is NOT ECBS: no bound on the flowtime, and a case
// can stay unsolved in a given priority order.
//   magat_sim_mapf_workspace_bytes   the reservation boards: 5 * T * 64 * 8 bytes per case
//   magat_sim_mapf_plan              one wavefront per case plans its agents one after another in `order`
// One wavefront per case, lane = map row, one 64-bit word per row (H, W <= 64): a whole board - the free cells, a reachable
// set R_t, a reservation layer - is one register pair across the wave.  Moving a board left / right is a 64-bit shift,
// up / down a DPP wave shift.  Everything is integer and bit arithmetic.
//   reservation boards   global workspace [case][t][V, A_up, A_left, A_down, A_right][row]: a board is one coalesced 512-byte load;
//                        zeroed here.  They do not depend on the search, so they are loaded MAPF_AHEAD layers ahead.
//   R layers             LDS, T * 512 bytes; every lane writes and reads only its own row, the backtrace tests each source cell
//                        on the lane that owns its row.
//   path of one agent    LDS, (row << 8 | col) per step, written by lane 0 in the backtrace; reserving it and writing it out
//                        is parallel over t.
// Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"      // u64, wave_shift, cells_up / cells_down, wave_any, has_bit
#include "sim_group.h"      // load_free
#include "sim_mapf_parts.h"   // MAPF_*, board_row, mapf_search, mapf_backtrace

namespace {

__global__ __launch_bounds__(64) void mapf_plan_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                       const int* __restrict__ start, const int* __restrict__ goal,
                                                       const int* __restrict__ order, int* paths, int* lengths,
                                                       int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                       int* __restrict__ failed_agent, u64* workspace, int N, int T) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  u64* R = reinterpret_cast<u64*>(smem_raw);      // [T][64]
  __shared__ int cells[MAPF_MAX_T];               // the path being reserved
  const int cs = blockIdx.x, lane = threadIdx.x;
  u64* boards = workspace + (long long)cs * T * MAPF_BOARDS * MAPF_SIDE;
  for (int i = lane; i < T * MAPF_BOARDS * MAPF_SIDE; i += 64) boards[i] = 0ull;
  const u64 free = load_free(map + cs * map_stride, H, W, lane);
  const long long a0 = (long long)cs * N;
  const int* ord = order ? order + a0 : nullptr;
  int* len = lengths + a0;
  // is `order` a permutation?  N entries in range, none named twice (counted in `lengths`, which is written again below)
  bool bad_order = false;
  if (ord) {
    for (int n = lane; n < N; n += 64) len[n] = 0;
    __syncthreads();
    for (int k = lane; k < N; k += 64) {
      const int a = ord[k];
      if (a < 0 || a >= N || atomicAdd(&len[a], 1) != 0) bad_order = true;
    }
    bad_order = wave_any(bad_order);
  }
  __syncthreads();      // the zeroed boards, and the counts before `lengths` is written
  u64 starts = 0ull, goals = 0ull;      // the planned agents' start and goal cells
  int failed = bad_order ? -2 : -1, longest = 1, k = 0;
  for (; failed == -1 && k < N; ++k) {
    const int a = __builtin_amdgcn_readfirstlane(ord ? ord[k] : k);
    const int sr = start[(a0 + a) * 2], sc = start[(a0 + a) * 2 + 1], gr = goal[(a0 + a) * 2], gc = goal[(a0 + a) * 2 + 1];
    const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
    const u64 sbit = inside ? 1ull << sc : 0ull, gbit = inside ? 1ull << gc : 0ull;
    const bool ok = wave_any(lane == sr && (free & ~starts & sbit)) && wave_any(lane == gr && (free & ~goals & gbit));
    const int tstar = ok ? mapf_search<true>(boards, R, free, sr, sc, gr, gc, T, lane) : -1;
    if (tstar < 0) {
      failed = a;
      break;
    }
    mapf_backtrace<true>(boards, R, cells, gr, gc, tstar, W, lane);
    __syncthreads();
    // reserve and write out, lanes over t: layer t belongs to one lane, so no two lanes touch one word
    int* p = paths + (a0 + a) * T * 2;
    for (int t = lane; t < T; t += 64) {
      const int cell = cells[t < tstar ? t : tstar], cr = cell >> 8, cc = cell & 255;
      boards[((long long)t * MAPF_BOARDS) * MAPF_SIDE + cr] |= 1ull << cc;
      if (t >= 1 && t <= tstar) {
        const int from = cells[t - 1], dr = cr - (from >> 8), dc = cc - (from & 255);
        const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : dc == 1 ? 3 : 4;
        if (d < 4) boards[((long long)t * MAPF_BOARDS + 1 + d) * MAPF_SIDE + cr] |= 1ull << cc;
      }
      p[2 * t] = cr;
      p[2 * t + 1] = cc;
    }
    if (lane == 0) len[a] = tstar + 1;
    if (lane == sr) starts |= sbit;
    if (lane == gr) goals |= gbit;
    longest = tstar + 1 > longest ? tstar + 1 : longest;
    __syncthreads();      // the next agent loads these boards and reuses `cells`
  }
  // the failing agent and the agents behind it (every agent when `order` is no permutation): the start cell, length 1
  if (failed != -1) {
    for (; k < N; ++k) {
      const int a = failed == -2 ? k : __builtin_amdgcn_readfirstlane(ord ? ord[k] : k);
      const int sr = start[(a0 + a) * 2], sc = start[(a0 + a) * 2 + 1];
      int* p = paths + (a0 + a) * T * 2;
      for (int t = lane; t < T; t += 64) {
        p[2 * t] = sr;
        p[2 * t + 1] = sc;
      }
      if (lane == 0) len[a] = 1;
    }
  }
  if (lane == 0) {
    makespan[cs] = longest - 1;
    solved[cs] = failed == -1 ? 1 : 0;
    failed_agent[cs] = failed;
  }
}

}  // namespace

extern "C" size_t magat_sim_mapf_workspace_bytes(int C, int T) {
  if (C <= 0 || T <= 0) return 0;
  return (size_t)C * T * MAPF_BOARDS * MAPF_SIDE * sizeof(u64);
}

extern "C" int magat_sim_mapf_plan(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                                   const int32_t* order, int32_t* paths, int32_t* lengths, int32_t* makespan, uint8_t* solved,
                                   int32_t* failed_agent, void* workspace, size_t workspace_bytes, int C, int N, int T,
                                   void* stream) {
  if (!map || !start || !goal || !paths || !lengths || !makespan || !solved || !failed_agent || !workspace) return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > MAPF_SIDE || W > MAPF_SIDE || T > MAPF_MAX_T) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_workspace_bytes(C, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  const size_t lds = (size_t)T * MAPF_SIDE * sizeof(u64);      // <= 128 KB, + 1 KB static
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds > 64 * 1024 && magat_ensure_dyn_lds(reinterpret_cast<const void*>(&mapf_plan_kernel), MAGAT_LDS_SIM_MAPF, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  magat_form_note(MAGAT_FORM_SIM_MAPF);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF, st);
  hipLaunchKernelGGL(mapf_plan_kernel, dim3((unsigned)C), dim3(64), lds, st, map, map_batched ? (long long)H * W : 0LL, H, W, start,
                     goal, order, paths, lengths, makespan, solved, failed_agent, static_cast<u64*>(workspace), N, T);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
