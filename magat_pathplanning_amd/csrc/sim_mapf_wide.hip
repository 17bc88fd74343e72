// The wide form of the path-finding expert of sim_mapf.hip: the same prioritized planning, cell for cell (restated
// in tests/mapf_restatement.py), on maps up to 256 x 256 with horizons up to 1024.
//   magat_sim_mapf_wide_workspace_bytes   C * T * 6 * rows * words * 8 bytes, rows = 64 * ceil(H / 64), words = 1, 2 or 4 >= W / 64
//   magat_sim_mapf_plan_wide              one workgroup per case plans its agents one after another in `order`
// One workgroup of `rows` threads per case, thread = map row, `words` 64-bit words per row in registers (row_board.h: wide
// boards).  Left / right are multi-word shifts, up / down DPP wave shifts whose boundary rows cross the wavefronts through LDS:
// one __syncthreads per layer, and the votes of the layer (goal reached, set empty; the backtrace's four candidates) ride on it.
//   layers    global workspace [case][t][V, A_up, A_left, A_down, A_right, R][row][word]: the five reservation boards of a layer
//             (zeroed here) and, behind them, the reachable set R_t of the agent being planned.  A thread loads and stores its
//             own row of a board (8 * words contiguous bytes, coalesced over the threads).  The reservation boards do not depend
//             on the search, nor do the R layers on the walk back, so both loops keep WMAPF_AHEAD layers of loads in flight.
//   path      LDS, (row << 8 | col) per step, written by thread 0 in the backtrace; reserving it and writing it out is
//             parallel over t.
// Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_entry.h"      // wide_launch
#include "sim_group.h"                // load_free
#include "sim_mapf_wide_parts.h"      // WMAPF_*, wide_rows / wide_words, wide_layers, wmapf_search, wmapf_backtrace

namespace {

template <int NW>
__global__ __launch_bounds__(WIDE_SIDE) void wmapf_plan_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                               const int* __restrict__ start, const int* __restrict__ goal,
                                                               const int* __restrict__ order, int* paths, int* lengths,
                                                               int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                               int* __restrict__ failed_agent, u64* workspace, int N, int T) {
  __shared__ wide_mail mail;
  __shared__ int cells[WMAPF_MAX_T];      // the path being reserved
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;      // nt = rows
  wide_seat s{&mail, tid & 63, tid >> 6, nt >> 6, 0};
  const long long layer_words = (long long)WMAPF_BOARDS * nt * NW;
  const wide_layers<NW> L{workspace + (long long)cs * T * layer_words, nt};
  for (int t = 0; t < T; ++t)      // the reservation boards; an R layer is written before it is read
    for (int i = tid; i < 5 * nt * NW; i += nt) L.base[t * layer_words + i] = 0ull;
  const wboard<NW> free = load_free<NW>(map + cs * map_stride, H, W, s, tid);
  const long long a0 = (long long)cs * N;
  const int* ord = order ? order + a0 : nullptr;
  int* len = lengths + a0;
  // is `order` a permutation?  N entries in range, none named twice (counted in `lengths`, which is written again below)
  bool bad_order = false;
  if (ord) {
    for (int n = tid; n < N; n += nt) len[n] = 0;
    __syncthreads();
    bool bad = false;
    for (int k = tid; k < N; k += nt) {
      const int a = ord[k];
      if (a < 0 || a >= N || atomicAdd(&len[a], 1) != 0) bad = true;
    }
    wide_post(s, 0, (int)wave_any(bad));
    bad_order = wide_or(s, wide_sync(s), 0) != 0;
  }
  __syncthreads();      // the zeroed boards, and the counts before `lengths` is written
  wboard<NW> starts = wb_zero<NW>(), goals = wb_zero<NW>();      // the planned agents' start and goal cells
  int failed = bad_order ? -2 : -1, longest = 1, k = 0;
  for (; failed == -1 && k < N; ++k) {
    const int a = __builtin_amdgcn_readfirstlane(ord ? ord[k] : k);
    const int sr = start[(a0 + a) * 2], sc = start[(a0 + a) * 2 + 1], gr = goal[(a0 + a) * 2], gc = goal[(a0 + a) * 2 + 1];
    const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
    const wboard<NW> sbit = inside ? wb_bit<NW>(sc) : wb_zero<NW>(), gbit = inside ? wb_bit<NW>(gc) : wb_zero<NW>();
    wide_post(s, 0, (int)wave_any(tid == sr && wb_any(free & ~starts & sbit)) | (int)wave_any(tid == gr && wb_any(free & ~goals & gbit)) << 1);
    const bool ok = wide_or(s, wide_sync(s), 0) == 3;
    const int tstar = ok ? wmapf_search<NW, true>(L, s, free, sr, sc, gr, gc, T, tid, nt) : -1;
    if (tstar < 0) {
      failed = a;
      break;
    }
    wmapf_backtrace<NW, true>(L, s, cells, gr, gc, tstar, W, tid);
    __syncthreads();
    // reserve and write out, threads over t: layer t belongs to one thread, so no two threads touch one word
    int* p = paths + (a0 + a) * T * 2;
    for (int t = tid; t < T; t += nt) {
      const int cell = cells[t < tstar ? t : tstar], cr = cell >> 8, cc = cell & 255;
      L.at(t, 0, cr)[cc >> 6] |= 1ull << (cc & 63);
      if (t >= 1 && t <= tstar) {
        const int from = cells[t - 1], dr = cr - (from >> 8), dc = cc - (from & 255);
        const int d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : dc == 1 ? 3 : 4;
        if (d < 4) L.at(t, 1 + d, cr)[cc >> 6] |= 1ull << (cc & 63);
      }
      p[2 * t] = cr;
      p[2 * t + 1] = cc;
    }
    if (tid == 0) len[a] = tstar + 1;
    if (tid == sr) starts = starts | sbit;
    if (tid == gr) goals = goals | gbit;
    longest = tstar + 1 > longest ? tstar + 1 : longest;
    __syncthreads();      // the next agent loads these boards and reuses `cells`
  }
  // the failing agent and the agents behind it (every agent when `order` is no permutation): the start cell, length 1
  if (failed != -1) {
    for (; k < N; ++k) {
      const int a = failed == -2 ? k : __builtin_amdgcn_readfirstlane(ord ? ord[k] : k);
      const int sr = start[(a0 + a) * 2], sc = start[(a0 + a) * 2 + 1];
      int* p = paths + (a0 + a) * T * 2;
      for (int t = tid; t < T; t += nt) {
        p[2 * t] = sr;
        p[2 * t + 1] = sc;
      }
      if (tid == 0) len[a] = 1;
    }
  }
  if (tid == 0) {
    makespan[cs] = longest - 1;
    solved[cs] = failed == -1 ? 1 : 0;
    failed_agent[cs] = failed;
  }
}

}  // namespace

extern "C" size_t magat_sim_mapf_wide_workspace_bytes(int C, int H, int W, int T) {
  if (C <= 0 || H <= 0 || W <= 0 || T <= 0 || H > WIDE_SIDE || W > WIDE_SIDE) return 0;
  return (size_t)C * T * WMAPF_BOARDS * wide_rows(H) * wide_words(W) * sizeof(u64);
}

extern "C" int magat_sim_mapf_plan_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                                        const int32_t* order, int32_t* paths, int32_t* lengths, int32_t* makespan, uint8_t* solved,
                                        int32_t* failed_agent, void* workspace, size_t workspace_bytes, int C, int N, int T,
                                        void* stream) {
  if (!map || !start || !goal || !paths || !lengths || !makespan || !solved || !failed_agent || !workspace) return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > WIDE_SIDE || W > WIDE_SIDE || T > WMAPF_MAX_T) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_wide_workspace_bytes(C, H, W, T)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)wide_rows(H));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
  magat_form_note(MAGAT_FORM_SIM_MAPF);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF, st);
  wide_launch(wide_words(W), [&](auto nw) {
    hipLaunchKernelGGL(wmapf_plan_kernel<decltype(nw)::value>, grid, block, 0, st, map, map_stride, H, W, start, goal, order, paths, lengths,
                       makespan, solved, failed_agent, ws, N, T);
  });
  magat_prof_end(pid, st);
  return magat_check_launch();
}
