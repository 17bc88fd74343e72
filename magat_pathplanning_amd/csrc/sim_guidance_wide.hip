// The wide form of the A*-guided state encodings: GlobalG_S|SD and SemiLG_S|SD on maps up to 256 x 256 (sim_guidance.hip holds
// the form for canvases up to 64 x 64, LocalG and the algorithm's description; the pieces both share are sim_guidance_parts.h).
//   magat_sim_guided_states_wide                   the arguments of magat_sim_guided_states + a workspace
//   magat_sim_replayed_states_wide                 SemiLG with the remembered maps rebuilt from the agents' schedules (no agent_view)
//   magat_sim_guided_states_wide_workspace_bytes   min(B N, GUIDEW_CAP) * canvas rows * canvas columns * 8 bytes
// The search is the narrow form's step for step - pop = lexicographic minimum of (f, g, row, col), closed at push with the first
// pusher as parent, neighbours up, left, down, right - so the tensors EQUAL the reference's.  What changes is where things live:
//   boards     grid/closed and the two parent bits, in LDS as NW 64-bit words a canvas row (word k = columns 64 k .. 64 k + 63),
//              NW = 2 .. 5 >= canvas columns / 64; 3 * rows * NW * 8 bytes, 34 KB at the largest canvas (286 x 286 at FOV 29)
//   open list  one 64-bit entry per cell, f << 36 | g << 18 | row << 9 | col (9-bit coordinates; g, f < 2^18: a serpentine path
//              can visit every cell), room for EVERY canvas cell - a cell is pushed at most once - in the caller's workspace
//   grid       min(B N, GUIDEW_CAP) workgroups of one wavefront; workgroup w owns slab w of the workspace and walks the agents
//              w, w + gridDim.x, ...  A wave reads and writes its own slab only; a wave's memory operations are performed in
//              order, so the wave-scope fences of the narrow form order the list's global stores and loads as they order LDS.
// The pop scans the live entries four independent 64-lane loads at a time, takes one wave-wide minimum of the entries (cells are
// unique in the list, so the minimum names one lane) and lets that lane name its slot.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_guidance_parts.h"

namespace {

constexpr int GUIDEW_SIDE = 256;          // map rows / columns
constexpr int GUIDEW_MAX_WORDS = 5;       // canvas columns <= 256 + 2 * 14 + 2 = 286 at FOV 29
// workgroups of a launch: four one-wave workgroups on each of the 256 compute units, one per SIMD - resident together at every
// canvas size (4 * 34 KB of LDS a compute unit), so the workspace is bounded by the device, not by B * N
constexpr int GUIDEW_CAP = 1024;

__host__ __device__ inline int guidew_words(int Wc) { return Wc <= 128 ? 2 : (Wc + 63) / 64; }
inline size_t guidew_lds_bytes(int Hc, int nw) { return (size_t)3 * Hc * nw * sizeof(u64) + 3 * GUIDE_MAX_WT * sizeof(unsigned); }

__device__ __forceinline__ int guidew_abs(int v) { return v < 0 ? -v : v; }

// REPLAY (magat_sim_replayed_states_wide): SemiLG without `view` - the cells the agent has seen so far are rebuilt from its
// schedule (hist; sim_guidance_parts.h) as NW words a padded row in par0's storage, which the search does not need before the grid
// is built; par0 is zeroed again behind the grid, so the form takes no LDS of its own.
template <int NW, bool REPLAY>
__global__ __launch_bounds__(64) void guided_states_wide_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int Wm,
                                                                const int* __restrict__ pos, const int* __restrict__ goal,
                                                                float* __restrict__ x, int fov, int N, long long agents, int semi,
                                                                int dyn, uint8_t* __restrict__ view, u64* workspace, GuideHistory hist) {
  GUIDE_DYN_LDS(smem_raw);
  const int lane = threadIdx.x;
  const int Wt = fov + 2, half = fov / 2;
  const int Hc = H + 2 * half + 2, Wc = Wm + 2 * half + 2, Hp = H + 2 * half, Wp = Wm + 2 * half;
  u64* unavail = reinterpret_cast<u64*>(smem_raw);                 // [Hc][NW] row masks: grid != 0, or closed
  u64* par0 = unavail + Hc * NW;                                   // [Hc][NW] bit 0 of the parent move
  u64* par1 = par0 + Hc * NW;                                      // [Hc][NW] bit 1
  unsigned* wmap = reinterpret_cast<unsigned*>(par1 + Hc * NW);    // [fov] obstacles in the FOV (outside the map = 1)
  unsigned* wocc = wmap + GUIDE_MAX_WT;                            // [fov] agents in the FOV
  unsigned* pmask = wocc + GUIDE_MAX_WT;                           // [Wt]  channel 1
  u64* open = workspace + (long long)blockIdx.x * Hc * Wc;         // [Hc * Wc] this workgroup's slab
  for (long long ag = blockIdx.x; ag < agents; ag += gridDim.x) {  // b * N + n
    const int b = (int)(ag / N);
    const uint8_t* mp = map + (long long)b * map_stride;
    const int cx = pos[ag * 2], cy = pos[ag * 2 + 1], gx = goal[ag * 2], gy = goal[ag * 2 + 1];
    GUIDE_WAVE_SYNC();                                             // the agent before this one is written out
    for (int i = lane; i < 2 * Hc * NW; i += 64) par0[i] = 0ull;    // par0 and par1; the grid loop below writes every word of unavail
    if (lane < GUIDE_MAX_WT) { wmap[lane] = 0u; wocc[lane] = 0u; pmask[lane] = 0u; }
    GUIDE_WAVE_SYNC();
    const bool pos_in = cx >= 0 && cx < H && cy >= 0 && cy < Wm, goal_in = gx >= 0 && gx < H && gy >= 0 && gy < Wm;
    const bool search = pos_in && goal_in;
    uint8_t* vw = (!REPLAY && semi && search) ? view + ag * (long long)Hp * Wp : nullptr;
    guide_window(mp, H, Wm, pos, b, N, cx, cy, fov, wmap, wocc, vw, lane);
    if constexpr (REPLAY) {
      if (search) {
        // a window is FOV rows of at most two words: lane = (row, which word); the ORs of different cells commute
        guide_history_walk(hist, b, (int)(ag - (long long)b * N), N, H, Wm, lane, [&](int ux, int uy) {
          const int k = (uy >> 6) + (lane & 1);
          const int first = uy > 64 * k ? uy - 64 * k : 0, last = uy + fov - 1 < 64 * k + 63 ? uy + fov - 1 - 64 * k : 63;
          if (lane < 2 * fov && k < NW && last >= first)
            atomicOr(&par0[(ux + (lane >> 1)) * NW + k], ((1ull << (last - first + 1)) - 1ull) << first);
        });
      }
    }
    GUIDE_WAVE_SYNC();
    const int sx = cx + half + 1, sy = cy + half + 1, tx = gx + half + 1, ty = gy + half + 1;      // start and goal on the canvas
    bool found = false;
    if (search) {
      // ---- the grid the search runs on, one ballot per word of a canvas row (lane = column inside the word)
      for (int r = 0; r < Hc; ++r) {
#pragma unroll
        for (int k = 0; k < NW; ++k) {
          const int c = 64 * k + lane;
          int val;
          if constexpr (REPLAY) {
            const bool inner = r >= 1 && r < Hc - 1 && c >= 1 && c < Wc - 1;
            val = guide_canvas_cell_replay(r, c, Hc, Wc, mp, H, Wm, cx, cy, fov, wmap, wocc,
                                           inner && has_bit(par0[(r - 1) * NW + ((c - 1) >> 6)], (c - 1) & 63), tx, ty);
          } else {
            val = guide_canvas_cell(r, c, Hc, Wc, mp, H, Wm, cx, cy, fov, wmap, wocc, semi || dyn, semi != 0, vw, tx, ty);
          }
          const u64 m = __ballot(val != 0);
          if (lane == 0) unavail[r * NW + k] = m;
        }
      }
      GUIDE_WAVE_SYNC();
      if constexpr (REPLAY) {
        for (int i = lane; i < Hc * NW; i += 64) par0[i] = 0ull;      // the seen cells are used up: the parent bits start clear
      }
      // ---- A*
      if (lane == 0) {
        unavail[sx * NW + (sy >> 6)] |= 1ull << (sy & 63);
        open[0] = (u64)(guidew_abs(sx - tx) + guidew_abs(sy - ty)) << 36 | (u64)(sx << 9 | sy);
      }
      GUIDE_WAVE_SYNC();
      int nopen = 1;
      while (nopen > 0) {
        // the lane's minimum and its slot; four loads of a round are independent of each other
        u64 best = ~0ull;
        int at = 0;
        for (int i = lane; i < nopen; i += 256) {
          const int i1 = i + 64, i2 = i + 128, i3 = i + 192;
          const u64 e0 = open[i];
          const u64 e1 = i1 < nopen ? open[i1] : ~0ull;
          const u64 e2 = i2 < nopen ? open[i2] : ~0ull;
          const u64 e3 = i3 < nopen ? open[i3] : ~0ull;
          const u64 a = guide_min(e0, e1), c = guide_min(e2, e3);
          const int ia = e1 < e0 ? i1 : i, ic = e3 < e2 ? i3 : i2;
          const u64 m = guide_min(a, c);
          const int im = c < a ? ic : ia;
          if (m < best) { best = m; at = im; }
        }
        const u64 top = guide_wave_min(best);
        const int owner = __builtin_ctzll(__ballot(best == top));      // entries are unique: one lane holds it
        const int slot = __builtin_amdgcn_readlane(at, owner);
        const int px = (int)((top >> 9) & 511u), py = (int)(top & 511u), g = (int)((top >> 18) & 0x3ffffu);
        if (lane == 0) open[slot] = open[nopen - 1];
        --nopen;
        if (px == tx && py == ty) { found = true; break; }
        GUIDE_WAVE_SYNC();
        bool push = false;
        int x2 = 0, y2 = 0;
        if (lane < 4) {
          x2 = px + (lane == 0 ? -1 : lane == 2 ? 1 : 0);
          y2 = py + (lane == 1 ? -1 : lane == 3 ? 1 : 0);
          push = x2 >= 0 && x2 < Hc && y2 >= 0 && y2 < Wc && !has_bit(unavail[x2 * NW + (y2 >> 6)], y2 & 63);
        }
        const u64 pm = __ballot(push);
        if (push) {
          const u64 bit = 1ull << (y2 & 63);
          const int w = x2 * NW + (y2 >> 6);
          atomicOr(&unavail[w], bit);                      // left and right can share a word
          if (lane & 1) atomicOr(&par0[w], bit);
          if (lane & 2) atomicOr(&par1[w], bit);
          const int g2 = g + 1;
          open[nopen + __popcll(pm & ((1ull << lane) - 1ull))] =
              (u64)(g2 + guidew_abs(x2 - tx) + guidew_abs(y2 - ty)) << 36 | (u64)g2 << 18 | (u64)(x2 << 9 | y2);
        }
        nopen += __popcll(pm);
        GUIDE_WAVE_SYNC();
      }
    }
    GUIDE_WAVE_SYNC();
    // ---- channel 1: the path cells that fall into the agent's window (window row a = canvas row - cx)
    if (lane == 0 && search) {
      auto mark = [&](int r, int c) {
        const int a = r - cx, q = c - cy;
        if (a >= 0 && a < Wt && q >= 0 && q < Wt) pmask[a] |= 1u << q;
      };
      if (found) {
        int ux = tx, uy = ty;
        for (int steps = 0; steps < Hc * Wc && (ux != sx || uy != sy); ++steps) {
          mark(ux, uy);
          const int w = ux * NW + (uy >> 6);
          const int d = (int)has_bit(par0[w], uy & 63) | (int)has_bit(par1[w], uy & 63) << 1;
          ux -= d == 0 ? -1 : d == 2 ? 1 : 0;
          uy -= d == 1 ? -1 : d == 3 ? 1 : 0;
        }
      }
      mark(sx, sy);
    }
    GUIDE_WAVE_SYNC();
    guide_write_states(x + ag * (long long)(3 * Wt * Wt), fov, wmap, wocc, pmask, true, lane);
  }
}

}  // namespace

extern "C" size_t magat_sim_guided_states_wide_workspace_bytes(int B, int N, int H, int W, int FOV) {
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV < 3 || !(FOV & 1) || FOV + 2 > GUIDE_MAX_WT) return 0;
  if (H > GUIDEW_SIDE || W > GUIDEW_SIDE || (long long)B * N > 0x7fffffffLL) return 0;
  const long long agents = (long long)B * N, groups = agents < GUIDEW_CAP ? agents : GUIDEW_CAP;
  const int half = FOV / 2;
  return (size_t)groups * (size_t)(H + 2 * half + 2) * (size_t)(W + 2 * half + 2) * sizeof(u64);
}

namespace {

// the launch both entry points share: the kernel of the canvas's word count, with or without the replay
template <bool REPLAY>
int guidew_launch(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos, const int32_t* goal, float* x, int FOV, int B,
                  int N, int semi, int dyn, uint8_t* view, void* workspace, const GuideHistory& hist, int form, void* stream) {
  const int half = FOV / 2, Hc = H + 2 * half + 2, Wc = W + 2 * half + 2, nw = guidew_words(Wc);
  const long long agents = (long long)B * N;
  const dim3 grid((unsigned)(agents < GUIDEW_CAP ? agents : GUIDEW_CAP)), block(64);
  const size_t lds = guidew_lds_bytes(Hc, nw);                 // <= 3 * 286 * 5 * 8 + 384 bytes
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  u64* ws = static_cast<u64*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(form);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_GUIDED, st);
  switch (nw) {
    case 2:
      hipLaunchKernelGGL((guided_states_wide_kernel<2, REPLAY>), grid, block, lds, st, map, map_stride, H, W, pos, goal, x, FOV, N, agents,
                         semi, dyn, view, ws, hist);
      break;
    case 3:
      hipLaunchKernelGGL((guided_states_wide_kernel<3, REPLAY>), grid, block, lds, st, map, map_stride, H, W, pos, goal, x, FOV, N, agents,
                         semi, dyn, view, ws, hist);
      break;
    case 4:
      hipLaunchKernelGGL((guided_states_wide_kernel<4, REPLAY>), grid, block, lds, st, map, map_stride, H, W, pos, goal, x, FOV, N, agents,
                         semi, dyn, view, ws, hist);
      break;
    default:
      hipLaunchKernelGGL((guided_states_wide_kernel<GUIDEW_MAX_WORDS, REPLAY>), grid, block, lds, st, map, map_stride, H, W, pos, goal, x,
                         FOV, N, agents, semi, dyn, view, ws, hist);
      break;
  }
  magat_prof_end(pid, st);
  return magat_check_launch();
}

}  // namespace

extern "C" int magat_sim_guided_states_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos,
                                            const int32_t* goal, float* x, int FOV, int B, int N, int mode, int dynamic_obstacles,
                                            uint8_t* agent_view, void* workspace, size_t workspace_bytes, void* stream) {
  if (!map || !pos || !goal || !x) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV <= 0 || !(FOV & 1)) return MAGAT_ERR_BAD_SHAPE;
  if (mode != MAGAT_GUIDE_GLOBAL && mode != MAGAT_GUIDE_SEMI) return MAGAT_ERR_UNSUPPORTED;      // LocalG: magat_sim_guided_states
  if (FOV < 3 || FOV + 2 > GUIDE_MAX_WT) return MAGAT_ERR_UNSUPPORTED;
  if (mode == MAGAT_GUIDE_SEMI && !agent_view) return MAGAT_ERR_NULL;
  if ((long long)B * N > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  if (H > GUIDEW_SIDE || W > GUIDEW_SIDE) return MAGAT_ERR_UNSUPPORTED;
  if (!workspace) return MAGAT_ERR_NULL;
  if (workspace_bytes < magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  const int semi = mode == MAGAT_GUIDE_SEMI ? 1 : 0;
  return guidew_launch<false>(map, map_batched, H, W, pos, goal, x, FOV, B, N, semi, dynamic_obstacles ? 1 : 0,
                              semi ? agent_view : nullptr, workspace, GuideHistory{}, MAGAT_FORM_SIM_GUIDED, stream);
}

extern "C" int magat_sim_replayed_states_wide(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos,
                                              const int32_t* goal, float* x, int FOV, int B, int N,
                                              const magat_sim_history_desc* history, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  if (!map || !pos || !goal || !x) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV <= 0 || !(FOV & 1)) return MAGAT_ERR_BAD_SHAPE;
  if (FOV < 3 || FOV + 2 > GUIDE_MAX_WT) return MAGAT_ERR_UNSUPPORTED;
  if ((long long)B * N > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  if (H > GUIDEW_SIDE || W > GUIDEW_SIDE) return MAGAT_ERR_UNSUPPORTED;
  GuideHistory hist;
  const int rc = guide_history_check(history, hist);
  if (rc != MAGAT_OK) return rc;
  if (!workspace) return MAGAT_ERR_NULL;
  if (workspace_bytes < magat_sim_guided_states_wide_workspace_bytes(B, N, H, W, FOV)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
  return guidew_launch<true>(map, map_batched, H, W, pos, goal, x, FOV, B, N, 1, 1, nullptr, workspace, hist, MAGAT_FORM_SIM_REPLAY,
                             stream);
}
