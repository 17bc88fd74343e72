// What the two forms of the A*-guided state kernel share (sim_guidance.hip: canvas up to 64 x 64, everything in LDS;
// sim_guidance_wide.hip: canvas up to 320 columns, the open list in a workspace): the wave-wide minimum, the agent's FOV window,
// the goal marker, one cell of the GlobalG / SemiLG search grid and the state tensor's write-out.  One wavefront per agent.
#pragma once
#include <cstdint>

#include "magat_common.h"

constexpr int GUIDE_MAX_WT = 32;          // FOV + 2: a window row is one 32-bit mask

#define GUIDE_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

template <int CTRL>
__device__ __forceinline__ unsigned long long guide_dpp_u64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, true);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
__device__ __forceinline__ unsigned long long guide_lane_u64(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
__device__ __forceinline__ unsigned long long guide_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
// wave-uniform minimum (all 64 lanes active): the rotations inside each row of 16 lanes, then the four rows
__device__ __forceinline__ unsigned long long guide_wave_min(unsigned long long v) {
  v = guide_min(v, guide_dpp_u64<0x128>(v));
  v = guide_min(v, guide_dpp_u64<0x124>(v));
  v = guide_min(v, guide_dpp_u64<0x122>(v));
  v = guide_min(v, guide_dpp_u64<0x121>(v));
  return guide_min(guide_min(guide_lane_u64(v, 0), guide_lane_u64(v, 16)), guide_min(guide_lane_u64(v, 32), guide_lane_u64(v, 48)));
}

// The agent's FOV window into wmap / wocc [fov] (zeroed by the caller, a wave sync before and after): the agents of instance b
// that stand inside it (setPosAgents + the FOV crop, :88-99) and its obstacles (outside the map = obstacle).  SemiLG (vw != null)
// writes the obstacle crop into the agent's remembered map BEFORE the search (:356-357), so that the grid only reads that map.
__device__ __forceinline__ void guide_window(const uint8_t* __restrict__ mp, int H, int Wm, const int* __restrict__ pos, int b, int N,
                                             int cx, int cy, int fov, unsigned* wmap, unsigned* wocc, uint8_t* vw, int lane) {
  const int half = fov / 2, Wp = Wm + 2 * half;
  for (int n = lane; n < N; n += 64) {
    const int px = pos[((long long)b * N + n) * 2], py = pos[((long long)b * N + n) * 2 + 1];
    const int ax = px - cx + half, ay = py - cy + half;
    if (px >= 0 && px < H && py >= 0 && py < Wm && ax >= 0 && ax < fov && ay >= 0 && ay < fov) atomicOr(&wocc[ax], 1u << ay);
  }
  for (int idx = lane; idx < fov * fov; idx += 64) {
    const int a = idx / fov, q = idx - a * fov;
    const int r = cx - half + a, c = cy - half + q;
    const bool blocked = (r >= 0 && r < H && c >= 0 && c < Wm) ? mp[(long long)r * Wm + c] != 0 : true;
    if (blocked) atomicOr(&wmap[a], 1u << q);
    if (vw) vw[(long long)(r + half) * Wp + (c + half)] = blocked ? 1 : 0;      // pos inside the map: the crop lies inside the padded map
  }
}

// the goal marker of 'Project_G' (fov_states_kernel): the goal itself inside the FOV, else projectedgoal (:101-120)
__device__ __forceinline__ void guide_goal_marker(int cx, int cy, int gx, int gy, bool goal_in, int fov, int& grow, int& gcol) {
  const int half = fov / 2, dist = (fov + 2) / 2;
  const int dx = gx - cx, dy = gy - cy;
  if (goal_in && dx >= -half && dx <= half && dy >= -half && dy <= half) {
    grow = dx + half + 1;
    gcol = dy + half + 1;
  } else {
    const int ady = dy < 0 ? -dy : dy, adx = dx < 0 ? -dx : dx;
    const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
    if (ady >= adx) {
      gcol = dist * (sy + 1);
      grow = (int)((double)dist + rint((double)dist * (double)dx / (double)ady));
    } else {
      grow = dist * (sx + 1);
      gcol = (int)((double)dist + rint((double)dist * (double)dy / (double)adx));
    }
  }
}

// Cell (r, c) of the GlobalG / SemiLG search grid, non-zero = blocked: the map padded by FOV/2 obstacle cells (GlobalG) or the
// agent's remembered map vr with the current FOV crop already written into it (SemiLG, :356-357), plus the agents inside the FOV
// ('_SD'; SemiLG always, :359), inside a free one-cell ring; the goal cell (tx, ty) is cleared when it holds exactly 1 (:372-374,
// :464-465).  Cells outside the Hc x Wc canvas are 0.
__device__ __forceinline__ int guide_canvas_cell(int r, int c, int Hc, int Wc, const uint8_t* __restrict__ mp, int H, int Wm, int cx,
                                                 int cy, int fov, const unsigned* wmap, const unsigned* wocc, bool agents,
                                                 bool semi, const uint8_t* vr, int tx, int ty) {
  int val = 0;
  if (r >= 1 && r < Hc - 1 && c >= 1 && c < Wc - 1) {
    const int half = fov / 2, Wp = Wm + 2 * half;
    const int pr = r - 1, pc = c - 1, mr = pr - half, mc = pc - half;
    const int fa = mr - cx + half, fc = mc - cy + half;
    const bool infov = fa >= 0 && fa < fov && fc >= 0 && fc < fov;
    if (infov) val = (int)((wmap[fa] >> fc) & 1u) + (agents ? (int)((wocc[fa] >> fc) & 1u) : 0);
    else if (semi) val = vr[(long long)pr * Wp + pc];
    else val = (mr >= 0 && mr < H && mc >= 0 && mc < Wm) ? (mp[(long long)mr * Wm + mc] != 0 ? 1 : 0) : 1;
    if (r == tx && c == ty && val == 1) val = 0;
  }
  return val;
}

// (3, FOV+2, FOV+2) floats of one agent: channel 0 the window's obstacles, 1 the path mask, 2 the window's agents
__device__ __forceinline__ void guide_write_states(float* __restrict__ xa, int fov, const unsigned* wmap, const unsigned* wocc,
                                                   const unsigned* pmask, bool agents_out, int lane) {
  const int Wt = fov + 2;
  for (int idx = lane; idx < 3 * Wt * Wt; idx += 64) {
    const int ch = idx / (Wt * Wt), pix = idx - ch * Wt * Wt;
    const int a = pix / Wt, c = pix - a * Wt;
    unsigned bit = 0u;
    if (ch == 1) bit = (pmask[a] >> c) & 1u;
    else if (a >= 1 && a <= fov && c >= 1 && c <= fov) bit = ch == 0 ? (wmap[a - 1] >> (c - 1)) & 1u : (agents_out ? (wocc[a - 1] >> (c - 1)) & 1u : 0u);
    xa[idx] = bit ? 1.f : 0.f;
  }
}
