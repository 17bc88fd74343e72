// What the two forms of the A*-guided state kernel share (sim_guidance.hip: canvas up to 64 x 64, everything in LDS;
// sim_guidance_wide.hip: canvas up to 320 columns, the open list in a workspace): the wave-wide minimum, the agent's FOV window,
// the goal marker, one cell of the GlobalG / SemiLG search grid and the state tensor's write-out.  One wavefront per agent.
#pragma once
#include <cstdint>

#include "magat_common.h"

constexpr int GUIDE_MAX_WT = 32;          // FOV + 2: a window row is one 32-bit mask

#define GUIDE_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)

// the kernels' dynamic LDS (tools/host_wave compiles them for the host, where it is the stand-in's buffer)
#ifdef MAGAT_HOST_WAVE
#define GUIDE_DYN_LDS(var) unsigned char* var = reinterpret_cast<unsigned char*>(host_wave::dyn_lds)
#else
#define GUIDE_DYN_LDS(var) extern __shared__ __align__(16) unsigned char var[]
#endif

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

// ---- the replay form of SemiLG (magat_sim_replayed_states[_wide]): the agent's remembered map is rebuilt from its schedule.
// The maps are static and guide_window writes the map's own crop, so the view after step t is
//   view(r, c) = seen(r, c) AND blocked(r - half, c - half),   seen = the union of the FOV x FOV windows (padded rows cell.row ..
//   cell.row + FOV - 1, columns cell.col .. cell.col + FOV - 1) of the agent's cells 0 .. t that lie on the map
// and only `seen` has to be rebuilt - as row masks, right before the search.
constexpr int GUIDE_MAX_STEPS = 1024;     // steps of a history: the wide horizon

// Where the cells of a batch row come from: row b is step row_step[b] of case row_case[b]; agent n's cell at step s is
// table[case][s][n] (expert_schedule's layout), or - the memory's store - cells[case][n][s] = row << 8 | col while s < lengths
// [case][n] and goal[case][n] behind it (expert_schedule_kernel's / expert_pick_kernel's rule).  Exactly one source is set.
struct GuideHistory {
  const int* row_case;         // (B,)
  const int* row_step;         // (B,)
  const int* table;            // (cases, T, N, 2), or null
  const uint16_t* cells;       // (cases, N, Lcap), or null
  const int* lengths;          // (cases, N)
  const int* goal;             // (cases, N, 2)
  int cases, T, Lcap;
};

// Calls window(row, col) - wave-uniform arguments, every lane - once for each cell of agent n's history in batch row b that lies
// on the map; a cell that repeats the one before it (a wait, the padding behind a path) is skipped.  The steps are loaded 64 at a
// time, lane = step, and broadcast from there.  case and step are clamped into the source: nothing is read outside it.
template <typename F>
__device__ __forceinline__ void guide_history_walk(const GuideHistory& h, int b, int n, int N, int H, int Wm, int lane, F&& window) {
  int c = __builtin_amdgcn_readfirstlane(h.row_case[b]), t = __builtin_amdgcn_readfirstlane(h.row_step[b]);
  const int tmax = (h.table ? h.T : GUIDE_MAX_STEPS) - 1;
  c = c < 0 ? 0 : (c >= h.cases ? h.cases - 1 : c);
  t = t < 0 ? 0 : (t > tmax ? tmax : t);
  const long long ag = (long long)c * N + n;
  int L = 0, gx = 0, gy = 0;
  if (!h.table) {
    L = h.lengths[ag];
    L = L < 0 ? 0 : (L > h.Lcap ? h.Lcap : L);      // never read behind the row
    gx = h.goal[2 * ag];
    gy = h.goal[2 * ag + 1];
  }
  int lastx = -1, lasty = -1;
  for (int s0 = 0; s0 <= t; s0 += 64) {
    const int s = s0 + lane;
    int rx = -1, ry = -1;
    if (s <= t) {
      if (h.table) {
        const long long i = (((long long)c * h.T + s) * N + n) * 2;
        rx = h.table[i];
        ry = h.table[i + 1];
      } else if (s < L) {
        const unsigned v = h.cells[ag * h.Lcap + s];
        rx = (int)(v >> 8);
        ry = (int)(v & 255u);
      } else {
        rx = gx;
        ry = gy;
      }
    }
    const int cnt = t - s0 + 1 < 64 ? t - s0 + 1 : 64;
    for (int j = 0; j < cnt; ++j) {
      const int ux = __builtin_amdgcn_readlane(rx, j), uy = __builtin_amdgcn_readlane(ry, j);
      if (ux == lastx && uy == lasty) continue;
      lastx = ux;
      lasty = uy;
      if (ux >= 0 && ux < H && uy >= 0 && uy < Wm) window(ux, uy);
    }
  }
}

// guide_canvas_cell of the replay form: a cell outside the current FOV holds `seen` AND blocked(cell) - a padding-ring cell that
// was never seen is free, a seen one is blocked: what the carried byte view holds.  seen: the bit of padded cell (r - 1, c - 1),
// read only inside the ring.  The agents inside the FOV always block (SemiLG).
__device__ __forceinline__ int guide_canvas_cell_replay(int r, int c, int Hc, int Wc, const uint8_t* __restrict__ mp, int H, int Wm,
                                                        int cx, int cy, int fov, const unsigned* wmap, const unsigned* wocc, bool seen,
                                                        int tx, int ty) {
  int val = 0;
  if (r >= 1 && r < Hc - 1 && c >= 1 && c < Wc - 1) {
    const int half = fov / 2;
    const int mr = r - 1 - half, mc = c - 1 - half;
    const int fa = mr - cx + half, fc = mc - cy + half;
    const bool infov = fa >= 0 && fa < fov && fc >= 0 && fc < fov;
    if (infov) val = (int)((wmap[fa] >> fc) & 1u) + (int)((wocc[fa] >> fc) & 1u);
    else if (seen) val = (mr >= 0 && mr < H && mc >= 0 && mc < Wm) ? (mp[(long long)mr * Wm + mc] != 0 ? 1 : 0) : 1;
    if (r == tx && c == ty && val == 1) val = 0;
  }
  return val;
}

// the history's checks of the two replay entry points, before anything is launched (MAGAT_OK, or the code to return)
inline int guide_history_check(const magat_sim_history_desc* h, GuideHistory& out) {
  if (!h || !h->row_case || !h->row_step) return MAGAT_ERR_NULL;
  const bool table = h->pos_table != nullptr, store = h->cells || h->lengths || h->goal;
  if (table && store) return MAGAT_ERR_UNSUPPORTED;      // both sources
  if (!table && !(h->cells && h->lengths && h->goal)) return MAGAT_ERR_NULL;      // neither, or half a store
  if (h->cases <= 0 || (table ? h->T <= 0 : h->Lcap <= 0)) return MAGAT_ERR_BAD_SHAPE;
  if (table && h->T > GUIDE_MAX_STEPS) return MAGAT_ERR_UNSUPPORTED;
  out = GuideHistory{h->row_case, h->row_step, h->pos_table, h->cells, h->lengths, h->goal, h->cases, table ? h->T : 0, table ? 0 : h->Lcap};
  return MAGAT_OK;
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
