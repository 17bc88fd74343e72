// A*-guided state encodings of the reference's state encoder on the device (dataloader/statetransformer_Guidance.py:241-495,
// config.guidance = LocalG_S|SD, GlobalG_S|SD, SemiLG_S|SD; the planner is offlineExpert/a_star.py:75-189).
//   magat_sim_replayed_states the SemiLG encoding with the remembered maps rebuilt from the agents' schedules (no agent_view)
//   magat_sim_guided_states   obstacle map + agent / goal coordinates (+ the agents' remembered maps) -> the
//                             (B,N,3,FOV+2,FOV+2) {0,1} state tensor whose channel 1 holds the cells of the reference's A* path
// The output is integer work and must EQUAL the reference's, so the search is the reference's step for step:
//   4-connected, unit cost, neighbours in the order up, left, down, right; heuristic |dr| + |dc|; the popped entry is the
//   lexicographic minimum of (f, g, row, col); a cell is closed when it is PUSHED and keeps its first pusher as parent; a cell is
//   entered only where the grid is 0; the start cell is never tested; an empty open list ends the search with the path [start].
// One wavefront per agent (the search is sequential, there are B x N of them): the grid, the closed set and the parents are
// 64-bit row masks in LDS, the open list one 32-bit word per entry - g << 12 | row << 6 | col - with room for EVERY cell of
// the canvas (a cell is pushed at most once, so the list cannot overflow).  The pop is a strided scan of the list and one
// wave-wide minimum of the packed (f, g, row, col, slot) keys through DPP row rotations; the four pushes are done by four lanes.
#include <cstdint>

#include "magat_common.h"
#include "sim_guidance_parts.h"

namespace {

constexpr int GUIDE_MAX_CANVAS = 64;      // rows / columns of the search canvas: a row is one 64-bit mask, coordinates take 6 bits
constexpr size_t GUIDE_LDS_HEAD = 3 * GUIDE_MAX_CANVAS * sizeof(unsigned long long) + 3 * GUIDE_MAX_WT * sizeof(unsigned);

// REPLAY (magat_sim_replayed_states): SemiLG without `view` - the wave first rebuilds which cells the agent has seen from its
// schedule (hist; sim_guidance_parts.h), one 64-bit mask per padded row held by lane = row, and the grid reads that.
template <bool REPLAY>
__global__ __launch_bounds__(64) void guided_states_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int Wm,
                                                           const int* __restrict__ pos, const int* __restrict__ goal,
                                                           float* __restrict__ x, int fov, int N, int mode, int dyn,
                                                           uint8_t* __restrict__ view, GuideHistory hist) {
  GUIDE_DYN_LDS(smem_raw);
  const int lane = threadIdx.x;
  const long long ag = blockIdx.x;                       // b * N + n
  const int b = (int)(ag / N);
  const int Wt = fov + 2, half = fov / 2, dist = Wt / 2;
  unsigned long long* unavail = reinterpret_cast<unsigned long long*>(smem_raw);      // [64] row masks: grid != 0, or closed
  unsigned long long* par0 = unavail + GUIDE_MAX_CANVAS;                              // [64] bit 0 of the parent move
  unsigned long long* par1 = par0 + GUIDE_MAX_CANVAS;                                 // [64] bit 1
  unsigned* wmap = reinterpret_cast<unsigned*>(par1 + GUIDE_MAX_CANVAS);              // [fov] obstacles in the FOV (outside the map = 1)
  unsigned* wocc = wmap + GUIDE_MAX_WT;                                               // [fov] agents in the FOV
  unsigned* pmask = wocc + GUIDE_MAX_WT;                                              // [Wt]  channel 1
  unsigned* open = pmask + GUIDE_MAX_WT;                                              // [canvas cells]
  const uint8_t* mp = map + (long long)b * map_stride;
  const int cx = pos[ag * 2], cy = pos[ag * 2 + 1], gx = goal[ag * 2], gy = goal[ag * 2 + 1];
  unavail[lane] = 0ull;
  par0[lane] = 0ull;
  par1[lane] = 0ull;
  if (lane < GUIDE_MAX_WT) { wmap[lane] = 0u; wocc[lane] = 0u; pmask[lane] = 0u; }
  GUIDE_WAVE_SYNC();
  const bool local = mode == MAGAT_GUIDE_LOCAL, semi = mode == MAGAT_GUIDE_SEMI;
  const bool pos_in = cx >= 0 && cx < H && cy >= 0 && cy < Wm, goal_in = gx >= 0 && gx < H && gy >= 0 && gy < Wm;
  const bool search = pos_in && goal_in;
  // the agents and the obstacles inside the FOV; SemiLG writes the obstacle crop into the agent's remembered map (guide_window)
  const int Hp = H + 2 * half, Wp = Wm + 2 * half;
  uint8_t* vw = (!REPLAY && semi && search) ? view + ag * (long long)Hp * Wp : nullptr;
  guide_window(mp, H, Wm, pos, b, N, cx, cy, fov, wmap, wocc, vw, lane);
  GUIDE_WAVE_SYNC();
  unsigned long long seen = 0ull;                        // REPLAY: padded row `lane` of the cells seen so far
  if constexpr (REPLAY) {
    if (search) {
      const unsigned long long span = (1ull << fov) - 1ull;      // a window's columns, shifted to its first
      guide_history_walk(hist, b, (int)(ag - (long long)b * N), N, H, Wm, lane, [&](int ux, int uy) {
        if (lane >= ux && lane < ux + fov) seen |= span << uy;
      });
    }
  }
  int grow, gcol;
  guide_goal_marker(cx, cy, gx, gy, goal_in, fov, grow, gcol);
  const int Hc = local ? Wt : H + 2 * half + 2, Wc = local ? Wt : Wm + 2 * half + 2;
  const int sx = local ? dist : cx + half + 1, sy = local ? dist : cy + half + 1;      // start and goal on the canvas
  const int tx = local ? grow : gx + half + 1, ty = local ? gcol : gy + half + 1;
  // ---- the grid the search runs on, one ballot per canvas row (lane = column)
  if (local) {
    // window map + (only '_SD') the agents in it, inside a FREE one-cell ring; centre cleared; the goal cell cleared when an
    // agent stands on it (:284-291; '_S' has no agents in its channel, so nothing collides there)
    const bool goal_inner = grow >= 1 && grow <= fov && gcol >= 1 && gcol <= fov;
    const bool collide = dyn && goal_inner && ((wocc[grow - 1] >> (gcol - 1)) & 1u);
    for (int r = 0; r < Hc; ++r) {
      int val = 0;
      if (r >= 1 && r <= fov && lane >= 1 && lane <= fov) {
        val = (int)((wmap[r - 1] >> (lane - 1)) & 1u) + (dyn ? (int)((wocc[r - 1] >> (lane - 1)) & 1u) : 0);
        if (r == dist && lane == dist) val = 0;
        if (collide && r == grow && lane == gcol) val = 0;
      }
      const unsigned long long m = __ballot(val != 0);
      if (lane == 0) unavail[r] = m;
    }
  } else if (search) {
    // the padded map or the agent's remembered map, the agents in the FOV, the free ring, the cleared goal (guide_canvas_cell)
    for (int r = 0; r < Hc; ++r) {
      int val;
      if constexpr (REPLAY) {
        const unsigned long long row = (r >= 1 && r < Hc - 1) ? guide_lane_u64(seen, r - 1) : 0ull;
        val = guide_canvas_cell_replay(r, lane, Hc, Wc, mp, H, Wm, cx, cy, fov, wmap, wocc,
                                       lane >= 1 && ((row >> ((lane - 1) & 63)) & 1ull), tx, ty);
      } else {
        val = guide_canvas_cell(r, lane, Hc, Wc, mp, H, Wm, cx, cy, fov, wmap, wocc, semi || dyn, semi, vw, tx, ty);
      }
      const unsigned long long m = __ballot(val != 0);
      if (lane == 0) unavail[r] = m;
    }
  }
  GUIDE_WAVE_SYNC();
  // ---- A*
  bool found = false;
  if (search) {
    if (lane == 0) {
      unavail[sx] |= 1ull << sy;
      open[0] = (unsigned)(sx << 6 | sy);
    }
    GUIDE_WAVE_SYNC();
    int nopen = 1;
    while (nopen > 0) {
      unsigned long long best = ~0ull;
      for (int i = lane; i < nopen; i += 64) {
        const unsigned e = open[i];
        const int g = (int)(e >> 12), ex = (int)((e >> 6) & 63u), ey = (int)(e & 63u);
        const int hx = ex - tx, hy = ey - ty;
        const unsigned f = (unsigned)(g + (hx < 0 ? -hx : hx) + (hy < 0 ? -hy : hy));
        // f < 2^13 | g < 2^12 | row, col | slot < 2^12: cells are unique in the list, the slot never decides
        best = guide_min(best, (unsigned long long)f << 36 | (unsigned long long)e << 12 | (unsigned long long)i);
      }
      best = guide_wave_min(best);
      const int slot = (int)(best & 4095u), px = (int)((best >> 18) & 63u), py = (int)((best >> 12) & 63u);
      const int g = (int)((best >> 24) & 4095u);
      if (lane == 0) open[slot] = open[nopen - 1];
      --nopen;
      if (px == tx && py == ty) { found = true; break; }
      GUIDE_WAVE_SYNC();
      bool push = false;
      int x2 = 0, y2 = 0;
      if (lane < 4) {
        x2 = px + (lane == 0 ? -1 : lane == 2 ? 1 : 0);
        y2 = py + (lane == 1 ? -1 : lane == 3 ? 1 : 0);
        push = x2 >= 0 && x2 < Hc && y2 >= 0 && y2 < Wc && !((unavail[x2] >> y2) & 1ull);
      }
      const unsigned long long pm = __ballot(push);
      if (push) {
        const unsigned long long bit = 1ull << y2;
        atomicOr(&unavail[x2], bit);                     // left and right share a row
        if (lane & 1) atomicOr(&par0[x2], bit);
        if (lane & 2) atomicOr(&par1[x2], bit);
        open[nopen + __popcll(pm & ((1ull << lane) - 1ull))] = (unsigned)((g + 1) << 12 | x2 << 6 | y2);
      }
      nopen += __popcll(pm);
      GUIDE_WAVE_SYNC();
    }
  }
  GUIDE_WAVE_SYNC();
  // ---- channel 1: the path cells that fall into the agent's window (LocalG: canvas = window, and the goal marker stays)
  if (lane == 0) {
    const int ox = local ? 0 : cx, oy = local ? 0 : cy;      // window row a = canvas row - ox
    auto mark = [&](int r, int c) {
      const int a = r - ox, q = c - oy;
      if (a >= 0 && a < Wt && q >= 0 && q < Wt) pmask[a] |= 1u << q;
    };
    if (local) mark(grow, gcol);
    if (search) {
      if (found) {
        int ux = tx, uy = ty;
        for (int steps = 0; steps < Hc * Wc && (ux != sx || uy != sy); ++steps) {
          mark(ux, uy);
          const int d = (int)((par0[ux] >> uy) & 1ull) | (int)((par1[ux] >> uy) & 1ull) << 1;
          ux -= d == 0 ? -1 : d == 2 ? 1 : 0;
          uy -= d == 1 ? -1 : d == 3 ? 1 : 0;
        }
      }
      mark(sx, sy);
    }
  }
  GUIDE_WAVE_SYNC();
  // LocalG_S writes channel 2 as zeros (:265-266)
  guide_write_states(x + ag * (long long)(3 * Wt * Wt), fov, wmap, wocc, pmask, !(local && !dyn), lane);
}

}  // namespace

extern "C" int magat_sim_guided_states(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos,
                                       const int32_t* goal, float* x, int FOV, int B, int N, int mode, int dynamic_obstacles,
                                       uint8_t* agent_view, void* stream) {
  if (!map || !pos || !goal || !x) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV <= 0 || !(FOV & 1)) return MAGAT_ERR_BAD_SHAPE;
  if (mode != MAGAT_GUIDE_LOCAL && mode != MAGAT_GUIDE_GLOBAL && mode != MAGAT_GUIDE_SEMI) return MAGAT_ERR_UNSUPPORTED;
  if (FOV < 3 || FOV + 2 > GUIDE_MAX_WT) return MAGAT_ERR_UNSUPPORTED;
  if (mode == MAGAT_GUIDE_SEMI && !agent_view) return MAGAT_ERR_NULL;
  if ((long long)B * N > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  const int half = FOV / 2;
  int Hc = FOV + 2, Wc = FOV + 2;
  if (mode != MAGAT_GUIDE_LOCAL) {
    if (H > GUIDE_MAX_CANVAS - 2 * half - 2 || W > GUIDE_MAX_CANVAS - 2 * half - 2) return MAGAT_ERR_UNSUPPORTED;
    Hc = H + 2 * half + 2;
    Wc = W + 2 * half + 2;
  }
  const size_t lds = GUIDE_LDS_HEAD + (size_t)Hc * Wc * sizeof(unsigned);      // <= 1920 + 16384 bytes
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_GUIDED);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_GUIDED, st);
  hipLaunchKernelGGL(guided_states_kernel<false>, dim3((unsigned)((long long)B * N)), dim3(64), lds, st, map,
                     map_batched ? (long long)H * W : 0LL, H, W, pos, goal, x, FOV, N, mode, dynamic_obstacles ? 1 : 0,
                     mode == MAGAT_GUIDE_SEMI ? agent_view : nullptr, GuideHistory{});
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_sim_replayed_states(const uint8_t* map, int map_batched, int H, int W, const int32_t* pos,
                                         const int32_t* goal, float* x, int FOV, int B, int N,
                                         const magat_sim_history_desc* history, void* stream) {
  if (!map || !pos || !goal || !x) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || FOV <= 0 || !(FOV & 1)) return MAGAT_ERR_BAD_SHAPE;
  if (FOV < 3 || FOV + 2 > GUIDE_MAX_WT) return MAGAT_ERR_UNSUPPORTED;
  if ((long long)B * N > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  const int half = FOV / 2;
  if (H > GUIDE_MAX_CANVAS - 2 * half - 2 || W > GUIDE_MAX_CANVAS - 2 * half - 2) return MAGAT_ERR_UNSUPPORTED;
  GuideHistory hist;
  const int rc = guide_history_check(history, hist);
  if (rc != MAGAT_OK) return rc;
  const int Hc = H + 2 * half + 2, Wc = W + 2 * half + 2;
  const size_t lds = GUIDE_LDS_HEAD + (size_t)Hc * Wc * sizeof(unsigned);
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_REPLAY);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_GUIDED, st);
  hipLaunchKernelGGL(guided_states_kernel<true>, dim3((unsigned)((long long)B * N)), dim3(64), lds, st, map,
                     map_batched ? (long long)H * W : 0LL, H, W, pos, goal, x, FOV, N, MAGAT_GUIDE_SEMI, 1, nullptr, hist);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
