// Planning cases made on the device: an obstacle map, its largest free component, and a start and a goal per agent - the
// head of the expert pipeline, in front of sim_mapf.hip (restated cell by cell in tests/cases_restatement.py).
//   magat_sim_cases_generate   one wavefront per case, one launch for C cases
// One wavefront per case, lane = map row, one 64-bit word per row (row_board.h): the obstacles, a flood front and the cells
// still free to draw from are one register pair each across the wave.
//   raw map      maze: the aisle walk is sequential, so it runs wave-uniform (position in scalars, the board in the lanes);
//                uniform: lane r draws its W cells; given: one ballot per row of the caller's map.
//   fill         seed at the lowest remaining free cell; flood = exact fill inside each row (a carry runs along a stretch of
//                free cells: one add upwards, one on the bit-reversed word downwards) + one step up and down (DPP wave
//                shifts), until nothing changes; keep the largest, the first on ties.
//   draws        the k-th cell of a board = prefix sum of the row popcounts (DPP row scan + three row totals), the row by one
//                ballot, the bit by a binary search over popcounts of that row's word.  Starts and the goals of the current
//                round wait in LDS (row << 8 | col) and are written out lanes over agents.
// Random numbers are a counter-based hash (splitmix64 finaliser) of (seed, global case index, stream, index): a case does
// not depend on the batch it is made in.  Everything is integer and bit arithmetic; every store is a per-lane (vector) store
// from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "cases_draw.h"      // the random stream, its limits, the lane scans

namespace {

constexpr int CASES_SIDE = 64;                    // rows = lanes, columns = bits
constexpr int CASES_MAX_N = CASES_SIDE * CASES_SIDE;
__device__ __forceinline__ u64 lane_word(u64 v, int lane) {      // wave-uniform `lane`
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int board_count(u64 board) { return wave_sum_int(__popcll(board)); }

// every stretch of consecutive `open` bits that holds a bit of f, whole (f is a subset of open).  Upwards: open + f carries
// from each seed to the end of its stretch and clears it, so open ^ (open + f) marks seed .. end (but a second seed of the same
// stretch, which f itself puts back); downwards the same on the reversed words.
__device__ __forceinline__ u64 row_fill(u64 f, u64 open) {
  const u64 up = (open ^ (open + f)) & open;
  const u64 fr = __brevll(f), openr = __brevll(open);
  const u64 down = __brevll((openr ^ (openr + fr)) & openr);
  return f | up | down;
}

// the k-th cell (0-based, row-major) of a board that holds more than k cells, as row << 8 | col.  Wave-uniform.
__device__ __forceinline__ int board_select(u64 board, int k, int lane) {
  const int cnt = __popcll(board);
  const int incl = wave_scan_int(cnt, lane);
  const u64 m = __builtin_amdgcn_ballot_w64(incl > k);
  const int row = __builtin_amdgcn_readfirstlane(m ? (int)__builtin_ctzll(m) : 0);
  int kk = k - __builtin_amdgcn_readlane(incl - cnt, row);
  const u64 word = lane_word(board, row);
  int pos = 0;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int c = __popcll((word >> pos) & ((1ull << s) - 1ull));
    if (kk >= c) {
      kk -= c;
      pos += s;
    }
  }
  return row << 8 | (pos & 63);
}

// mapGen of the reference: `aisles` walks of `walk` steps over the even lattice; a step lists the distance-2 neighbours left,
// right, up, down under the reference's conditions and takes neighbours[below(len - 1)] - never the last one listed.
__device__ u64 maze_board(u64 key, int H, int W, int aisles, int walk, int lane) {
  u64 obst = 0ull;
  for (int i = 0; i < aisles; ++i) {
    int x = 2 * below(draw32(key, STREAM_AISLE_X, (u64)i), W / 2), y = 2 * below(draw32(key, STREAM_AISLE_Y, (u64)i), H / 2);
    if (lane == y) obst |= 1ull << x;
    for (int j = 0; j < walk; ++j) {
      const bool left = x > 1, right = x < W - 2, up = y > 1, down = y < H - 2;
      const int n = (int)left + (int)right + (int)up + (int)down;
      if (n == 0) continue;
      int p = below(draw32(key, STREAM_WALK, (u64)i * (u64)walk + (u64)j), n - 1), px = x, py = y;
      if (left) {
        if (p == 0) px = x - 2;
        --p;
      }
      if (right) {
        if (p == 0) px = x + 2;
        --p;
      }
      if (up) {
        if (p == 0) py = y - 2;
        --p;
      }
      if (down) {
        if (p == 0) py = y + 2;
        --p;
      }
      if (wave_any(lane == py && has_bit(obst, px))) continue;
      if (lane == py) obst |= 1ull << px;
      if (lane == (y + py) / 2) obst |= 1ull << ((x + px) / 2);
      x = px;
      y = py;
    }
  }
  return obst;
}

__global__ __launch_bounds__(64) void cases_kernel(int kind, const uint8_t* __restrict__ map_in, long long map_stride, int H, int W,
                                                   int aisles, int walk, u64 threshold, u64 seed, u64 first_case,
                                                   uint8_t* __restrict__ map_out, int* __restrict__ start, int* __restrict__ goal,
                                                   int* __restrict__ free_cells, uint8_t* __restrict__ valid, int N) {
  __shared__ u64 rows[CASES_SIDE];
  __shared__ unsigned short scell[CASES_MAX_N], gcell[CASES_MAX_N];
  const int cs = blockIdx.x, lane = threadIdx.x;
  const u64 key = mix64(seed + CASES_M * (first_case + (u64)cs + 1ull));
  const u64 inside = lane < H ? (W == 64 ? ~0ull : (1ull << W) - 1ull) : 0ull;      // lanes >= H and bits >= W are off the map
  // (a) the raw obstacles
  u64 obst = 0ull;
  if (kind == MAGAT_CASES_GIVEN) {
    const uint8_t* mp = map_in + cs * map_stride;
    for (int r = 0; r < H; ++r) {
      const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] != 0);
      if (lane == r) obst = word;
    }
  } else if (kind == MAGAT_CASES_UNIFORM) {
    if (lane < H)
      for (int c = 0; c < W; ++c)
        if ((u64)draw32(key, STREAM_CELL, (u64)(lane * W + c)) < threshold) obst |= 1ull << c;
  } else {
    obst = maze_board(key, H, W, aisles, walk, lane);
  }
  // (b) the largest 4-connected free component; ties: the one found first, which holds the lowest cell
  u64 remaining = ~obst & inside, kept = 0ull;
  int F = 0;
  for (;;) {
    if (board_count(remaining) <= F) break;      // what is left cannot beat the best (covers: nothing left)
    const u64 has = __builtin_amdgcn_ballot_w64(remaining != 0ull);
    const int r0 = (int)__builtin_ctzll(has);
    u64 f = lane == r0 ? remaining & (0ull - remaining) : 0ull;
    for (;;) {
      const u64 prev = f;
      f = row_fill(f, remaining);
      f |= (cells_up(f) | cells_down(f)) & remaining;
      if (!wave_any(f != prev)) break;
    }
    const int n = board_count(f);
    if (n > F) {
      F = n;
      kept = f;
    }
    remaining &= ~f;
  }
  // (c) starts: ordered distinct cells of the kept region; goals: the same, in rounds, until no agent's goal is its start
  bool ok = F >= N + 1;
  if (ok) {
    u64 avail = kept;
    for (int a = 0; a < N; ++a) {
      const int cell = board_select(avail, below(draw32(key, STREAM_START, (u64)a), F - a), lane);
      if (lane == 0) scell[a] = (unsigned short)cell;
      if (lane == (cell >> 8)) avail &= ~(1ull << (cell & 63));
    }
    __syncthreads();
    ok = false;
    for (int round = 0; round < CASES_ROUNDS && !ok; ++round) {
      avail = kept;
      ok = true;
      for (int a = 0; a < N; ++a) {
        const int cell = board_select(avail, below(draw32(key, STREAM_GOAL, (u64)round * (u64)N + (u64)a), F - a), lane);
        if (cell == (int)scell[a]) {      // the whole tuple is drawn again
          ok = false;
          break;
        }
        if (lane == 0) gcell[a] = (unsigned short)cell;
        if (lane == (cell >> 8)) avail &= ~(1ull << (cell & 63));
      }
    }
  }
  // (d) write out: the map lanes over cells, the agents lanes over a
  rows[lane] = ~kept & inside;
  __syncthreads();
  uint8_t* mo = map_out + (long long)cs * H * W;
  for (int i = lane; i < H * W; i += 64) {
    const int r = i / W, c = i - r * W;
    mo[i] = (uint8_t)((rows[r] >> c) & 1ull);
  }
  const long long a0 = (long long)cs * N;
  for (int a = lane; a < N; a += 64) {
    const int s = ok ? (int)scell[a] : -1, g = ok ? (int)gcell[a] : -1;
    start[(a0 + a) * 2] = ok ? s >> 8 : -1;
    start[(a0 + a) * 2 + 1] = ok ? s & 255 : -1;
    goal[(a0 + a) * 2] = ok ? g >> 8 : -1;
    goal[(a0 + a) * 2 + 1] = ok ? g & 255 : -1;
  }
  if (lane == 0) {
    free_cells[cs] = F;
    valid[cs] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int magat_sim_cases_generate(int kind, const uint8_t* map_in, int map_batched, int H, int W, int aisles, int walk,
                                        uint64_t threshold, uint64_t seed, int64_t first_case, uint8_t* map_out, int32_t* start,
                                        int32_t* goal, int32_t* free_cells, uint8_t* valid, int C, int N, void* stream) {
  if (!map_out || !start || !goal || !free_cells || !valid || (kind == MAGAT_CASES_GIVEN && !map_in)) return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || aisles < 0 || walk < 0) return MAGAT_ERR_BAD_SHAPE;
  if (kind != MAGAT_CASES_MAZE && kind != MAGAT_CASES_UNIFORM && kind != MAGAT_CASES_GIVEN) return MAGAT_ERR_BAD_SHAPE;
  if (H > CASES_SIDE || W > CASES_SIDE || N > H * W) return MAGAT_ERR_UNSUPPORTED;
  if (kind == MAGAT_CASES_MAZE && (H < 4 || W < 4 || aisles > CASES_MAX_AISLES || walk > CASES_MAX_WALK)) return MAGAT_ERR_UNSUPPORTED;
  if (first_case < 0 || first_case > (1ll << 32) - C) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_MAPF);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF, st);
  hipLaunchKernelGGL(cases_kernel, dim3((unsigned)C), dim3(64), 0, st, kind, map_in, map_batched ? (long long)H * W : 0LL, H, W, aisles,
                     walk, (u64)threshold, (u64)seed, (u64)first_case, map_out, start, goal, free_cells, valid, N);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
