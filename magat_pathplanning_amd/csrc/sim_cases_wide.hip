// The wide form of the case generator of sim_cases.hip: the same cases, cell for cell and draw for draw (restated
// in tests/cases_restatement.py), on maps up to 256 x 256.
//   magat_sim_cases_generate_wide   one workgroup per case, one launch for C cases
// One workgroup of 64 * ceil(H / 64) threads per case, thread = map row, 1, 2 or 4 words per row in registers (row_board.h:
// wide boards); what crosses the wavefronts goes through LDS, one __syncthreads per round.
//   raw map      maze: the aisle walk is sequential, so the first wavefront runs it alone on a bitmap in LDS (256 x 256 bits =
//                8 KB), then every thread takes its row; uniform: thread r draws its W cells; given: one ballot per row and word.
//   fill         seed at the lowest remaining free cell; flood = exact fill inside each row (row_fill of sim_cases.hip as a
//                multi-word add: the carry runs across the words of the row, upwards and, on the reversed row, downwards) + one
//                step up and down, until a round changes nothing; keep the largest, the first on ties.  One barrier per round:
//                it carries the boundary rows and the "something changed" votes; one per component for the three counts.
//   draws        the k-th cell of a board = prefix sum of the row popcounts, per wave by DPP, the wave totals through LDS (one
//                barrier per draw); the thread that owns the row finds the word and the bit, keeps the cell in LDS (row << 8 |
//                col, 16 bits at 256 too) and takes it off its row.  A goal round is drawn to its end and voted on once.
// Every store is a per-lane (vector) store from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "cases_draw.h"

namespace {

constexpr int WCASES_MAX_N = 4096;      // starts and goals wait in LDS: 2 x 8 KB

template <int NW>
__device__ __forceinline__ wboard<NW> wide_row_fill(const wboard<NW>& f, const wboard<NW>& open) {
  const wboard<NW> up = (open ^ wb_add(open, f)) & open;
  const wboard<NW> fr = wb_reverse(f), openr = wb_reverse(open);
  const wboard<NW> down = wb_reverse((openr ^ wb_add(openr, fr)) & openr);
  return f | up | down;
}

// The k-th cell (0-based, row-major) of a board that holds more than k cells: row << 8 | col on the thread that owns its row,
// -1 on every other thread.  One round of the mail.
template <int NW>
__device__ __forceinline__ int wide_select(wide_seat& s, const wboard<NW>& board, int k, int tid) {
  const int cnt = wb_count(board);
  int incl = wave_scan_int(cnt, s.lane);
  wide_post(s, 0, __builtin_amdgcn_readlane(incl, 63));
  incl += wide_sum_before(s, wide_sync(s), 0);
  if (incl <= k || incl - cnt > k) return -1;
  int kk = k - (incl - cnt), col0 = 0;
  u64 word = 0ull;
  bool found = false;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const int c = __popcll(board.w[j]);
    if (!found && kk < c) {
      word = board.w[j];
      col0 = 64 * j;
      found = true;
    }
    if (!found) kk -= c;
  }
  int pos = 0;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    const int c = __popcll((word >> pos) & ((1ull << sh) - 1ull));
    if (kk >= c) {
      kk -= c;
      pos += sh;
    }
  }
  return tid << 8 | (col0 + (pos & 63));
}

// mapGen of the reference as maze_board of sim_cases.hip walks it, by one wavefront on a bitmap in LDS (row y = NW words);
// lane 0 sets the cells, every lane reads them back (one wave: its LDS accesses stay in order).
template <int NW>
__device__ void wide_maze(u64* bitmap, u64 key, int H, int W, int aisles, int walk, int lane) {
  for (int i = 0; i < aisles; ++i) {
    int x = 2 * below(draw32(key, STREAM_AISLE_X, (u64)i), W / 2), y = 2 * below(draw32(key, STREAM_AISLE_Y, (u64)i), H / 2);
    if (lane == 0) bitmap[y * NW + (x >> 6)] |= 1ull << (x & 63);
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
      if (has_bit(bitmap[py * NW + (px >> 6)], px & 63)) continue;
      if (lane == 0) {
        bitmap[py * NW + (px >> 6)] |= 1ull << (px & 63);
        const int mx = (x + px) / 2, my = (y + py) / 2;
        bitmap[my * NW + (mx >> 6)] |= 1ull << (mx & 63);
      }
      x = px;
      y = py;
    }
  }
}

template <int NW>
__global__ __launch_bounds__(WIDE_SIDE) void wcases_kernel(int kind, const uint8_t* __restrict__ map_in, long long map_stride, int H,
                                                           int W, int aisles, int walk, u64 threshold, u64 seed, u64 first_case,
                                                           uint8_t* __restrict__ map_out, int* __restrict__ start,
                                                           int* __restrict__ goal, int* __restrict__ free_cells,
                                                           uint8_t* __restrict__ valid, int N) {
  __shared__ wide_mail mail;
  __shared__ u64 rows[WIDE_SIDE * NW];      // the maze walk's bitmap, then the output board
  __shared__ unsigned short scell[WCASES_MAX_N], gcell[WCASES_MAX_N];
  const int cs = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  wide_seat s{&mail, tid & 63, tid >> 6, nt >> 6, 0};
  const u64 key = mix64(seed + CASES_M * (first_case + (u64)cs + 1ull));
  const wboard<NW> inside = tid < H ? wb_columns<NW>(W) : wb_zero<NW>();      // rows >= H and bits >= W are off the map
  // (a) the raw obstacles
  wboard<NW> obst = wb_zero<NW>();
  if (kind == MAGAT_CASES_GIVEN) {
    const uint8_t* mp = map_in + cs * map_stride;
    for (int r = 64 * s.wave; r < H && r < 64 * s.wave + 64; ++r) {
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        const int col = 64 * k + s.lane;
        const u64 word = __builtin_amdgcn_ballot_w64(col < W && mp[r * W + (col < W ? col : 0)] != 0);
        if (tid == r) obst.w[k] = word;
      }
    }
  } else if (kind == MAGAT_CASES_UNIFORM) {
    if (tid < H) {
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        u64 word = 0ull;
        for (int b = 0; b < 64 && 64 * k + b < W; ++b)
          word |= (u64)((u64)draw32(key, STREAM_CELL, (u64)(tid * W + 64 * k + b)) < threshold) << b;
        obst.w[k] = word;
      }
    }
  } else {
    for (int i = tid; i < nt * NW; i += nt) rows[i] = 0ull;
    __syncthreads();
    if (s.wave == 0) wide_maze<NW>(rows, key, H, W, aisles, walk, s.lane);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NW; ++k) obst.w[k] = rows[tid * NW + k];
    __syncthreads();      // `rows` is written again in (d)
  }
  // (b) the largest 4-connected free component; ties: the one found first, which holds the lowest cell
  wboard<NW> remaining = ~obst & inside, kept = wb_zero<NW>();
  int F = 0;
  // the cells that remain, and the first row that holds one
  u64 has = __builtin_amdgcn_ballot_w64(wb_any(remaining));
  wide_post(s, 0, wave_sum_int(wb_count(remaining)));
  wide_post(s, 1, has ? 64 * s.wave + (int)__builtin_ctzll(has) : WIDE_SIDE);
  int p = wide_sync(s);
  int left = wide_sum(s, p, 0), r0 = wide_min(s, p, 1);
  while (left > F) {      // what is left can still beat the best (covers: nothing left)
    wboard<NW> f = wb_zero<NW>();
    if (tid == r0) {      // the lowest bit of the row
      bool done = false;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        if (!done && remaining.w[k]) {
          f.w[k] = remaining.w[k] & (0ull - remaining.w[k]);
          done = true;
        }
      }
    }
    // A round: fill the rows, then one step up and down.  It votes on what the row fill changed and on what the vertical
    // step of the round before did; when neither did anything, the round before ended on the fixed point.
    bool grew = true;
    for (;;) {
      const wboard<NW> g = wide_row_fill(f, remaining);
      wide_post_rows(s, g, g);
      wide_post(s, 0, (int)wave_any(grew || wb_any(g ^ f)));
      p = wide_sync(s);
      if (!wide_or(s, p, 0)) break;
      f = g | ((wide_cells_up(s, p, g) | wide_cells_down(s, p, g)) & remaining);
      grew = wb_any(f ^ g);
    }
    remaining = remaining & ~f;
    has = __builtin_amdgcn_ballot_w64(wb_any(remaining));
    wide_post(s, 0, wave_sum_int(wb_count(remaining)));
    wide_post(s, 1, has ? 64 * s.wave + (int)__builtin_ctzll(has) : WIDE_SIDE);
    wide_post(s, 2, wave_sum_int(wb_count(f)));
    p = wide_sync(s);
    left = wide_sum(s, p, 0);
    r0 = wide_min(s, p, 1);
    const int n = wide_sum(s, p, 2);
    if (n > F) {
      F = n;
      kept = f;
    }
  }
  // (c) starts: ordered distinct cells of the kept region; goals: the same, in rounds, until no agent's goal is its start
  bool ok = F >= N + 1;
  if (ok) {
    wboard<NW> avail = kept;
    for (int a = 0; a < N; ++a) {
      const int cell = wide_select(s, avail, below(draw32(key, STREAM_START, (u64)a), F - a), tid);
      if (cell >= 0) {
        scell[a] = (unsigned short)cell;
        avail = avail & ~wb_bit<NW>(cell & 255);
      }
    }
    __syncthreads();
    ok = false;
    for (int round = 0; round < CASES_ROUNDS && !ok; ++round) {
      avail = kept;
      bool clash = false;      // a goal on its agent's start: the whole tuple is drawn again
      for (int a = 0; a < N; ++a) {
        const int cell = wide_select(s, avail, below(draw32(key, STREAM_GOAL, (u64)round * (u64)N + (u64)a), F - a), tid);
        if (cell >= 0) {
          clash = clash || cell == (int)scell[a];
          gcell[a] = (unsigned short)cell;
          avail = avail & ~wb_bit<NW>(cell & 255);
        }
      }
      wide_post(s, 0, (int)wave_any(clash));
      ok = !wide_or(s, wide_sync(s), 0);
    }
  }
  // (d) write out: the map threads over cells, the agents threads over a
  const wboard<NW> closed = ~kept & inside;
#pragma unroll
  for (int k = 0; k < NW; ++k) rows[tid * NW + k] = closed.w[k];
  __syncthreads();
  uint8_t* mo = map_out + (long long)cs * H * W;
  for (int i = tid; i < H * W; i += nt) {
    const int r = i / W, c = i - r * W;
    mo[i] = (uint8_t)((rows[r * NW + (c >> 6)] >> (c & 63)) & 1ull);
  }
  const long long a0 = (long long)cs * N;
  for (int a = tid; a < N; a += nt) {
    const int sc = ok ? (int)scell[a] : -1, gc = ok ? (int)gcell[a] : -1;
    start[(a0 + a) * 2] = ok ? sc >> 8 : -1;
    start[(a0 + a) * 2 + 1] = ok ? sc & 255 : -1;
    goal[(a0 + a) * 2] = ok ? gc >> 8 : -1;
    goal[(a0 + a) * 2 + 1] = ok ? gc & 255 : -1;
  }
  if (tid == 0) {
    free_cells[cs] = F;
    valid[cs] = ok ? 1 : 0;
  }
}

}  // namespace

extern "C" int magat_sim_cases_generate_wide(int kind, const uint8_t* map_in, int map_batched, int H, int W, int aisles, int walk,
                                             uint64_t threshold, uint64_t seed, int64_t first_case, uint8_t* map_out, int32_t* start,
                                             int32_t* goal, int32_t* free_cells, uint8_t* valid, int C, int N, void* stream) {
  if (!map_out || !start || !goal || !free_cells || !valid || (kind == MAGAT_CASES_GIVEN && !map_in)) return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || aisles < 0 || walk < 0) return MAGAT_ERR_BAD_SHAPE;
  if (kind != MAGAT_CASES_MAZE && kind != MAGAT_CASES_UNIFORM && kind != MAGAT_CASES_GIVEN) return MAGAT_ERR_BAD_SHAPE;
  if (H > WIDE_SIDE || W > WIDE_SIDE || N > WCASES_MAX_N || N > H * W) return MAGAT_ERR_UNSUPPORTED;
  if (kind == MAGAT_CASES_MAZE && (H < 4 || W < 4 || aisles > CASES_MAX_AISLES || walk > CASES_MAX_WALK)) return MAGAT_ERR_UNSUPPORTED;
  if (first_case < 0 || first_case > (1ll << 32) - C) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)C), block((unsigned)(64 * ((H + 63) / 64)));
  const long long map_stride = map_batched ? (long long)H * W : 0LL;
  magat_form_note(MAGAT_FORM_SIM_MAPF);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF, st);
  if (W <= 64)
    hipLaunchKernelGGL(wcases_kernel<1>, grid, block, 0, st, kind, map_in, map_stride, H, W, aisles, walk, (u64)threshold, (u64)seed,
                       (u64)first_case, map_out, start, goal, free_cells, valid, N);
  else if (W <= 128)
    hipLaunchKernelGGL(wcases_kernel<2>, grid, block, 0, st, kind, map_in, map_stride, H, W, aisles, walk, (u64)threshold, (u64)seed,
                       (u64)first_case, map_out, start, goal, free_cells, valid, N);
  else
    hipLaunchKernelGGL(wcases_kernel<4>, grid, block, 0, st, kind, map_in, map_stride, H, W, aisles, walk, (u64)threshold, (u64)seed,
                       (u64)first_case, map_out, start, goal, free_cells, valid, N);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
