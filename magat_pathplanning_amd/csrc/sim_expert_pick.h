// The expert memory's gather (magat_sim_expert_pick, sim_expert.hip): sample numbers -> the rows of a minibatch, decoded from
// the stored schedules.  The kernel stands in a header of its own so that tools/host_wave/expert_pick_check.cpp can compile
// exactly this text for the host.  One thread per (sample, agent); the N threads of a sample share the copy of its map.
#pragma once
#include <cstdint>

namespace {

constexpr int EXPERT_PICK_THREADS = 256;

struct ExpertPickArgs {
  const uint16_t* cells;       // (count, N, Lcap): row << 8 | col, padded behind lengths with the path's last cell
  const int* lengths;          // (count, N)
  const int* goal;             // (count, N, 2)
  const int* makespan;         // (count,)
  const double* radii;         // (count,)
  const long long* cum;        // (count,): inclusive prefix sums of makespan + 1
  const uint8_t* maps;         // (count, H, W), or null: one shared map, nothing is copied
  const long long* indices;    // (M,)
  int* case_out;               // (M,)
  int* step_out;               // (M,)
  int* pos;                    // (M, N, 2)
  float* target;               // (M, N, 5)
  long long* action;           // (M, N)
  int* goal_out;               // (M, N, 2)
  double* radii_out;           // (M,)
  uint8_t* map_out;            // (M, H, W), or null with maps
  int* flag;                   // (1,): the smallest row whose index was out of range, over all calls
  int count, N, Lcap, HW, M;
  int map_words;               // 1: HW % 4 == 0 and both map pointers are 4-byte aligned - the copy moves 32-bit words
};

__global__ __launch_bounds__(EXPERT_PICK_THREADS) void expert_pick_kernel(ExpertPickArgs a) {
  const long long idx = (long long)blockIdx.x * EXPERT_PICK_THREADS + threadIdx.x;      // m * N + n
  if (idx >= (long long)a.M * a.N) return;
  const int n = (int)(idx % a.N), m = (int)(idx / a.N);
  // sample -> (case, step): the first case whose inclusive prefix sum is above j
  const long long total = a.cum[a.count - 1];
  long long j = a.indices[m];
  if (j < 0 || j >= total) {
    if (n == 0) atomicMin(a.flag, m);
    j = j < 0 || total <= 0 ? 0 : total - 1;      // clamped: the row is a real sample, no later kernel sees made-up positions
  }
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {                                // log2(count) steps: 20 for a store of a million cases
    const int mid = (lo + hi) >> 1;
    if (a.cum[mid] > j) hi = mid; else lo = mid + 1;
  }
  const int c = lo;
  const int last = a.makespan[c] < 0 ? 0 : a.makespan[c];
  long long tl = j - (c ? a.cum[c - 1] : 0);
  tl = tl < 0 ? 0 : (tl > last ? last : tl);       // (a consistent store never needs this)
  const int t = (int)tl;
  // expert_schedule_kernel's rule on the packed cells
  const long long ag = (long long)c * a.N + n;
  int L = a.lengths[ag];
  L = L < 0 ? 0 : (L > a.Lcap ? a.Lcap : L);      // never read behind the row
  const uint16_t* p = a.cells + ag * a.Lcap;
  const int gx = a.goal[2 * ag], gy = a.goal[2 * ag + 1];
  int cx = gx, cy = gy, nx = gx, ny = gy;
  if (t < L) { cx = p[t] >> 8; cy = p[t] & 255; }
  if (t < L - 1) { nx = p[t + 1] >> 8; ny = p[t + 1] & 255; }
  const int dx = nx - cx, dy = ny - cy;
  const int key = (dx == -1 && dy == 0) ? 0 : (dx == 0 && dy == -1) ? 1 : (dx == 1 && dy == 0) ? 2 : (dx == 0 && dy == 1) ? 3
                  : (dx == 0 && dy == 0) ? 4 : -1;      // up, left, down, right, stop; -1 cannot be stored (append checks)
  a.pos[2 * idx] = cx;
  a.pos[2 * idx + 1] = cy;
  float* row = a.target + idx * 5;
  for (int q = 0; q < 5; ++q) row[q] = q == key ? 1.f : 0.f;
  a.action[idx] = key < 0 ? 0 : key;               // target.argmax(-1): the first maximum of an all-zero row is 0
  a.goal_out[2 * idx] = gx;
  a.goal_out[2 * idx + 1] = gy;
  if (n == 0) {
    a.case_out[m] = c;
    a.step_out[m] = t;
    a.radii_out[m] = a.radii[c];
  }
  if (a.maps) {
    const uint8_t* src = a.maps + (long long)c * a.HW;
    uint8_t* dst = a.map_out + (long long)m * a.HW;
    if (a.map_words) {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
      uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
      for (int i = n; i < a.HW / 4; i += a.N) d4[i] = s4[i];
    } else {
      for (int i = n; i < a.HW; i += a.N) dst[i] = src[i];
    }
  }
}

}  // namespace
