// Expert schedules -> imitation samples on the device: the integer / float64 part of the reference's data transformer
// (onlineExpert/DataTransformer_local_onlineExpert.py: obtainSchedule :181-223, computeAdjacencyMatrix :291-353) and of
// multiRobotSimNew.getPathTarget (utils/new_simulator.py:226-277), for C cases at once.
//   magat_sim_expert_schedule   padded per-agent paths -> positions, one-hot action targets, step validity, bad-move report
//                               (one thread per (case, step, agent))
//   magat_sim_expert_radius     the transformer's carried radius: R, R * 1.1, ... until EVERY step of a case is connected
//                               (one workgroup per (case, step) finds that step's count, one thread per case takes the
//                                maximum and repeats the multiplications)
//   magat_sim_expert_stats      first move, arrival step, makespan, flowtime and the expert's positions from the targets
//                               (one wavefront per case, lanes over agents, the scan over steps is sequential)
//   magat_sim_expert_pick       the expert memory's gather: sample numbers -> (case, step), positions, targets, actions, goals,
//                               radii and maps of a minibatch, decoded from the stored schedules (sim_expert_pick.h: one thread
//                               per (sample, agent))
// State tensors and GSOs of the samples come from the existing kernels (sim_frontend.hip, sim_guidance.hip) on the decoded
// positions.  Every output is written by per-thread (vector) stores.
#include <cstdint>

#include "magat_common.h"
#include "sim_connect.h"
#include "sim_expert_pick.h"

namespace {

constexpr int EXPERT_THREADS = 256;
// expert_radius_step_kernel's static LDS words, behind its 3 N dynamic ints; the launcher's bound counts sizeof of this
struct ExpertRadiusFlags {
  int changed, count;
  long long bound;
};
constexpr size_t EXPERT_RADIUS_STATIC_LDS = sizeof(ExpertRadiusFlags);

__global__ __launch_bounds__(EXPERT_THREADS) void expert_schedule_kernel(const int* __restrict__ paths, const int* __restrict__ lengths,
                                                                         const int* __restrict__ goal, const int* __restrict__ makespan,
                                                                         int* __restrict__ pos, float* __restrict__ target,
                                                                         uint8_t* __restrict__ valid, unsigned* __restrict__ bad,
                                                                         int C, int N, int Lmax, int T) {
  const long long idx = (long long)blockIdx.x * EXPERT_THREADS + threadIdx.x;      // (c * T + t) * N + n
  if (idx >= (long long)C * T * N) return;
  const int n = (int)(idx % N);
  const long long ct = idx / N;
  const int t = (int)(ct % T), c = (int)(ct / T);
  const int Tc = makespan[c] + 1;
  const bool live = t < Tc;
  int cx = 0, cy = 0, key = -1;
  if (live) {
    const long long a = (long long)c * N + n;
    int L = lengths[a];
    L = L < 0 ? 0 : (L > Lmax ? Lmax : L);                         // never read behind the padding
    const int* p = paths + a * (long long)Lmax * 2;
    const int gx = goal[2 * a], gy = goal[2 * a + 1];
    int nx = gx, ny = gy;
    cx = gx;
    cy = gy;
    if (t < L) { cx = p[2 * t]; cy = p[2 * t + 1]; }
    if (t < L - 1) { nx = p[2 * t + 2]; ny = p[2 * t + 3]; }
    const int dx = nx - cx, dy = ny - cy;
    // delta.index([dx, dy]): up, left, down, right, stop (:45-49, :216)
    key = (dx == -1 && dy == 0) ? 0 : (dx == 0 && dy == -1) ? 1 : (dx == 1 && dy == 0) ? 2 : (dx == 0 && dy == 1) ? 3
          : (dx == 0 && dy == 0) ? 4 : -1;
    if (key < 0) atomicMin(&bad[c], (unsigned)t * (unsigned)N + (unsigned)n);      // C * T * N < 2^31 (checked by the launcher)
  }
  pos[2 * idx] = cx;
  pos[2 * idx + 1] = cy;
  float* row = target + idx * 5;
  for (int q = 0; q < 5; ++q) row[q] = q == key ? 1.f : 0.f;
  if (n == 0) valid[ct] = live ? 1 : 0;
}

// k_t of one (case, step): the smallest k with the graph (distance < R * 1.1^k, the product taken k times in sequence)
// connected.  Connectivity is monotone in the threshold, so the reference's carried threshold ends at max_t k_t.
__global__ __launch_bounds__(EXPERT_THREADS) void expert_radius_step_kernel(const int* __restrict__ pos, const uint8_t* __restrict__ valid,
                                                                            double R0, int* __restrict__ step_grow, int N,
                                                                            int max_steps) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;      // b = c * T + step
  if (!valid[b]) {                                                  // block-uniform
    if (t == 0) step_grow[b] = 0;
    return;
  }
  int* px = reinterpret_cast<int*>(smem_raw);
  int* py = px + N;
  int* seen = py + N;
  __shared__ ExpertRadiusFlags f;
  for (int n = t; n < N; n += nt) {
    px[n] = pos[((long long)b * N + n) * 2 + 0];
    py[n] = pos[((long long)b * N + n) * 2 + 1];
  }
  // thread 0 turns each candidate radius into its integer bound (a float64 sqrt loop) once and the others read it behind a
  // barrier; it is replaced only behind sim_graph_connected's closing barrier, when every thread holds its copy
  double r = R0;
  int k = 0;
  bool connected = false;
  while (true) {
    if (t == 0) f.bound = sim_dist2_bound(r);
    __syncthreads();
    const long long d2_bound = f.bound;
    connected = sim_graph_connected(px, py, seen, &f.changed, &f.count, N, d2_bound, t, nt);
    if (connected || k >= max_steps) break;                         // block-uniform
    r = r * 1.1;
    ++k;
  }
  if (t == 0) step_grow[b] = connected ? k : -1;
}

__global__ __launch_bounds__(64) void expert_radius_case_kernel(const int* __restrict__ step_grow, double R0,
                                                                double* __restrict__ radii, int* __restrict__ grow_steps, int C,
                                                                int T, int max_steps) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  int k = 0;
  bool failed = false;
  for (int t = 0; t < T; ++t) {
    const int kt = step_grow[(long long)c * T + t];
    failed |= kt < 0;
    k = kt > k ? kt : k;
  }
  if (failed) k = max_steps;
  double r = R0;
  for (int i = 0; i < k; ++i) r = r * 1.1;      // threshold = threshold * 1.1, k times (:320)
  radii[c] = r;
  grow_steps[c] = failed ? -1 : k;
}

__global__ __launch_bounds__(64) void expert_stats_kernel(const float* __restrict__ target, const int* __restrict__ start,
                                                          const int* __restrict__ goal, const uint8_t* __restrict__ valid,
                                                          int* __restrict__ first_move, int* __restrict__ end_step,
                                                          int* __restrict__ makespan_out, int* __restrict__ flowtime_out,
                                                          int* __restrict__ epos, int T, int N) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int DX[5] = {-1, 0, 1, 0, 0}, DY[5] = {0, -1, 0, 1, 0};      // up, left, down, right, stop (new_simulator.py:56-65)
  int flow = 0, emax = -2147483647 - 1, fmin = 2147483647;
  for (int n = lane; n < N; n += 64) {
    const long long a = (long long)c * N + n;
    int x = start[2 * a], y = start[2 * a + 1];
    const int gx = goal[2 * a], gy = goal[2 * a + 1];
    int fm = 0, es = 0;
    int* ep = epos + ((long long)c * (T + 1) * N + n) * 2;
    ep[0] = x;
    ep[1] = y;
    for (int t = 0; t < T; ++t) {
      if (valid[(long long)c * T + t]) {
        const float* row = target + (((long long)c * T + t) * N + n) * 5;
        int key = 0;                                   // np.argmax: the first maximum
        float best = row[0];
        for (int q = 1; q < 5; ++q)
          if (row[q] > best) { best = row[q]; key = q; }
        if (key != 4 && fm == 0) fm = t + 1;           // (:253-254; "== 0" cannot tell "never" from "not yet" - reproduced)
        x += DX[key];
        y += DY[key];
        if (x == gx && y == gy && es == 0) es = t + 1; // (:259-263)
      }
      ep[(long long)(t + 1) * N * 2] = x;
      ep[(long long)(t + 1) * N * 2 + 1] = y;
    }
    first_move[a] = fm;
    end_step[a] = es;
    flow += es - fm + 1;
    emax = es > emax ? es : emax;
    fmin = fm < fmin ? fm : fmin;
  }
  for (int o = 32; o > 0; o >>= 1) {
    flow += __shfl_xor(flow, o, 64);
    const int e2 = __shfl_xor(emax, o, 64), f2 = __shfl_xor(fmin, o, 64);
    emax = e2 > emax ? e2 : emax;
    fmin = f2 < fmin ? f2 : fmin;
  }
  if (lane == 0) {
    flowtime_out[c] = flow;
    makespan_out[c] = emax - fmin + 1;
  }
}

}  // namespace

extern "C" int magat_sim_expert_schedule(const int32_t* paths, const int32_t* lengths, const int32_t* goal,
                                         const int32_t* makespan, int32_t* pos, float* target, uint8_t* valid, int32_t* bad,
                                         int C, int N, int Lmax, int T, void* stream) {
  if (!paths || !lengths || !goal || !makespan || !pos || !target || !valid || !bad) return MAGAT_ERR_NULL;
  if (C <= 0 || N <= 0 || Lmax <= 0 || T <= 0) return MAGAT_ERR_BAD_SHAPE;
  const long long items = (long long)C * T * N;
  if (items > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_EXPERT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_EXPERT, st);
  if (hipMemsetAsync(bad, 0xff, (size_t)C * sizeof(int32_t), st) != hipSuccess) return MAGAT_ERR_LAUNCH;      // -1: no bad move
  hipLaunchKernelGGL(expert_schedule_kernel, dim3((unsigned)((items + EXPERT_THREADS - 1) / EXPERT_THREADS)), dim3(EXPERT_THREADS),
                     0, st, paths, lengths, goal, makespan, pos, target, valid, reinterpret_cast<unsigned*>(bad), C, N, Lmax, T);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_sim_expert_radius(const int32_t* pos, const uint8_t* valid, double comm_radius, int32_t* step_grow,
                                       double* radii, int32_t* grow_steps, int C, int T, int N, int max_steps, void* stream) {
  if (!pos || !valid || !step_grow || !radii || !grow_steps) return MAGAT_ERR_NULL;
  if (C <= 0 || T <= 0 || N <= 0 || !(comm_radius > 0.0) || max_steps <= 0) return MAGAT_ERR_BAD_SHAPE;
  if ((long long)C * T > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  const size_t lds = (size_t)3 * N * sizeof(int);
  if (lds + EXPERT_RADIUS_STATIC_LDS > 64 * 1024) return MAGAT_ERR_UNSUPPORTED;      // N <= 5460
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_EXPERT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_EXPERT, st);
  hipLaunchKernelGGL(expert_radius_step_kernel, dim3((unsigned)((long long)C * T)), dim3(EXPERT_THREADS), lds, st, pos, valid,
                     comm_radius, step_grow, N, max_steps);
  hipLaunchKernelGGL(expert_radius_case_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, step_grow, comm_radius, radii,
                     grow_steps, C, T, max_steps);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_sim_expert_stats(const float* target, const int32_t* start, const int32_t* goal, const uint8_t* valid,
                                      int32_t* expert_first_move, int32_t* expert_end_step, int32_t* makespan_target,
                                      int32_t* flowtime_target, int32_t* expert_pos, int C, int T, int N, void* stream) {
  if (!target || !start || !goal || !valid || !expert_first_move || !expert_end_step || !makespan_target || !flowtime_target ||
      !expert_pos)
    return MAGAT_ERR_NULL;
  if (C <= 0 || T <= 0 || N <= 0) return MAGAT_ERR_BAD_SHAPE;
  if ((long long)C * (T + 1) * N > 0x3fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_EXPERT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_EXPERT, st);
  hipLaunchKernelGGL(expert_stats_kernel, dim3((unsigned)C), dim3(64), 0, st, target, start, goal, valid, expert_first_move,
                     expert_end_step, makespan_target, flowtime_target, expert_pos, T, N);
  magat_prof_end(pid, st);
  return magat_check_launch();
}

extern "C" int magat_sim_expert_pick(const uint16_t* cells, const int32_t* lengths, const int32_t* goal, const int32_t* makespan,
                                     const double* radii, const int64_t* cum, const uint8_t* maps, const int64_t* indices,
                                     int32_t* case_out, int32_t* step_out, int32_t* pos, float* target, int64_t* action,
                                     int32_t* goal_out, double* radii_out, uint8_t* map_out, int32_t* flag, int count, int N, int Lcap,
                                     int H, int W, int M, void* stream) {
  if (!cells || !lengths || !goal || !makespan || !radii || !cum || !indices || !case_out || !step_out || !pos || !target || !action ||
      !goal_out || !radii_out || !flag)
    return MAGAT_ERR_NULL;
  if (count <= 0 || N <= 0 || Lcap <= 0 || H <= 0 || W <= 0 || M <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > 256 || W > 256) return MAGAT_ERR_UNSUPPORTED;            // a cell is row << 8 | col
  const long long items = (long long)M * N, HW = (long long)H * W;
  if (items > 0x7fffffffLL || (long long)M * HW > 0x7fffffffLL) return MAGAT_ERR_UNSUPPORTED;
  if ((maps == nullptr) != (map_out == nullptr)) return MAGAT_ERR_UNSUPPORTED;
  ExpertPickArgs a;
  a.cells = cells; a.lengths = lengths; a.goal = goal; a.makespan = makespan; a.radii = radii;
  a.cum = reinterpret_cast<const long long*>(cum); a.maps = maps; a.indices = reinterpret_cast<const long long*>(indices);
  a.case_out = case_out; a.step_out = step_out; a.pos = pos; a.target = target; a.action = reinterpret_cast<long long*>(action);
  a.goal_out = goal_out; a.radii_out = radii_out; a.map_out = map_out; a.flag = flag;
  a.count = count; a.N = N; a.Lcap = Lcap; a.HW = (int)HW; a.M = M;
  a.map_words = maps && HW % 4 == 0 && (reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(map_out)) % 4 == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  magat_form_note(MAGAT_FORM_SIM_EXPERT);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_EXPERT, st);
  hipLaunchKernelGGL(expert_pick_kernel, dim3((unsigned)((items + EXPERT_PICK_THREADS - 1) / EXPERT_PICK_THREADS)), dim3(EXPERT_PICK_THREADS),
                     0, st, a);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
