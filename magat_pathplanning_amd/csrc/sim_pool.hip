// The case pool of the closed-loop evaluation (rollout.py: EpisodePool): B slots over a queue of C cases.
// A slot whose episode is over writes its case's result row and takes the next case of the queue, on the device, in the call that
// ends the episode - the reference's validation / test loop (agents/decentralplannerlocal_OnlineExpert_GAT.py:859-957) without a
// batch that waits for its slowest case.
//   magat_sim_pool_step[_wide]   magat_sim_step[_wide] with the step number and the limit per slot (sim_frontend.hip's kernel:
//                                magat_sim_step_slots), `over` and the sticky flag word per slot
//   magat_sim_pool_turn          result rows, trajectories, refill in ascending slot order, step-0 radius of the new cases
//   magat_sim_pool_uniforms      one float64 in [0, 1) per (seed, case, step, agent): a case's draws do not depend on its slot
// The turn is two launches.  The first, one wavefront, counts the finished slots and moves the queue's counters; the second, one
// workgroup per slot, reads what the first left: no workgroup reads a word that another workgroup of its own launch writes.
#include <cstdint>

#include "magat_common.h"
#include "cases_draw.h"
#include "sim_connect.h"

#ifdef MAGAT_HOST_WAVE
#define POOL_DYN_LDS(var) unsigned char* var = reinterpret_cast<unsigned char*>(host_wave::dyn_lds)
#else
#define POOL_DYN_LDS(var) extern __shared__ __align__(16) unsigned char var[]
#endif

namespace {

constexpr int POOL_THREADS = 256;
constexpr int POOL_STREAM_UNIFORM = 16;      // the draws' stream field holds STREAM + step: clear of the case generator's streams
enum { CNT_NEXT = 0, CNT_REMAINING = 1, CNT_BASE = 2 };

// one wavefront: the finished slots of this turn take the cases base, base + 1, ...; next and remaining move on
__global__ __launch_bounds__(64) void pool_count_kernel(const int* __restrict__ over, int* __restrict__ counters, int B, int init) {
  const int lane = threadIdx.x;
  int c = 0;
  for (int j = lane; j < B; j += 64) c += (init || over[j] != 0) ? 1 : 0;
  const int total = wave_sum_int(c);
  if (lane == 0) {
    const int next = counters[CNT_NEXT];
    counters[CNT_BASE] = next;
    counters[CNT_NEXT] = next + total;           // beyond the queue's end once it is drained: the slots then go idle
    if (!init) counters[CNT_REMAINING] -= total;
  }
}

__global__ __launch_bounds__(POOL_THREADS) void pool_turn_kernel(magat_sim_pool_desc d, int init) {
  POOL_DYN_LDS(smem_raw);
  const int b = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
  const int N = d.N, C = d.C, cells = d.H * d.W;
  __shared__ int s_rank, s_reach, changed, count;
  const bool fin = init || d.over[b] != 0;                       // block-uniform
  const int c_old = d.slot_case[b];
  const int step = d.slot_step[b];
  if (!fin) {
    if (c_old < 0) return;                                       // idle
    if (d.record) {
      const int k = step - d.first_step + 1;                     // the cells after the call of `step`
      if (k >= 0 && k < d.traj_cells)
        for (int n = t; n < N; n += nt) {
          const long long a = (long long)b * N + n;
          d.traj[((long long)c_old * N + n) * d.traj_cells + k] = (uint16_t)((d.pos[2 * a] << 8) | (d.pos[2 * a + 1] & 255));
        }
    }
    __syncthreads();                                             // every thread holds `step`
    if (t == 0) d.slot_step[b] = step + 1;
    return;
  }
  // ---- the slot's episode is over: its case's row
  if (t == 0) s_reach = 0;
  __syncthreads();
  if (!init && c_old >= 0) {
    int r = 0;
    for (int n = t; n < N; n += nt) {
      const long long a = (long long)b * N + n, q = (long long)c_old * N + n;
      r += d.reach_goal[a] ? 1 : 0;
      d.r_end_pos[2 * q] = d.pos[2 * a];
      d.r_end_pos[2 * q + 1] = d.pos[2 * a + 1];
      d.r_first_move[q] = d.first_move[a];
      d.r_end_step[q] = d.end_step[a];
    }
    if (r) atomicAdd(&s_reach, r);
  }
  // rank among the finished slots: those with a lower index (wave 0; the other waves wait at the barrier)
  if (t < 64) {
    int c = 0;
    for (int j = t; j < b; j += 64) c += (init || d.over[j] != 0) ? 1 : 0;
    const int rank = wave_sum_int(c);
    if (t == 0) s_rank = rank;
  }
  __syncthreads();
  if (!init && c_old >= 0 && t == 0) {
    const int sticky = d.sticky[b];
    int* row = d.rows + c_old;
    row[(long long)MAGAT_POOL_RETIRED * C] = 1;
    row[(long long)MAGAT_POOL_ALL_REACH * C] = d.done[b];
    row[(long long)MAGAT_POOL_NUM_REACH * C] = s_reach;
    row[(long long)MAGAT_POOL_STEPS * C] = step;
    row[(long long)MAGAT_POOL_MAKESPAN * C] = d.makespan[b];
    row[(long long)MAGAT_POOL_FLOWTIME * C] = d.flowtime[b];
    row[(long long)MAGAT_POOL_PREDICTED * C] = (sticky & 15) ? 1 : 0;
    row[(long long)MAGAT_POOL_FLAG_BITS * C] = sticky;
    if (d.record) d.traj_len[c_old] = step - d.first_step + 1;   // the start and one cell per call that moved
  }
  // ---- refill
  const int c_new = d.counters[CNT_BASE] + s_rank;
  if (c_new >= C) {                                              // the queue is drained: idle, the positions stay
    if (t == 0) d.slot_case[b] = -1;
    return;
  }
  int* px = reinterpret_cast<int*>(smem_raw);
  int* py = px + N;
  int* seen = py + N;
  for (int n = t; n < N; n += nt) {
    const long long a = (long long)b * N + n, q = (long long)c_new * N + n;
    const int x = d.q_start[2 * q], y = d.q_start[2 * q + 1];
    px[n] = x;
    py[n] = y;
    d.pos[2 * a] = x;
    d.pos[2 * a + 1] = y;
    d.goal[2 * a] = d.q_goal[2 * q];
    d.goal[2 * a + 1] = d.q_goal[2 * q + 1];
    d.reach_goal[a] = 0;
    d.first_move[a] = 0;
    d.end_step[a] = 0;
    if (d.record) d.traj[q * d.traj_cells] = (uint16_t)((x << 8) | (y & 255));
  }
  if (d.map_batched)
    for (int i = t; i < cells; i += nt) d.map[(long long)b * cells + i] = d.q_map[(long long)c_new * cells + i];
  if (d.agent_view) {                                            // 'SemiLG_*': nothing seen yet (AgentState.setmap)
    uint8_t* v = d.agent_view + (long long)b * d.agent_view_bytes;
    for (long long i = t; i < d.agent_view_bytes; i += nt) v[i] = 0;
  }
  if (t == 0) {
    d.slot_case[b] = c_new;
    d.slot_step[b] = d.first_step;
    d.slot_maxstep[b] = d.q_maxstep[c_new];
    d.sticky[b] = 0;
  }
  // the new case's step-0 radius: sim_radius_kernel's loop (sim_frontend.hip), the same predicate and the same products
  double r = d.comm_radius / 1.1;
  int steps = 0;
  bool connected = false;
  while (!connected && steps < d.radius_max_steps) {
    r = r * 1.1;
    ++steps;
    connected = sim_graph_connected(px, py, seen, &changed, &count, N, sim_dist2_bound(r), t, nt);
  }
  if (t == 0) {
    d.radii[b] = r;
    d.r_radius[c_new] = r;
    d.rows[(long long)MAGAT_POOL_STATUS * C + c_new] = connected ? 0 : MAGAT_POOL_STATUS_DISCONNECTED;
  }
}

__global__ __launch_bounds__(POOL_THREADS) void pool_uniforms_kernel(const int* __restrict__ slot_case, const int* __restrict__ slot_step,
                                                                     double* __restrict__ u, unsigned long long seed, int B, int N) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * N) return;
  const int b = (int)(idx / N), n = (int)(idx - (long long)b * N);
  const int c = slot_case[b];
  double v = 0.0;
  if (c >= 0) {
    const u64 key = mix64((u64)seed + CASES_M * ((u64)c + 1));
    const int stream = POOL_STREAM_UNIFORM + slot_step[b];
    const u64 hi = draw32(key, stream, 2 * (u64)n), lo = draw32(key, stream, 2 * (u64)n + 1);
    v = (double)((hi << 21) | (lo >> 11)) * 0x1p-53;             // 53 bits: exact, below 1
  }
  u[idx] = v;
}

int pool_step(const magat_sim_step_desc* d, const int32_t* slot_case, const int32_t* slot_step, const int32_t* slot_maxstep,
              int32_t* over, int32_t* sticky, bool wide, void* workspace, size_t workspace_bytes, void* stream) {
  magat_sim_pool_slots s{slot_case, slot_step, slot_maxstep, over, sticky};
  return magat_sim_step_slots(d, &s, stream, wide, workspace, workspace_bytes);
}

}  // namespace

extern "C" int magat_sim_pool_step(const magat_sim_step_desc* d, const int32_t* slot_case, const int32_t* slot_step,
                                   const int32_t* slot_maxstep, int32_t* over, int32_t* sticky, void* stream) {
  return pool_step(d, slot_case, slot_step, slot_maxstep, over, sticky, false, nullptr, 0, stream);
}

extern "C" int magat_sim_pool_step_wide(const magat_sim_step_desc* d, const int32_t* slot_case, const int32_t* slot_step,
                                        const int32_t* slot_maxstep, int32_t* over, int32_t* sticky, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return pool_step(d, slot_case, slot_step, slot_maxstep, over, sticky, true, workspace, workspace_bytes, stream);
}

extern "C" int magat_sim_pool_turn(const magat_sim_pool_desc* d, int init, void* stream) {
  if (!d) return MAGAT_ERR_NULL;
  if (!d->q_map || !d->q_start || !d->q_goal || !d->q_maxstep || !d->slot_case || !d->slot_step || !d->slot_maxstep || !d->over ||
      !d->sticky || !d->pos || !d->goal || !d->reach_goal || !d->first_move || !d->end_step || !d->done || !d->flowtime ||
      !d->makespan || !d->radii || !d->counters || !d->rows || !d->r_radius || !d->r_end_pos || !d->r_first_move || !d->r_end_step)
    return MAGAT_ERR_NULL;
  if ((d->map_batched && !d->map) || (d->record && (!d->traj || !d->traj_len))) return MAGAT_ERR_NULL;
  if (d->B <= 0 || d->C <= 0 || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->B > d->C || !(d->comm_radius > 0.0) ||
      d->radius_max_steps <= 0 || (d->record && d->traj_cells <= 0) || (d->agent_view && d->agent_view_bytes <= 0))
    return MAGAT_ERR_BAD_SHAPE;
  if (d->record && (d->H > 256 || d->W > 256)) return MAGAT_ERR_UNSUPPORTED;      // a cell is row << 8 | col
  const size_t lds = (size_t)3 * d->N * sizeof(int);
  if (lds > 60 * 1024) return MAGAT_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pool_count_kernel, dim3(1), dim3(64), 0, st, d->over, d->counters, d->B, init ? 1 : 0);
  hipLaunchKernelGGL(pool_turn_kernel, dim3(d->B), dim3(POOL_THREADS), lds, st, *d, init ? 1 : 0);
  return magat_check_launch();
}

extern "C" int magat_sim_pool_uniforms(const int32_t* slot_case, const int32_t* slot_step, double* u, uint64_t seed, int B, int N,
                                       void* stream) {
  if (!slot_case || !slot_step || !u) return MAGAT_ERR_NULL;
  if (B <= 0 || N <= 0) return MAGAT_ERR_BAD_SHAPE;
  const long long total = (long long)B * N;
  hipLaunchKernelGGL(pool_uniforms_kernel, dim3((unsigned)((total + POOL_THREADS - 1) / POOL_THREADS)), dim3(POOL_THREADS), 0,
                     static_cast<hipStream_t>(stream), slot_case, slot_step, u, (unsigned long long)seed, B, N);
  return magat_check_launch();
}
