// Runs the case pool's turn and uniforms kernels - magat_sim_pool_turn, magat_sim_pool_uniforms (csrc/sim_pool.hip) - on the host,
// one thread per lane (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/sim_pool_check.cpp -o sim_pool_check
//   sim_pool_check case.txt > result.txt
// The move step is not part of this program (its kernel needs a device): between two turns a stand-in step advances every slot
// that holds a case by a fixed rule - tests/test_host_rollout.py applies the same rule to tests/rollout_restatement.py's pool:
//   t = slot_step, c = slot_case;  over = t >= slot_maxstep;  done = (c + t) % 2;  makespan = 100 + t;  flowtime = 200 + c + t;
//   if not over: sticky |= 1 << (t % 6);  agent n: row = (row + 1) % H;  if (n + t) % 3 == 0: reach = 1, end_step = t if it was 0;
//   if n % 2 == 0 and first_move == 0: first_move = t
// case.txt: whitespace-separated B N H W C first_step record traj_cells max_steps calls seed, the radius (a float), then the maps
// (C H W), start (C N 2), goal (C N 2), maxstep (C).  Out come, one line each: the return code of the first fill; per call the
// uniforms (B N, hex floats), then slot_case, slot_step, slot_maxstep (B each), radii (B, hex), counters (2), pos (B N 2) after
// the turn; at the end rows (9 C), r_radius (C, hex), end_pos (C N 2), first_move, end_step (C N), traj_len (C), traj (C N cells).
#include <cstdio>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
int magat_sim_step_slots(const magat_sim_step_desc*, const magat_sim_pool_slots*, void*, bool, void*, size_t) { return MAGAT_ERR_UNSUPPORTED; }

#include "../../magat_pathplanning_amd/csrc/sim_pool.hip"

template <typename T>
static bool read_all(FILE* f, std::vector<T>& v) {
  for (auto& x : v) {
    long long t;
    if (fscanf(f, "%lld", &t) != 1) return false;
    x = (T)t;
  }
  return true;
}
template <typename T>
static void line(const std::vector<T>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf("%lld%c", (long long)v[i], i + 1 == v.size() ? '\n' : ' ');
  if (v.empty()) printf("\n");
}
static void line_f(const std::vector<double>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf("%a%c", v[i], i + 1 == v.size() ? '\n' : ' ');
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int B, N, H, W, C, first_step, record, traj_cells, max_steps, calls;
  unsigned long long seed;
  double radius;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d %d %llu %lf", &B, &N, &H, &W, &C, &first_step, &record, &traj_cells, &max_steps, &calls,
                   &seed, &radius) != 12)
    return 2;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || traj_cells <= 0 || calls < 0) return 2;
  std::vector<uint8_t> q_map((size_t)C * H * W);
  std::vector<int32_t> q_start((size_t)C * N * 2), q_goal((size_t)C * N * 2), q_maxstep(C);
  if (!read_all(f, q_map) || !read_all(f, q_start) || !read_all(f, q_goal) || !read_all(f, q_maxstep)) return 2;
  fclose(f);
  // every buffer has exactly its documented size
  std::vector<int32_t> slot_case(B, -1), slot_step(B, 0), slot_maxstep(B, 0), over(B, 0), sticky(B, 0), pos((size_t)B * N * 2, 0),
      goal((size_t)B * N * 2, 0), first_move((size_t)B * N, 0), end_step((size_t)B * N, 0), done(B, 0), flowtime(B, 0), makespan(B, 0),
      counters(4, 0), rows((size_t)MAGAT_POOL_COLUMNS * C, 0), r_end_pos((size_t)C * N * 2, 0), r_first_move((size_t)C * N, 0),
      r_end_step((size_t)C * N, 0), traj_len(C, 0);
  std::vector<uint8_t> map((size_t)B * H * W, 0), reach((size_t)B * N, 0);
  std::vector<double> radii(B, 0.0), r_radius(C, 0.0), u((size_t)B * N, -1.0);
  std::vector<uint16_t> traj((size_t)C * N * traj_cells, 0);
  counters[1] = C;
  magat_sim_pool_desc d = {};
  d.q_map = q_map.data(); d.q_start = q_start.data(); d.q_goal = q_goal.data(); d.q_maxstep = q_maxstep.data();
  d.map_batched = 1; d.H = H; d.W = W; d.C = C; d.B = B; d.N = N;
  d.first_step = first_step; d.record = record; d.traj_cells = traj_cells; d.radius_max_steps = max_steps;
  d.comm_radius = radius;
  d.slot_case = slot_case.data(); d.slot_step = slot_step.data(); d.slot_maxstep = slot_maxstep.data();
  d.over = over.data(); d.sticky = sticky.data(); d.map = map.data(); d.pos = pos.data(); d.goal = goal.data();
  d.reach_goal = reach.data(); d.first_move = first_move.data(); d.end_step = end_step.data();
  d.done = done.data(); d.flowtime = flowtime.data(); d.makespan = makespan.data(); d.radii = radii.data();
  d.counters = counters.data(); d.rows = rows.data(); d.r_radius = r_radius.data(); d.r_end_pos = r_end_pos.data();
  d.r_first_move = r_first_move.data(); d.r_end_step = r_end_step.data();
  d.traj = record ? traj.data() : nullptr; d.traj_len = record ? traj_len.data() : nullptr;
  printf("%d\n", magat_sim_pool_turn(&d, 1, nullptr));
  for (int k = 0; k < calls; ++k) {
    if (magat_sim_pool_uniforms(slot_case.data(), slot_step.data(), u.data(), seed, B, N, nullptr) != MAGAT_OK) return 3;
    line_f(u);
    for (int b = 0; b < B; ++b) {                                   // the stand-in step
      over[b] = 0;
      const int c = slot_case[b], t = slot_step[b];
      if (c < 0) continue;
      over[b] = t >= slot_maxstep[b] ? 1 : 0;
      done[b] = (c + t) % 2;
      makespan[b] = 100 + t;
      flowtime[b] = 200 + c + t;
      if (over[b]) continue;
      sticky[b] |= 1 << (t % 6);
      for (int n = 0; n < N; ++n) {
        const size_t a = (size_t)b * N + n;
        pos[2 * a] = (pos[2 * a] + 1) % H;
        if ((n + t) % 3 == 0) {
          reach[a] = 1;
          if (end_step[a] == 0) end_step[a] = t;
        }
        if (n % 2 == 0 && first_move[a] == 0) first_move[a] = t;
      }
    }
    if (magat_sim_pool_turn(&d, 0, nullptr) != MAGAT_OK) return 3;
    line(slot_case); line(slot_step); line(slot_maxstep); line_f(radii);
    line(std::vector<int32_t>(counters.begin(), counters.begin() + 2));
    line(pos);
  }
  line(rows); line_f(r_radius); line(r_end_pos); line(r_first_move); line(r_end_step); line(traj_len); line(traj);
  return 0;
}
