// Runs the kernel of magat_sim_expert_pick (csrc/sim_expert_pick.h) on the host, one thread per lane of its workgroups
// (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/expert_pick_check.cpp -o pick_check
//   pick_check case.txt > result.txt
// (add -fsanitize=address,undefined to have every access of the kernel checked: every buffer here has exactly its documented
// size.)  case.txt: whitespace-separated count N Lcap H W M has_maps, then cells (count N Lcap), lengths (count N), goal
// (count N 2), makespan (count), radii (count, decimal), cum (count), maps (count H W, when has_maps), indices (M); out come
// the flag, then case, step, pos, target, action, goal, radii and map (when has_maps), one line each.
// tests/test_host_memory.py compares it with tests/memory_restatement.py.
#include <cstdio>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"
#include "../../magat_pathplanning_amd/csrc/sim_expert_pick.h"

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
static void print_all(const std::vector<T>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf("%lld%c", (long long)v[i], i + 1 == v.size() ? '\n' : ' ');
  if (v.empty()) printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  int count, N, Lcap, H, W, M, has_maps;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d", &count, &N, &Lcap, &H, &W, &M, &has_maps) != 7) return 2;
  if (count <= 0 || N <= 0 || Lcap <= 0 || H <= 0 || W <= 0 || M <= 0) return 2;
  const size_t HW = (size_t)H * W;
  std::vector<uint16_t> cells((size_t)count * N * Lcap);
  std::vector<int32_t> lengths((size_t)count * N), goal((size_t)count * N * 2), makespan(count);
  std::vector<double> radii(count);
  std::vector<long long> cum(count), indices(M);
  std::vector<uint8_t> maps(has_maps ? count * HW : 0);
  if (!read_all(f, cells) || !read_all(f, lengths) || !read_all(f, goal) || !read_all(f, makespan)) return 2;
  for (auto& r : radii)
    if (fscanf(f, "%lf", &r) != 1) return 2;
  if (!read_all(f, cum) || !read_all(f, maps) || !read_all(f, indices)) return 2;
  fclose(f);
  std::vector<int32_t> case_out(M, -7), step_out(M, -7), pos((size_t)M * N * 2, -7), goal_out((size_t)M * N * 2, -7), flag(1, 0x7fffffff);
  std::vector<float> target((size_t)M * N * 5, -7.f);
  std::vector<long long> action((size_t)M * N, -7);
  std::vector<double> radii_out(M, -7.0);
  std::vector<uint8_t> map_out(has_maps ? M * HW : 0, 7);
  ExpertPickArgs a;
  a.cells = cells.data(); a.lengths = lengths.data(); a.goal = goal.data(); a.makespan = makespan.data(); a.radii = radii.data();
  a.cum = cum.data(); a.maps = has_maps ? maps.data() : nullptr; a.indices = indices.data();
  a.case_out = case_out.data(); a.step_out = step_out.data(); a.pos = pos.data(); a.target = target.data(); a.action = action.data();
  a.goal_out = goal_out.data(); a.radii_out = radii_out.data(); a.map_out = has_maps ? map_out.data() : nullptr; a.flag = flag.data();
  a.count = count; a.N = N; a.Lcap = Lcap; a.HW = (int)HW; a.M = M;
  a.map_words = has_maps && HW % 4 == 0;      // (vectors are aligned; the library's launcher looks at the pointers too)
  const long long items = (long long)M * N;
  hipLaunchKernelGGL(expert_pick_kernel, dim3((unsigned)((items + EXPERT_PICK_THREADS - 1) / EXPERT_PICK_THREADS)),
                     dim3(EXPERT_PICK_THREADS), 0, nullptr, a);
  print_all(flag);
  print_all(case_out);
  print_all(step_out);
  print_all(pos);
  print_all(target);
  print_all(action);
  print_all(goal_out);
  for (int m = 0; m < M; ++m) printf("%.17g%c", radii_out[m], m + 1 == M ? '\n' : ' ');
  print_all(map_out);
  return 0;
}
