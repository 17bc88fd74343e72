// Runs csrc/sim_mapf_ecbs_wide.hip on the host, one thread per lane of a workgroup of 1 to 4 wavefronts (hip/hip_runtime.h next to
// this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/mapf_ecbs_wide_check.cpp -o ecbs_wide_check
//   ecbs_wide_check case.txt > result.txt
// (add -fsanitize=address,undefined, or -fsanitize=thread, to have every access and every barrier of the kernel checked).
// case.txt and result.txt are those of mapf_ecbs_check.cpp:
// whitespace-separated integers C N T H W max_nodes map_batched w_milli levels, the map(s), start (C N 2), goal (C N 2).
// result.txt: the return code, then paths, lengths, makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit.
// tests/test_host_ecbs_wide.py compares it with the restatement.
#include <cstdio>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}

#include "../../magat_pathplanning_amd/csrc/sim_mapf_ecbs_wide.hip"

template <typename T>
static bool read_all(FILE* f, std::vector<T>& v) {
  for (auto& x : v) {
    long long t;
    if (fscanf(f, "%lld", &t) != 1) return false;
    x = (T)t;
  }
  return true;
}
static void print_all(const std::vector<int32_t>& v) {
  for (size_t i = 0; i < v.size(); ++i) printf("%d%c", v[i], i + 1 == v.size() ? '\n' : ' ');
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int C, N, T, H, W, max_nodes, batched, w_milli, levels;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d %d", &C, &N, &T, &H, &W, &max_nodes, &batched, &w_milli, &levels) != 9) return 2;
  std::vector<uint8_t> map((size_t)(batched ? C : 1) * H * W), solved(C, 9);
  std::vector<int32_t> start((size_t)C * N * 2), goal((size_t)C * N * 2), paths((size_t)C * N * T * 2, -7), lengths((size_t)C * N, -7);
  std::vector<int32_t> out[8];
  for (auto& o : out) o.assign(C, -7);
  if (!read_all(f, map) || !read_all(f, start) || !read_all(f, goal)) return 2;
  fclose(f);
  const size_t bytes = magat_sim_mapf_ecbs_wide_workspace_bytes(C, H, W, N, T, max_nodes, levels);
  std::vector<unsigned long long> ws(bytes / 8 + 1, 0xa5a5a5a5a5a5a5a5ull);      // exactly the size asked for: a sanitizer sees one word too far
  ws.resize(bytes / 8);
  const int rc = magat_sim_mapf_ecbs_wide(map.data(), batched, H, W, start.data(), goal.data(), paths.data(), lengths.data(),
                                          out[0].data(), solved.data(), out[1].data(), out[2].data(), out[3].data(), out[4].data(),
                                          out[5].data(), out[6].data(), ws.data(), bytes, C, N, T, max_nodes, w_milli, levels, nullptr);
  printf("%d\n", rc);
  print_all(paths);
  print_all(lengths);
  print_all(out[0]);
  print_all(std::vector<int32_t>(solved.begin(), solved.end()));
  for (int i = 1; i <= 6; ++i) print_all(out[i]);
  return 0;
}
