// Runs csrc/sim_mapf_lns_wide.hip on the host, one thread per lane of a workgroup of 1 to 4 wavefronts (hip/hip_runtime.h next to
// this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/mapf_lns_wide_check.cpp -o lns_wide_check
//   lns_wide_check case.txt > result.txt
// (add -fsanitize=address,undefined, or -fsanitize=thread, to have every access and every barrier of the kernel checked).
// case.txt and result.txt are those of mapf_lns_check.cpp: whitespace-separated integers C N T H W iterations k map_batched, the
// map(s), solved (C), paths (C N T 2), lengths (C N), makespan (C); out come the return code, then paths, lengths, makespan,
// flowtime_before, flowtime_after, accepted, status.  tests/test_host_lns_wide.py compares it with the restatement.
#include <cstdio>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}

#include "../../magat_pathplanning_amd/csrc/sim_mapf_lns_wide.hip"

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
  int C, N, T, H, W, iterations, k, batched;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d %d", &C, &N, &T, &H, &W, &iterations, &k, &batched) != 8) return 2;
  std::vector<uint8_t> map((size_t)(batched ? C : 1) * H * W), solved(C);
  std::vector<int32_t> paths((size_t)C * N * T * 2), lengths((size_t)C * N), makespan(C), fb(C, -7), fa(C, -7), acc(C, -7), status(C, -7);
  if (!read_all(f, map) || !read_all(f, solved) || !read_all(f, paths) || !read_all(f, lengths) || !read_all(f, makespan)) return 2;
  fclose(f);
  const size_t bytes = magat_sim_mapf_improve_wide_workspace_bytes(C, H, W, N, T);
  std::vector<unsigned long long> ws(bytes / 8 + 1, 0xa5a5a5a5a5a5a5a5ull);      // exactly the size asked for: a sanitizer sees one word too far
  ws.resize(bytes / 8);
  const int rc = magat_sim_mapf_improve_wide(map.data(), batched, H, W, solved.data(), paths.data(), lengths.data(), makespan.data(),
                                             fb.data(), fa.data(), acc.data(), status.data(), ws.data(), bytes, C, N, T, iterations, k,
                                             nullptr);
  printf("%d\n", rc);
  print_all(paths);
  print_all(lengths);
  print_all(makespan);
  print_all(fb);
  print_all(fa);
  print_all(acc);
  print_all(status);
  return 0;
}
