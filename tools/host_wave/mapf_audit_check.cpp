// Runs csrc/sim_mapf_audit.hip and csrc/sim_mapf_audit_wide.hip on the host, one thread per lane of a workgroup of 1 to 4
// wavefronts (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/mapf_audit_check.cpp -o audit_check
//   audit_check 64|wide case.txt > result.txt
// (add -fsanitize=address,undefined, or -fsanitize=thread, to have every access and every barrier of the kernels checked).
// case.txt: whitespace-separated integers C N T H W map_batched has_solved, the map(s), solved (C, when has_solved), paths
// (C N T 2), lengths (C N), start (C N 2), goal (C N 2); out come the return code, then status, fault, dist, flowtime_bound,
// makespan_bound, flowtime, makespan, one line each.  tests/test_host_audit.py compares it with the restatement.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}

#include "../../magat_pathplanning_amd/csrc/sim_mapf_audit.hip"
#include "../../magat_pathplanning_amd/csrc/sim_mapf_audit_wide.hip"

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
  if (argc < 3) return 2;
  const bool wide = strcmp(argv[1], "wide") == 0;
  FILE* f = fopen(argv[2], "r");
  int C, N, T, H, W, batched, has_solved;
  if (!f || fscanf(f, "%d %d %d %d %d %d %d", &C, &N, &T, &H, &W, &batched, &has_solved) != 7) return 2;
  std::vector<uint8_t> map((size_t)(batched ? C : 1) * H * W), solved(has_solved ? C : 0);
  std::vector<int32_t> paths((size_t)C * N * T * 2), lengths((size_t)C * N), start((size_t)C * N * 2), goal((size_t)C * N * 2);
  std::vector<int32_t> status(C, -7), fault((size_t)C * 4, -7), dist((size_t)C * N, -7), fb(C, -7), mb(C, -7), flow(C, -7), span(C, -7);
  if (!read_all(f, map) || !read_all(f, solved) || !read_all(f, paths) || !read_all(f, lengths) || !read_all(f, start) ||
      !read_all(f, goal))
    return 2;
  fclose(f);
  const size_t bytes = wide ? magat_sim_mapf_audit_wide_workspace_bytes(C, H, W, N, T) : magat_sim_mapf_audit_workspace_bytes(C, N, T);
  std::vector<unsigned long long> ws(bytes / 8 + 1, 0xa5a5a5a5a5a5a5a5ull);      // exactly the size asked for: a sanitizer sees one word too far
  ws.resize(bytes / 8);
  const uint8_t* sv = has_solved ? solved.data() : nullptr;
  const int rc = wide ? magat_sim_mapf_audit_wide(map.data(), batched, H, W, sv, paths.data(), lengths.data(), start.data(), goal.data(),
                                                  status.data(), fault.data(), dist.data(), fb.data(), mb.data(), flow.data(),
                                                  span.data(), ws.data(), bytes, C, N, T, nullptr)
                      : magat_sim_mapf_audit(map.data(), batched, H, W, sv, paths.data(), lengths.data(), start.data(), goal.data(),
                                             status.data(), fault.data(), dist.data(), fb.data(), mb.data(), flow.data(), span.data(),
                                             ws.data(), bytes, C, N, T, nullptr);
  printf("%d\n", rc);
  print_all(status);
  print_all(fault);
  print_all(dist);
  print_all(fb);
  print_all(mb);
  print_all(flow);
  print_all(span);
  return 0;
}
