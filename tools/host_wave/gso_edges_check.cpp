// Runs the edge-structure kernels - magat_gso_edges_build (csrc/gso_edges.hip) - on the host, one thread per lane of their
// four-wave workgroups (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/gso_edges_check.cpp -o gso_edges_check
//   gso_edges_check case.txt > result.txt
// (add -fsanitize=address,undefined to have every access of the kernels checked: every buffer here has exactly its documented
// size, the workspace included.)  case.txt: whitespace-separated B N rule cap per_instance, then the radii (B of them when
// per_instance, else one; any float syntax strtod reads, hex floats included) and pos (B N 2).  Out come, one line each: the
// return code, nnz, rowptr, colidx, cscptr, cscsrc, cscpos - the three index arrays with min(nnz, cap) entries.
// tests/test_host_edges.py compares it with tests/edges_restatement.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }      // (sim_connect.h's sweep)
int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}

#include "../../magat_pathplanning_amd/csrc/gso_edges.hip"

static void line(const int* v, long long n) {
  for (long long i = 0; i < n; ++i) printf("%d%c", v[i], i + 1 == n ? '\n' : ' ');
  if (n <= 0) printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int B, N, rule, per_instance;
  long long cap;
  if (!f || fscanf(f, "%d %d %d %lld %d", &B, &N, &rule, &cap, &per_instance) != 5) return 2;
  if (B <= 0 || N <= 0 || cap < 0) return 2;
  std::vector<double> radii(per_instance ? B : 1);
  for (auto& r : radii) {
    char word[64];
    if (fscanf(f, "%63s", word) != 1) return 2;
    r = strtod(word, nullptr);
  }
  std::vector<int32_t> pos((size_t)B * N * 2);
  for (auto& x : pos) {
    long long t;
    if (fscanf(f, "%lld", &t) != 1) return 2;
    x = (int32_t)t;
  }
  fclose(f);
  // every buffer has exactly its documented size; the index arrays do not exist when cap == 0
  std::vector<int> rowptr((size_t)B * (N + 1), -7), cscptr((size_t)B * (N + 1), -7);
  int* colidx = cap ? static_cast<int*>(malloc(cap * sizeof(int))) : nullptr;
  int* cscsrc = cap ? static_cast<int*>(malloc(cap * sizeof(int))) : nullptr;
  int* cscpos = cap ? static_cast<int*>(malloc(cap * sizeof(int))) : nullptr;
  for (long long k = 0; k < cap; ++k) colidx[k] = cscsrc[k] = cscpos[k] = -7;
  long long nnz = -7;
  const size_t bytes = magat_gso_edges_workspace_bytes(B, N);
  void* ws = bytes ? aligned_alloc(256, bytes) : nullptr;      // (a multiple of 256 bytes, dirty)
  if (ws) memset(ws, 0xa5, bytes);
  const int rc = magat_gso_edges_build(pos.data(), per_instance ? radii.data() : nullptr, per_instance ? 0.0 : radii[0], rule,
                                       rowptr.data(), colidx, cscptr.data(), cscsrc, cscpos, cap, &nnz, ws, bytes, B, N, nullptr);
  printf("%d\n%lld\n", rc, nnz);
  const long long kept = nnz < 0 ? 0 : nnz < cap ? nnz : cap;
  line(rowptr.data(), (long long)rowptr.size());
  line(colidx, kept);
  line(cscptr.data(), (long long)cscptr.size());
  line(cscsrc, kept);
  line(cscpos, kept);
  for (long long k = kept; k < cap; ++k)
    if (colidx[k] != -7 || cscsrc[k] != -7 || cscpos[k] != -7) return 4;      // nothing behind the edges is written
  free(ws);
  free(colidx);
  free(cscsrc);
  free(cscpos);
  return 0;
}
