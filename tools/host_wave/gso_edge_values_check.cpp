// Runs the edge-value kernel - magat_gso_edge_values (csrc/gso_edge_values.hip) - on the host, one thread per lane of its
// four-wave workgroup (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/gso_edge_values_check.cpp -o gso_edge_values_check
//   gso_edge_values_check case.txt > result.txt
// (add -fsanitize=address,undefined to have every access of the kernel checked: every buffer here has exactly its documented size,
// the workspace included, and the workspace is dirty.)  case.txt: whitespace-separated B N cap symmetric_norm normalize lds_limit
// nnz, then rowptr (B (N + 1)) and colidx (min(nnz, cap)).  lds_limit: bytes of LDS the entry may plan with, its static 144 included - at most the
// 128 KB of the stand-in; a small one sends the tridiagonal matrix to the workspace, as 4096 agents do on the device.  Out come, one line
// each: the return code, lambda (B hex floats), vals (min(nnz, cap) hex floats; an entry the kernel left alone prints as nan).
// tests/test_host_edge_values.py compares it with tests/edge_values_restatement.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../magat_pathplanning_amd/csrc/magat_common.h"

int magat_prof_begin(int, hipStream_t) { return -1; }
void magat_prof_end(int, hipStream_t) {}
void magat_form_note(int) {}
int magat_ensure_dyn_lds(const void*, int, size_t) { return MAGAT_OK; }

#include "../../magat_pathplanning_amd/csrc/gso_edge_values.hip"

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int B, N, sym, normalize;
  long long cap, nnz, limit;
  if (!f || fscanf(f, "%d %d %lld %d %d %lld %lld", &B, &N, &cap, &sym, &normalize, &limit, &nnz) != 7) return 2;
  if (B <= 0 || N <= 0 || cap < 0 || nnz < 0 || limit <= 0 || limit > (long long)sizeof(host_wave::dyn_lds)) return 2;
  gev_lds_limit = (size_t)limit;
  const long long kept = nnz < cap ? nnz : cap;
  std::vector<int> rowptr((size_t)B * (N + 1));
  for (auto& x : rowptr)
    if (fscanf(f, "%d", &x) != 1) return 2;
  // colidx and vals have exactly cap entries (they do not exist when cap == 0); lambda B; the workspace what the entry asks for
  int* colidx = cap ? static_cast<int*>(malloc(cap * sizeof(int))) : nullptr;
  float* vals = cap ? static_cast<float*>(malloc(cap * sizeof(float))) : nullptr;
  for (long long k = 0; k < cap; ++k) {
    colidx[k] = -7;
    vals[k] = nanf("");
  }
  for (long long k = 0; k < kept; ++k)
    if (fscanf(f, "%d", &colidx[k]) != 1) return 2;
  fclose(f);
  std::vector<double> lambda(B, -7.0);
  const size_t bytes = magat_gso_edge_values_workspace_bytes(B, N);
  void* ws = bytes ? aligned_alloc(256, bytes) : nullptr;      // (a multiple of 256 bytes, dirty)
  if (ws) memset(ws, 0xa5, bytes);
  const int rc = magat_gso_edge_values(rowptr.data(), colidx, &nnz, cap, sym, normalize, lambda.data(), vals, ws, bytes, B, N, nullptr);
  printf("%d\n", rc);
  for (int b = 0; b < B; ++b) printf("%a%c", lambda[b], b + 1 == B ? '\n' : ' ');
  for (long long k = 0; k < kept; ++k) printf("%a%c", (double)vals[k], k + 1 == kept ? '\n' : ' ');
  if (kept <= 0) printf("\n");
  free(ws);
  free(colidx);
  free(vals);
  return 0;
}
