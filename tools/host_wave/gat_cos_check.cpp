// Runs gat_cos_backward_kernel (csrc/gat_cos_parts.h: the backward of GAT_Similarity's normalisation) on the host, one thread per
// lane of its four-wave workgroups (hip/hip_runtime.h next to this file), without a GPU:
//   c++ -std=c++17 -O1 -g -pthread -I tools/host_wave -x c++ tools/host_wave/gat_cos_check.cpp -o gat_cos_check
//   gat_cos_check case.txt > result.txt
// (add -fsanitize=address,undefined to have every access of the kernel checked: every buffer here has exactly its documented
// size.)  case.txt: the integers G M NC qoff blocks, then Xhat (M G), Z (M NC), norms (2 M), dXd (M G), dZ (M NC) as the bit
// patterns of their float32 values, whitespace-separated; out come dXd and dZ after the kernel, the same way, one line each.
// tests/test_host_similarity_train.py compares them with the restatement in tests/similarity_train_cases.py.
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

static inline float cos_host_shfl(float v, int mask) {      // (the stand-in's shuffle exchanges ints)
  int u;
  memcpy(&u, &v, 4);
  u = host_wave::shfl_xor(u, mask);
  memcpy(&v, &u, 4);
  return v;
}
#undef __shfl_xor
#define __shfl_xor(v, m, w) cos_host_shfl(v, m)

#include "../../magat_pathplanning_amd/csrc/gat_cos_parts.h"

static bool read_all(FILE* f, std::vector<float>& v) {
  for (auto& x : v) {
    unsigned u;
    if (fscanf(f, "%u", &u) != 1) return false;
    memcpy(&x, &u, 4);
  }
  return true;
}

static void print_all(const std::vector<float>& v) {
  for (size_t i = 0; i < v.size(); ++i) {
    unsigned u;
    memcpy(&u, &v[i], 4);
    printf("%u%c", u, i + 1 == v.size() ? '\n' : ' ');
  }
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  int G, NC, qoff, blocks;
  long long M;
  if (!f || fscanf(f, "%d %lld %d %d %d", &G, &M, &NC, &qoff, &blocks) != 5) return 2;
  if (M <= 0 || blocks <= 0 || qoff < 0 || (qoff & 3) || (NC & 3) || qoff + G > NC) return 2;
  std::vector<float> Xhat((size_t)M * G), Z((size_t)M * NC), norms((size_t)2 * M), dXd((size_t)M * G), dZ((size_t)M * NC);
  if (!read_all(f, Xhat) || !read_all(f, Z) || !read_all(f, norms) || !read_all(f, dXd) || !read_all(f, dZ)) return 2;
  fclose(f);
  const float *xh = Xhat.data(), *z = Z.data(), *nr = norms.data();
  float *dx = dXd.data(), *dz = dZ.data();
  switch (G) {
    case 16: hipLaunchKernelGGL(gat_cos_backward_kernel<16>, dim3(blocks), dim3(256), 0, nullptr, xh, z, nr, dx, dz, M, NC, qoff); break;
    case 32: hipLaunchKernelGGL(gat_cos_backward_kernel<32>, dim3(blocks), dim3(256), 0, nullptr, xh, z, nr, dx, dz, M, NC, qoff); break;
    case 64: hipLaunchKernelGGL(gat_cos_backward_kernel<64>, dim3(blocks), dim3(256), 0, nullptr, xh, z, nr, dx, dz, M, NC, qoff); break;
    case 128: hipLaunchKernelGGL(gat_cos_backward_kernel<128>, dim3(blocks), dim3(256), 0, nullptr, xh, z, nr, dx, dz, M, NC, qoff); break;
    case 256: hipLaunchKernelGGL(gat_cos_backward_kernel<256>, dim3(blocks), dim3(256), 0, nullptr, xh, z, nr, dx, dz, M, NC, qoff); break;
    default: return 2;
  }
  print_all(dXd);
  print_all(dZ);
  return 0;
}
