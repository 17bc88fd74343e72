// The communication graph's edge test and connectivity sweep, shared by the simulator's step-0 radius (sim_frontend.hip) and
// the data transformer's carried radius (sim_expert.hip): one copy, so that both grow their radii on the same predicate.
#pragma once
#include "magat_common.h"

// The reference's edge test is float64: sqrt(dx^2 + dy^2) < R on integer cell offsets.  The correctly rounded square root is
// monotone, so the test is "squared distance < q" for one integer q per radius: the smallest q whose rounded root is not below R,
// found by stepping from floor(R^2) with the very same float64 expression - exact, and no square root per pair.
__device__ inline long long sim_dist2_bound(double R) {
  if (!(R > 0.0)) return 0;                                  // sqrt(.) >= 0: nothing is closer than R
  if (R >= 3.0e9) return 0x7fffffffffffffffLL;               // int32 coordinates: squared distances stay below 2^65 / 4
  long long q = (long long)floor(R * R);
  while (q > 0 && !(sqrt((double)(q - 1)) < R)) --q;
  while (sqrt((double)q) < R) ++q;
  return q;
}

// Is the graph (squared distance < d2_bound, no self loops) over the N agents px / py connected?  The reference tests this
// through the Laplacian's spectrum (graphTools.isConnected: exactly one eigenvalue below 1e-9); here it is a reachability
// sweep from agent 0 over the same distance test - the same predicate, evaluated exactly.  Called by every thread of the
// workgroup (t of nt); px, py, seen [N] and the two words changed / count live in LDS.  Begins and ends with a barrier.
__device__ inline bool sim_graph_connected(const int* px, const int* py, int* seen, int* changed, int* count, int N,
                                           long long d2_bound, int t, int nt) {
  __syncthreads();
  for (int n = t; n < N; n += nt) seen[n] = n == 0 ? 1 : 0;
  while (true) {
    __syncthreads();
    if (t == 0) *changed = 0;
    __syncthreads();
    for (int i = t; i < N; i += nt) {
      if (seen[i]) continue;
      bool hit = false;
      for (int j = 0; j < N && !hit; ++j) {
        if (!seen[j] || j == i) continue;
        const long long dx = px[i] - px[j], dy = py[i] - py[j];
        hit = dx * dx + dy * dy < d2_bound;
      }
      if (hit) { seen[i] = 1; *changed = 1; }
    }
    __syncthreads();
    if (!*changed) break;
  }
  if (t == 0) *count = 0;
  __syncthreads();
  int c = 0;
  for (int n = t; n < N; n += nt) c += seen[n];
  if (c) atomicAdd(count, c);
  __syncthreads();
  return *count == N;
}
