// An optimal multi-agent path-finding expert for C cases at once: conflict-based search (CBS) on the device (the
// rule is in include/magat_hip.h, restated cell by cell in tests/cbs_restatement.py).  Optimal and complete up to a node budget,
// and its open list bounds the optimal flowtime from below.
//   magat_sim_mapf_cbs_workspace_bytes   per case: the constraint boards, the root's paths, the node pool, two cell rows
//   magat_sim_mapf_cbs                   one wavefront per case runs the whole tree; one launch, no host round trip
// The tree is sim_mapf_tree.h's walk, under the plain rule (FOCAL = false): the open node with the smallest (cost, index).  This
// file brings its form.  The layout of mapf_plan_kernel (sim_mapf.hip): lane = map row, one 64-bit word per row.  Per case:
//   constraint boards   workspace [t][V, A_up, A_left, A_down, A_right][row], zeroed here once; before a search the bits of the
//                       agent's chain are set by the lanes of their rows, after it exactly those are cleared.  No soft boards.
//   low-level search    the planner's (sim_mapf_parts.h): without boards for the root, on the constraint boards for a child; the
//                       arrival is t* itself.
//   node pool           workspace: 16 bytes per node (parent, cost, agent | board | open | length, t | cell) and its agent's new
//                       path, T cells of 16 bits (row << 8 | col); the root's N paths and lengths beside it.
//   LDS                 the R layers of a search, T * 512 bytes; their first 32 KB are the two cell-owner grids of the conflict scan
//                       as well (BORROWS_GRIDS: the walk sets them to "nobody" again after every search).
// Integer and bit arithmetic only.  Every store is a per-lane (vector) store or an LDS atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_MAX_N, audit_stage2 - the walk's conflict scan
#include "sim_mapf_cbs_parts.h"        // cbs_wave
#include "sim_mapf_parts.h"            // MAPF_*, mapf_search, mapf_backtrace
#include "sim_mapf_tree.h"             // cbs_node, mapf_tree_search, tree_entry_check

namespace {

constexpr int CBS_MAX_NODES = 4096;
constexpr size_t CBS_GRID_BYTES = 2 * MAPF_SIDE * MAPF_SIDE * sizeof(int);

// per case, in 64-bit words: boards | root paths | node paths | nodes | root lengths | the audit's two cell rows
struct cbs_layout {
  long long root, npath, nodes, rlen, at, words;
};
__host__ __device__ inline cbs_layout cbs_case_layout(int N, int T, int M) {
  cbs_layout l;
  l.root = (long long)T * MAPF_BOARDS * MAPF_SIDE;
  l.npath = l.root + ((long long)N * T + 3) / 4;
  l.nodes = l.npath + ((long long)M * T + 3) / 4;
  l.rlen = l.nodes + (long long)M * 2;
  l.at = l.rlen + ((long long)N + 1) / 2;
  l.words = l.at + N;
  return l;
}

struct cbs_form : cbs_wave {
  static constexpr bool FOCAL = false, BORROWS_GRIDS = true;
  u64* R;      // [T][64]
  int *own0, *own1;
  int T, W, ta;
  template <bool SET>
  __device__ __forceinline__ void reserve(const int*) const {}
  template <bool CHILD>
  __device__ __forceinline__ int search(int sr, int sc, int gr, int gc) {
    if constexpr (CHILD) ta = mapf_search<true>(hard, R, free, sr, sc, gr, gc, T, tid);
    else ta = mapf_search<false>(nullptr, R, free, sr, sc, gr, gc, T, tid);
    return ta;
  }
  template <bool CHILD>
  __device__ __forceinline__ void trace(int* cells, int gr, int gc) const {
    mapf_backtrace<CHILD>(CHILD ? hard : nullptr, R, cells, gr, gc, ta, W, tid);
  }
};

__global__ __launch_bounds__(64) void mapf_cbs_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                      const int* __restrict__ start, const int* __restrict__ goal, int* paths,
                                                      int* lengths, int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                      int* __restrict__ status, int* __restrict__ flowtime,
                                                      int* __restrict__ lower_bound, int* __restrict__ nodes_out,
                                                      int* __restrict__ expanded_out, int* __restrict__ horizon_hit, u64* workspace,
                                                      int N, int T, int max_nodes) {
  HIP_DYNAMIC_SHARED(u64, R)
  __shared__ int cells[MAPF_MAX_T];
  const int cs = blockIdx.x, lane = threadIdx.x;
  const cbs_layout lay = cbs_case_layout(N, T, max_nodes);
  u64* boards = workspace + (long long)cs * lay.words;
  const long long a0 = (long long)cs * N;
  const tree_case<cbs_node> k{start + a0 * 2, goal + a0 * 2, paths + a0 * T * 2, lengths + a0,
                              reinterpret_cast<uint16_t*>(boards + lay.root), reinterpret_cast<uint16_t*>(boards + lay.npath),
                              reinterpret_cast<cbs_node*>(boards + lay.nodes), reinterpret_cast<int*>(boards + lay.rlen), nullptr, nullptr,
                              reinterpret_cast<int*>(boards + lay.at), cells, N, T, H, W, max_nodes, 0};
  for (int i = lane; i < T * MAPF_BOARDS * MAPF_SIDE; i += 64) boards[i] = 0ull;
  cbs_form f{{{lane}, boards}, R, reinterpret_cast<int*>(R), reinterpret_cast<int*>(R) + MAPF_SIDE * MAPF_SIDE, T, W, 0};
  f.load_free(map + cs * map_stride, H, W);
  mapf_tree_search(f, k, tree_out{makespan, solved, status, flowtime, lower_bound, nodes_out, expanded_out, horizon_hit}, cs);
}

}  // namespace

extern "C" size_t magat_sim_mapf_cbs_workspace_bytes(int C, int N, int T, int max_nodes) {
  if (C <= 0 || N <= 0 || T <= 0 || max_nodes <= 0 || N > AUDIT_MAX_N || T > MAPF_MAX_T || max_nodes > CBS_MAX_NODES) return 0;
  return (size_t)C * (size_t)cbs_case_layout(N, T, max_nodes).words * sizeof(u64);
}

extern "C" int magat_sim_mapf_cbs(const uint8_t* map, int map_batched, int H, int W, const int32_t* start, const int32_t* goal,
                                  int32_t* paths, int32_t* lengths, int32_t* makespan, uint8_t* solved, int32_t* status,
                                  int32_t* flowtime, int32_t* lower_bound, int32_t* nodes, int32_t* expanded, int32_t* horizon_hit,
                                  void* workspace, size_t workspace_bytes, int C, int N, int T, int max_nodes, void* stream) {
  const int rc = tree_entry_check({map, start, goal, paths, lengths, makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit},
                                  H, W, C, N, T, max_nodes, true, true, MAPF_SIDE, MAPF_MAX_T, CBS_MAX_NODES, workspace, workspace_bytes,
                                  magat_sim_mapf_cbs_workspace_bytes(C, N, T, max_nodes));
  if (rc != MAGAT_OK) return rc;
  // dynamic LDS: the R layers or the two owner grids, whichever is larger: 32 .. 128 KB; + 1 KB static
  size_t lds = (size_t)T * MAPF_SIDE * sizeof(u64);
  lds = lds < CBS_GRID_BYTES ? CBS_GRID_BYTES : lds;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds > 64 * 1024 && magat_ensure_dyn_lds(reinterpret_cast<const void*>(&mapf_cbs_kernel), MAGAT_LDS_SIM_MAPF_CBS, lds) != MAGAT_OK)
    return MAGAT_ERR_LAUNCH;
  magat_form_note(MAGAT_FORM_SIM_MAPF_CBS);
  const int pid = magat_prof_begin(MAGAT_TAG_SIM_MAPF_CBS, st);
  hipLaunchKernelGGL(mapf_cbs_kernel, dim3((unsigned)C), dim3(64), lds, st, map, map_batched ? (long long)H * W : 0LL, H, W, start,
                     goal, paths, lengths, makespan, solved, status, flowtime, lower_bound, nodes, expanded, horizon_hit,
                     static_cast<u64*>(workspace), N, T, max_nodes);
  magat_prof_end(pid, st);
  return magat_check_launch();
}
