// An optimal multi-agent path-finding expert for C cases at once: conflict-based search (CBS) on the device (the
// rule is in include/magat_hip.h, restated cell by cell in tests/cbs_restatement.py).  Optimal and complete up to a node budget,
// and its open list bounds the optimal flowtime from below.
//   magat_sim_mapf_cbs_workspace_bytes   per case: the constraint boards, the root's paths, the node pool, two cell rows
//   magat_sim_mapf_cbs                   one wavefront per case runs the whole tree; one launch, no host round trip
// The layout of mapf_plan_kernel (sim_mapf.hip): lane = map row, one 64-bit word per row.  The low-level search of one agent IS
// the planner's (sim_mapf_parts.h) on boards that hold the agent's constraints; the conflict to branch on is the audit's stage 2
// (sim_mapf_audit_parts.h).  Per case:
//   constraint boards   workspace [t][V, A_up, A_left, A_down, A_right][row], zeroed here once; before a search the bits of the
//                       agent's chain are set by the lanes of their rows, after it exactly those are cleared.
//   node pool           workspace: 16 bytes per node (parent, cost, agent | board | open | length, t | cell) and its agent's new
//                       path, T cells of 16 bits (row << 8 | col); the root's N paths and lengths beside it.
//   schedule of a node  assembled into `paths` / `lengths` themselves (the outputs are the scratch): the chain to the root is
//                       walked once, an agent takes the path of the first node that names it - a bit per agent in a register
//                       of lane a >> 6 - and the root's otherwise.  The answer is then already where it belongs.
//   LDS                 the R layers of a search, T * 512 bytes; between two searches the first 32 KB of them are the two
//                       cell-owner grids of the conflict scan (they are filled again before every scan).
//   open list           a linear scan by the wave for the smallest (cost, index).
// Integer and bit arithmetic only.  Every store is a per-lane (vector) store or an LDS atomic from plain C++.
#include <cstdint>

#include "magat_common.h"
#include "row_board.h"
#include "sim_mapf_audit_parts.h"      // AUDIT_MAX_N, AUDIT_NONE, audit_stage2
#include "sim_mapf_cbs_parts.h"        // cbs_wave_min / _max, cbs_mark, cbs_mark_chain, cbs_place
#include "sim_mapf_parts.h"            // MAPF_*, mapf_search, mapf_backtrace

namespace {

constexpr int CBS_MAX_NODES = 4096;
constexpr int CBS_OPEN = 1 << 15;
constexpr size_t CBS_GRID_BYTES = 2 * MAPF_SIDE * MAPF_SIDE * sizeof(int);

struct cbs_node {
  int parent;
  int cost;      // the flowtime of the node's schedule; -1: the child found no arrival
  int who;       // agent | board << 12 | open << 15 | (length - 1) << 16
  int what;      // the constraint: t | row << 16 | col << 24
};

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

__global__ __launch_bounds__(64) void mapf_cbs_kernel(const uint8_t* __restrict__ map, long long map_stride, int H, int W,
                                                      const int* __restrict__ start, const int* __restrict__ goal, int* paths,
                                                      int* lengths, int* __restrict__ makespan, uint8_t* __restrict__ solved,
                                                      int* __restrict__ status, int* __restrict__ flowtime,
                                                      int* __restrict__ lower_bound, int* __restrict__ nodes_out,
                                                      int* __restrict__ expanded_out, int* __restrict__ horizon_hit, u64* workspace,
                                                      int N, int T, int max_nodes) {
  HIP_DYNAMIC_SHARED(u64, R)                      // [T][64]; between two searches: the owner grids of the conflict scan
  __shared__ int cells[MAPF_MAX_T];               // the path just traced
  const int cs = blockIdx.x, lane = threadIdx.x;
  const cbs_layout lay = cbs_case_layout(N, T, max_nodes);
  u64* boards = workspace + (long long)cs * lay.words;
  uint16_t* root = reinterpret_cast<uint16_t*>(boards + lay.root);
  uint16_t* npath = reinterpret_cast<uint16_t*>(boards + lay.npath);
  cbs_node* nodes = reinterpret_cast<cbs_node*>(boards + lay.nodes);
  int* rlen = reinterpret_cast<int*>(boards + lay.rlen);
  int* at = reinterpret_cast<int*>(boards + lay.at);
  int* own = reinterpret_cast<int*>(R);
  const long long a0 = (long long)cs * N;
  int* len = lengths + a0;
  int* rows = paths + a0 * T * 2;
  const int *st = start + a0 * 2, *gl = goal + a0 * 2;
  for (int i = lane; i < T * MAPF_BOARDS * MAPF_SIDE; i += 64) boards[i] = 0ull;
  const uint8_t* mp = map + cs * map_stride;
  u64 free = 0ull;
  for (int r = 0; r < H; ++r) {
    const u64 word = __builtin_amdgcn_ballot_w64(lane < W && mp[r * W + (lane < W ? lane : 0)] == 0);
    if (lane == r) free = word;
  }
  int state = -1, count = 0, expanded = 0, hit = 0, bound = -1;      // state: the status once it is known
  // screening: every start and goal on a free cell of its own, before any cell indexes anything
  u64 starts = 0ull, goals = 0ull;
  for (int a = 0; a < N && state < 0; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const bool inside = sr >= 0 && sr < H && sc >= 0 && sc < W && gr >= 0 && gr < H && gc >= 0 && gc < W;
    const u64 sbit = inside ? 1ull << sc : 0ull, gbit = inside ? 1ull << gc : 0ull;
    const bool ok = wave_any(lane == sr && (free & ~starts & sbit)) && wave_any(lane == gr && (free & ~goals & gbit));
    if (!ok) state = 3;
    if (lane == sr) starts |= sbit;
    if (lane == gr) goals |= gbit;
  }
  // the root: every agent's free path
  int cost = 0;
  for (int a = 0; a < N && state < 0; ++a) {
    const int sr = __builtin_amdgcn_readfirstlane(st[2 * a]), sc = __builtin_amdgcn_readfirstlane(st[2 * a + 1]);
    const int gr = __builtin_amdgcn_readfirstlane(gl[2 * a]), gc = __builtin_amdgcn_readfirstlane(gl[2 * a + 1]);
    const int tstar = mapf_search<false>(nullptr, R, free, sr, sc, gr, gc, T, lane);
    if (tstar < 0) {
      state = 2, hit = 1;
      break;
    }
    __syncthreads();
    mapf_backtrace<false>(nullptr, R, cells, gr, gc, tstar, W, lane);
    __syncthreads();
    for (int t = lane; t <= tstar; t += 64) root[(long long)a * T + t] = (uint16_t)cells[t];
    if (lane == 0) rlen[a] = tstar + 1;
    cost += tstar;
    __syncthreads();      // `cells` is traced again
  }
  if (state < 0) {
    if (lane == 0) nodes[0] = cbs_node{-1, cost, CBS_OPEN, 0};
    count = 1;
  }
  int best_cost = 0;
  while (state < 0) {
    __syncthreads();      // the nodes, their paths, the cleared boards
    // the open node with the smallest (cost, index)
    int bc = AUDIT_NONE, bi = AUDIT_NONE;
    for (int i = lane; i < count; i += 64) {
      const cbs_node nd = nodes[i];
      if ((nd.who & CBS_OPEN) && nd.cost < bc) bc = nd.cost, bi = i;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const int oc = __shfl_xor(bc, off, 64), oi = __shfl_xor(bi, off, 64);
      if (oc < bc || (oc == bc && oi < bi)) bc = oc, bi = oi;
    }
    if (bi == AUDIT_NONE) {
      state = 2;
      break;
    }
    best_cost = bc;
    __syncthreads();      // everybody has read the node before it is closed
    if (lane == 0) nodes[bi].who &= ~CBS_OPEN;
    // its schedule: the first node of the chain that names an agent holds its path, the root the others'
    u64 named = 0ull;      // agents 64 * lane .. 64 * lane + 63
    for (int i = bi; i > 0; i = __builtin_amdgcn_readfirstlane(nodes[i].parent)) {
      const int who = __builtin_amdgcn_readfirstlane(nodes[i].who), x = who & 4095;
      if (wave_any(lane == (x >> 6) && has_bit(named, x & 63))) continue;
      if (lane == (x >> 6)) named |= 1ull << (x & 63);
      const int lx = (who >> 16 & 255) + 1;
      cbs_place(rows + (long long)x * T * 2, npath + (long long)i * T, lx, T, lane);
      if (lane == 0) len[x] = lx;
    }
    for (int a = 0; a < N; ++a) {
      if (wave_any(lane == (a >> 6) && has_bit(named, a & 63))) continue;
      const int la = __builtin_amdgcn_readfirstlane(rlen[a]);
      cbs_place(rows + (long long)a * T * 2, root + (long long)a * T, la, T, lane);
      if (lane == 0) len[a] = la;
    }
    for (int i = lane; i < H * W; i += 64) own[i] = own[MAPF_SIDE * MAPF_SIDE + i] = AUDIT_NONE;
    __syncthreads();
    int t2 = -1;
    const int key2 = audit_stage2(rows, N, T, W, own, own + MAPF_SIDE * MAPF_SIDE, at, at + N, lane, 64, [](int key) {
      key = cbs_wave_min(key);
      __syncthreads();
      return key;
    }, &t2);
    if (key2 == AUDIT_NONE) {
      state = 0;
      break;
    }
    if (count + 2 > max_nodes) {
      state = 1, bound = bc;
      break;
    }
    ++expanded;
    const int kind = key2 & 1;
    for (int k = 0; k < 2; ++k) {
      const int x = k ? key2 >> 1 & 4095 : key2 >> 13, child = count + k;
      const int lx = __builtin_amdgcn_readfirstlane(len[x]);
      const int* px = rows + (long long)x * T * 2;
      const int th = t2 < lx ? t2 : lx - 1;
      int cr = __builtin_amdgcn_readfirstlane(px[2 * th]), cc = __builtin_amdgcn_readfirstlane(px[2 * th + 1]), board = 0;
      if (kind) {      // its own step at t2: from (fr, fc) in direction d - closed by bit (fr, fc) of A_opp(d)[t2]
        const int fr = __builtin_amdgcn_readfirstlane(px[2 * t2 - 2]), fc = __builtin_amdgcn_readfirstlane(px[2 * t2 - 1]);
        const int dr = cr - fr, dc = cc - fc, d = dr == -1 ? 0 : dc == -1 ? 1 : dr == 1 ? 2 : 3;
        board = 1 + ((d + 2) & 3), cr = fr, cc = fc;
      }
      cbs_mark<true>(boards, board, t2, cr, cc, lane);
      cbs_mark_chain<true>(boards, nodes, bi, x, lane);
      __syncthreads();
      const int sr = __builtin_amdgcn_readfirstlane(st[2 * x]), sc = __builtin_amdgcn_readfirstlane(st[2 * x + 1]);
      const int gr = __builtin_amdgcn_readfirstlane(gl[2 * x]), gc = __builtin_amdgcn_readfirstlane(gl[2 * x + 1]);
      const int tstar = mapf_search<true>(boards, R, free, sr, sc, gr, gc, T, lane);
      __syncthreads();
      if (tstar >= 0) {
        mapf_backtrace<true>(boards, R, cells, gr, gc, tstar, W, lane);
        __syncthreads();
        for (int t = lane; t <= tstar; t += 64) npath[(long long)child * T + t] = (uint16_t)cells[t];
      } else {
        hit = 1;
      }
      if (lane == 0)
        nodes[child] = cbs_node{bi, tstar >= 0 ? bc - (lx - 1) + tstar : -1,
                                x | board << 12 | (tstar >= 0 ? CBS_OPEN | tstar << 16 : 0), t2 | cr << 16 | cc << 24};
      __syncthreads();      // every load of the boards lies behind
      cbs_mark<false>(boards, board, t2, cr, cc, lane);
      cbs_mark_chain<false>(boards, nodes, bi, x, lane);
      __syncthreads();
    }
    count += 2;
  }
  // the answer stands in paths / lengths already; every other case gets the start cells
  int longest = 0;
  if (state == 0) {
    __syncthreads();
    for (int base = 0; base < N; base += 64) {
      const int b = base + lane, lb = b < N ? len[b] : 1;
      longest = lb - 1 > longest ? lb - 1 : longest;
    }
    longest = cbs_wave_max(longest);
  } else {
    __syncthreads();      // the conflict scan has read the rows
    for (int a = 0; a < N; ++a) {
      const int sr = st[2 * a], sc = st[2 * a + 1];
      int* p = rows + (long long)a * T * 2;
      for (int t = lane; t < T; t += 64) {
        p[2 * t] = sr;
        p[2 * t + 1] = sc;
      }
      if (lane == 0) len[a] = 1;
    }
  }
  if (lane == 0) {
    makespan[cs] = longest;
    solved[cs] = state == 0 ? 1 : 0;
    status[cs] = state;
    flowtime[cs] = state == 0 ? best_cost : -1;
    lower_bound[cs] = state == 0 ? best_cost : bound;
    nodes_out[cs] = count;
    expanded_out[cs] = expanded;
    horizon_hit[cs] = hit;
  }
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
  if (!map || !start || !goal || !paths || !lengths || !makespan || !solved || !status || !flowtime || !lower_bound || !nodes ||
      !expanded || !horizon_hit || !workspace)
    return MAGAT_ERR_NULL;
  if (H <= 0 || W <= 0 || C <= 0 || N <= 0 || T <= 0 || max_nodes <= 0) return MAGAT_ERR_BAD_SHAPE;
  if (H > MAPF_SIDE || W > MAPF_SIDE || T > MAPF_MAX_T || N > AUDIT_MAX_N || max_nodes > CBS_MAX_NODES) return MAGAT_ERR_UNSUPPORTED;
  if (workspace_bytes < magat_sim_mapf_cbs_workspace_bytes(C, N, T, max_nodes)) return MAGAT_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(workspace) % sizeof(u64)) return MAGAT_ERR_WORKSPACE;
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
