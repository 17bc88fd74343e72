// Which launches one call of the CSR graph layer takes (magat_gat_forward_cs[rc]_*, magat_gnn_forward_csr_f32, the training
// forwards magat_gat_train_forward_*): ONE pure function of the call's scalars, a few flags, two options and the device's CU
// count, so that the decision can be checked on a CPU (tools/host_wave/gat_csr_route_check.cpp against
// tests/gat_csr_route_restatement.py).  Every admission condition, every grid and the workspace layout stand here once.
// Plain C++, no HIP.  gat_csr_f32.hip reads the Route and launches; gat_csr_fused.hip is handed its grids; gat_train.hip shares
// the agent limit, the rows grid and the dimension check.
#pragma once
#include <cstddef>

#include "gat_route.h"

namespace magat_csr {

using magat_gat::kXcd;
using magat_gat::MODE_GNN;
using magat_gat::MODE_KEYQUERY;
using magat_gat::MODE_GAT_ORIGIN;
using magat_gat::MODE_SIMILARITY;
using magat_gat::pack_columns;
using magat_gat::supported_width;

// Largest N of the entries that transpose the GSO themselves (magat_hip.h: "any N <= 8190"): csr_transpose_kernel keeps
// 2 N + 2 ints in LDS, under 64 KiB.  (The check once read `bytes > 64 KiB` and let N = 8191 - exactly 64 KiB - through.)
constexpr int kCsrMaxN = 8190;
static_assert((2 * kCsrMaxN + 2) * sizeof(int) < 64 * 1024 && (2 * (kCsrMaxN + 1) + 2) * sizeof(int) >= 64 * 1024, "");
constexpr int kTiledMinN = 8, kTiledMaxN = 1024;      // the LDS-tiled score and hop kernels: 8 rows per wave step, 16 waves of 8 steps
constexpr int kFusedWaves = 8;                        // gat_csr_fused.hip: waves per workgroup, 32 graph rows each
constexpr long long kGridMax = 0x7fffffffLL;

// B > 0 && N > 0 && nnz >= 0 && K > 0 && P > 0 (&& G > 0 && F > 0 where the entry checks the widths here and not by supported_width)
inline bool dims_ok(int B, int N, long long nnz, int K, int P, int G = 1, int F = 1) {
  return !(B <= 0 || N <= 0 || nnz < 0 || G <= 0 || F <= 0 || K <= 0 || P <= 0);
}
// workgroups of a launch that keeps an instance on one XCD: whole XCD rounds of instances, `per_instance` workgroups each
inline long long xcd_grid(int B, long long per_instance) { return (long long)((B + kXcd - 1) / kXcd) * kXcd * per_instance; }
// ... of a wave-per-row launch: `per_instance_factor` x 4-row tiles each
inline long long rows_grid(int B, int N, int per_instance_factor) { return xcd_grid(B, (long long)per_instance_factor * ((N + 3) / 4)); }

enum Pass { PASS_INFER = 0, PASS_TRAIN = 1, PASS_TRAIN_COS = 2 };
enum Refusal {             // in the order the entries answer them
  REFUSE_NONE = 0,
  REFUSE_DIMS = 1,         // a dimension <= 0, nnz < 0                                                  MAGAT_ERR_BAD_SHAPE
  REFUSE_MODE = 2,         // not a mode of this entry                                                   MAGAT_ERR_UNSUPPORTED
  REFUSE_COSINE = 3,       // GAT_Similarity: float32 only, one head, G = F                              MAGAT_ERR_UNSUPPORTED
  REFUSE_GNN = 4,          // GraphFilterBatch: one head, edge values for the hops, G a multiple of 4    MAGAT_ERR_BAD_SHAPE
  REFUSE_SHAPE = 5,        // G != F (attention modes), a width without kernels                          MAGAT_ERR_UNSUPPORTED
  REFUSE_AGENTS = 6,       // N > kCsrMaxN                                                               MAGAT_ERR_UNSUPPORTED
  REFUSE_LDY = 7,          // ldy below the row width or not a multiple of 4                             MAGAT_ERR_BAD_SHAPE
  REFUSE_XALIGN = 8,       // X not on a 16-byte boundary                                                MAGAT_ERR_UNSUPPORTED
  REFUSE_GRID = 9,         // training: B N or the hop grid beyond an int, refused before the maps GEMM  MAGAT_ERR_BAD_SHAPE
                           // (inference refuses a grid where it would launch it: the launchers compare with kGridMax)
  REFUSE_BF16_MAPS = 10    // bf16 storage, unfused: the conv GEMM wants NC and G in multiples of 32; answered BEHIND the
                           // workspace check, like before                                              MAGAT_ERR_UNSUPPORTED
};
enum Code { CODE_OK = 0, CODE_BAD_SHAPE = 1, CODE_UNSUPPORTED = 2 };      // (gat_csr_f32.hip maps them to MAGAT_*)
inline Code refusal_code(Refusal r) {
  return r == REFUSE_NONE ? CODE_OK : (r == REFUSE_DIMS || r == REFUSE_GNN || r == REFUSE_LDY || r == REFUSE_GRID) ? CODE_BAD_SHAPE : CODE_UNSUPPORTED;
}
enum Maps {
  MAPS_NONE = 0,           // the fused form: the maps run on the matrix cores inside the graph kernels
  MAPS_AUTO = 1,           // magat_gat_maps_gemm: the guarded f16x3 split GEMM, or float32 MFMA where option GAT_SPLIT or the shape says so
  MAPS_F32 = 2,            // forced float32 MFMA: GAT_Similarity (the direction of a tiny agent's q_j must survive) and training
                           // (Z is kept for the backward; caller-owned buffers have no status word for a guarded split GEMM)
  MAPS_BF16 = 3            // bf16 in, bf16 out on the conv GEMM (weights = plane 0 of the packed bf16x3 block)
};
enum Graph { GRAPH_NONE = 0, GRAPH_EDGE = 1, GRAPH_TILED = 2 };      // per-edge gathers from L2, or the LDS-tiled kernels
enum K1 {
  K1_NONE = 0,
  K1_ALONE = 1,            // K = 1 and nobody wants the attention values (or there are none: GraphFilterBatch): csr_k1_kernel only
  K1_AFTER_SCORES = 2      // K = 1, behind the transposition (training) and the scores
};

struct RouteIn {
  int B, N;
  long long nnz;
  int G, F, K, P, mode, concat, ldy;
  int esz;                 // bytes of a stored feature: 4 (float) or 2 (bf16)
  bool have_csc;           // the caller brings the column view magat_gso_csr_build made
  bool attention;          // the caller wants the attention values (att_opt)
  bool edge_vals;          // GraphFilterBatch: the GSO values were handed over
  bool y_f32;              // bf16 storage with float32 result rows
  bool x_aligned;          // X on a 16-byte boundary
  Pass pass;
  int csr_tiled, csr_fused;      // the options, read once per call
  int cus;                 // compute units of the current device
};

struct Workspace {         // byte offsets into the caller's workspace (256-byte aligned pieces) and the size of all of it
  size_t status, z, cscptr, cscsrc, cscpos, csctmp, att, t0, t1, ytmp, order, xhat, total;
};

struct Route {
  Refusal refusal;
  bool fused;              // gat_csr_fused.hip: rank, scores and hop kernels; none of the launches below but the grids fused_*
  Maps maps;
  bool prepare;            // gat_cos_prepare_kernel behind the maps GEMM
  bool cos_train_note;     // form counter MAGAT_FORM_GAT_COS_TRAIN
  bool transpose;          // csr_transpose_kernel + csr_sort_columns_kernel run in this call ...
  bool transpose_booked;   // ... under MAGAT_TAG_GSO_CSR (inference books them, the training forward never did)
  Graph scores;
  K1 k1;
  int hops;                // K - 1, or 0 in the forms without hop launches
  Graph hop_kind;
  int hop_buffers;         // of the workspace: hop h writes buffer h & 1 (training: the caller's T_k block instead)
  bool head_mean;          // head_mean_relu_csr_kernel merges the heads from Ytmp
  int act_relu;            // ReLU in the last store (not for GraphFilterBatch, not in training: autograd owns it; mean: in the merge)
  int NC;                  // columns of Z
  long long grid_transpose, grid_sort, grid_scores, grid_k1, grid_hop, grid_mean;      // 0 = not launched
  long long grid_fused_rank, grid_fused_scores, grid_fused_hop;                        // (rank: x of a (B, 2) grid)
  Workspace ws;            // inference only
};

// ---- admission ------------------------------------------------------------------------------------------------------------------
// the form with the maps inside the graph kernels (gat_csr_fused.hip): bf16 storage + the column view of magat_gso_csr_build
inline bool fused_form(const RouteIn& in) {
  return in.esz == 2 && in.have_csc && in.csr_fused && in.mode == MODE_KEYQUERY && in.K == 2 && in.G == 128 && in.F == 128 &&
         in.concat && (in.P == 1 || in.P == 2 || in.P == 4);
}
// which: 1 = scores, 2 = hop (option CSR_TILED = bit mask); a row of `width` features is a whole number of 128-byte slices
inline bool tiled_ok(const RouteIn& in, int width, int which) {
  return (in.csr_tiled & which) && in.N <= kTiledMaxN && in.N >= kTiledMinN && (width * in.esz) % 128 == 0;
}

inline Workspace workspace(const RouteIn& in, bool fused) {
  const size_t B = (size_t)in.B, N = (size_t)in.N, nnz = (size_t)in.nnz, esz = (size_t)in.esz;
  Workspace w;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
  w.status = take(256);              // range-guard status words of the maps GEMM (first bytes of the workspace)
  w.z = take(fused ? 0 : B * N * pack_columns(in.G, in.F, in.K, in.P, in.mode) * esz);      // (the fused form has no maps in memory)
  // (the column view: nothing is reserved for it when the caller brings the one magat_gso_csr_build made)
  w.cscptr = take(in.have_csc ? 0 : B * (N + 1) * sizeof(int));
  w.cscsrc = take(in.have_csc ? 0 : nnz * sizeof(int));
  w.cscpos = take(in.have_csc ? 0 : nnz * sizeof(int));
  w.csctmp = take(in.have_csc ? 0 : nnz * sizeof(int));
  w.att = take((size_t)in.P * nnz * sizeof(float));
  const size_t tb = in.K > 2 ? B * N * in.P * in.F * esz : 0;
  w.t0 = take(tb);
  w.t1 = take(in.K > 3 ? tb : 0);
  w.ytmp = take(in.concat ? 0 : B * N * in.P * in.F * esz);
  w.order = take(fused ? 2 * B * N * sizeof(int) : 0);      // csr_rank_kernel: rows by out-degree, rows by in-degree
  w.xhat = take(in.mode == MODE_SIMILARITY ? B * N * in.G * sizeof(float) : 0);      // normalised X rows (magat_gat_cos_prepare)
  w.total = o;
  return w;
}

inline Route route(const RouteIn& in) {
  const int B = in.B, N = in.N, G = in.G, F = in.F, K = in.K, P = in.P, mode = in.mode;
  Route r = {};
  auto refuse = [&](Refusal why) { r.refusal = why; return r; };
  const bool train = in.pass != PASS_INFER;
  if (!(train ? dims_ok(B, N, in.nnz, K, P) : dims_ok(B, N, in.nnz, K, P, G, F))) return refuse(REFUSE_DIMS);
  if (mode < MODE_KEYQUERY || mode > (train ? MODE_GAT_ORIGIN : MODE_SIMILARITY)) return refuse(REFUSE_MODE);
  const bool gnn = mode == MODE_GNN;      // fixed edge weights (the GSO values) instead of attention
  // GAT_Similarity: float32 only, one head; the generic score and hop kernels run as KeyQuery on normalised operands
  const bool cosine = mode == MODE_SIMILARITY;
  if (cosine && (in.esz != 4 || P != 1 || G != F)) return refuse(REFUSE_COSINE);
  if (gnn && (P != 1 || (in.nnz > 0 && K > 1 && !in.edge_vals) || (G & 3))) return refuse(REFUSE_GNN);
  if ((!gnn && G != F) || !supported_width(F)) return refuse(REFUSE_SHAPE);
  if (N > kCsrMaxN) return refuse(REFUSE_AGENTS);
  r.NC = pack_columns(G, F, K, P, mode);
  r.grid_k1 = 2048;
  r.hops = K - 1;
  // per-edge forms: scores 8 lanes per row (fewer below 32 features), 256 / lanes rows per workgroup; hops a wave per row
  const int score_rows = 256 / ((G / 4) < 8 ? (G / 4) : 8);
  const long long edge_scores = xcd_grid(B, (long long)P * ((N + score_rows - 1) / score_rows)), edge_hop = rows_grid(B, N, P);

  if (train) {
    // sizes the launches cannot express (the maps GEMM takes its row count as an int; the hop grid is the largest), refused
    // here and not behind the maps GEMM
    if ((long long)B * N > kGridMax || edge_hop > kGridMax) return refuse(REFUSE_GRID);
    r.maps = MAPS_F32;
    r.prepare = r.cos_train_note = in.pass == PASS_TRAIN_COS;      // cosine scores = KeyQuery scores of the normalised operands
    r.transpose = true;
    r.scores = GRAPH_EDGE;
    r.k1 = K == 1 ? K1_AFTER_SCORES : K1_NONE;
    r.hop_kind = r.hops ? GRAPH_EDGE : GRAPH_NONE;
  } else {
    const int width = in.concat ? P * F : F;
    if (in.ldy < width || (in.ldy & 3)) return refuse(REFUSE_LDY);
    // X rows are read in 16-byte pieces (the maps GEMMs, the range guard's float32 re-run, the fused bf16 kernels): an X that is
    // not on a 16-byte boundary is refused before anything is launched (magat_hip.h, "Alignment")
    if (!in.x_aligned) return refuse(REFUSE_XALIGN);
    r.fused = fused_form(in);
    r.ws = workspace(in, r.fused);
    if (r.fused) {
      // a workgroup per CU of the instance's XCD at the most; the hop kernel holds two heads' weights, so its workgroups split
      // into P / 2 head groups
      const int per_xcd = in.cus / kXcd > 0 ? in.cus / kXcd : 1;
      const int ng = (N + 31) / 32, nchunk = (ng + kFusedWaves - 1) / kFusedWaves;
      const long long items = xcd_grid(B, nchunk) / kXcd;
      const int ngrp = P >= 2 ? P / 2 : 1, per = per_xcd / ngrp > 0 ? per_xcd / ngrp : 1;
      r.hops = 0;
      r.act_relu = 1;
      r.grid_k1 = 0;
      r.grid_fused_rank = B;
      r.grid_fused_scores = kXcd * (items < per_xcd ? items : per_xcd);
      r.grid_fused_hop = kXcd * ngrp * (items < per ? items : per);
      return r;
    }
    r.maps = cosine ? MAPS_F32 : in.esz == 2 ? MAPS_BF16 : MAPS_AUTO;
    if (r.maps == MAPS_BF16 && ((r.NC % 32) || (G % 32))) r.refusal = REFUSE_BF16_MAPS;      // (with the layout: the workspace check comes first)
    r.prepare = cosine;
    r.act_relu = gnn ? 0 : in.concat;      // GraphFilterBatch has no nonlinearity of its own
    r.head_mean = !in.concat;
    if (K == 1 && (!in.attention || gnn)) {
      r.k1 = K1_ALONE;
    } else {
      r.transpose = r.transpose_booked = K > 1 && !in.have_csc;
      // the tiled score kernel is KeyQuery's; GAT_Similarity keeps the per-edge kernels for scores and hops
      r.scores = gnn ? GRAPH_NONE : (mode == MODE_KEYQUERY && tiled_ok(in, G, 1)) ? GRAPH_TILED : GRAPH_EDGE;
      r.k1 = K == 1 ? K1_AFTER_SCORES : K1_NONE;
      r.hop_kind = !r.hops ? GRAPH_NONE : (!cosine && tiled_ok(in, F, 2)) ? GRAPH_TILED : GRAPH_EDGE;
    }
    r.hop_buffers = K > 3 ? 2 : K > 2 ? 1 : 0;
    if (r.head_mean) {
      const long long blocks = ((long long)B * N * (F / 4) + 255) / 256;
      r.grid_mean = blocks > 4096 ? 4096 : blocks;
    }
  }
  if (r.k1 == K1_NONE) r.grid_k1 = 0;
  if (r.transpose) {
    r.grid_transpose = B;
    r.grid_sort = ((long long)B * N + 3) / 4;
  }
  const long long tiled = xcd_grid(B, P);      // a workgroup per (instance, head)
  r.grid_scores = r.scores == GRAPH_TILED ? tiled : r.scores == GRAPH_EDGE ? edge_scores : 0;
  r.grid_hop = r.hop_kind == GRAPH_TILED ? tiled : r.hop_kind == GRAPH_EDGE ? edge_hop : 0;
  return r;
}

}  // namespace magat_csr
