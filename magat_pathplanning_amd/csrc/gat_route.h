// Which launches one call of the dense graph layer (magat_gat_forward_*_f32) takes: ONE pure function of the call's scalars, the
// options, one fact about the build and the device's CU count, so that the decision can be checked on a CPU
// (tools/host_wave/gat_route_check.cpp against tests/gat_route_restatement.py).  Every admission condition stands here once.
// Plain C++, no HIP.  gat_f32.hip reads the Route and launches; gat_mfma.hip / gat_small.hip / gat_mid.hip are handed the form
// it decided (OneLaunch) and share the size helpers below.
#pragma once
#include <cstddef>

namespace magat_gat {

// (the values of MAGAT_MODE_* and MAGAT_NUM_XCD: gat_f32.hip asserts that they are)
enum Mode { MODE_KEYQUERY = 0, MODE_GAT_MODIFIED = 1, MODE_GAT_ORIGIN = 2, MODE_GNN = 3, MODE_SIMILARITY = 4 };
constexpr int kXcd = 8;
constexpr size_t kLdsBytes = 160 * 1024;      // LDS of a CU

enum Refusal {
  REFUSE_NONE = 0,
  REFUSE_DIMS = 1,     // a dimension <= 0 (MAGAT_ERR_BAD_SHAPE; the others MAGAT_ERR_UNSUPPORTED)
  REFUSE_MODE = 2,     // not an attention mode of this entry
  REFUSE_SHAPE = 3,    // G != F, a width without kernels, N > 128, GAT_Similarity with more than one head
  REFUSE_TILES = 4     // beyond gat_dense_kernel's LDS tiles and not the one shape gat_mid.hip + gat_slim_kernel serve; answered
                       // behind the checks of ldy, X and the workspace, like before
};
enum Form {
  ONE_MFMA = 0,        // gat_mfma.hip: 128 features, N <= 102
  ONE_SMALL = 1,       // gat_small.hip: 32 / 64 features on graphs of at most 32 agents, a wave per instance
  ONE_MID = 2,         // gat_mid.hip: 32 / 64 features on 33 .. 128 agents, 128 features on 103 .. 128: a workgroup of ceil(N / 32)
                       // waves per instance
  TWO_LAUNCH = 3       // maps GEMM + gat_dense_kernel
};
enum Guard {           // what follows a one-launch form when the range guard is on, every launch predicated on the flag it raises
  GUARD_NONE = 0,
  GUARD_ONE = 1,       // gat_rerun_small_kernel: the whole float32 form as one launch
  GUARD_ONE_TAIL = 2,  // ... with the caller's skinny layer (the action head) in the same launch
  GUARD_TWO = 3,       // float32 maps GEMM + gat_dense_kernel
  GUARD_SLIM = 4       // float32 maps GEMM + gat_slim_kernel (beyond gat_dense_kernel's tiles)
};
enum Maps {
  MAPS_NONE = 0,       // a one-launch form without a chunked re-run: nobody writes Z
  MAPS_SPLIT = 1,      // f16x3 split GEMM
  MAPS_SPLIT_GUARD = 2,  // ... with its own range guard: a predicated float32 GEMM and the one-thread bookkeeping kernel behind it
  MAPS_F32 = 3         // float32 MFMA GEMM (exact products): the re-run, GAT_Similarity, GAT_SPLIT = 0 or a width it cannot tile
};
enum Book {            // which launch moves the guard's flag to status[2], counts the re-run and clears the flag
  BOOK_NONE = 0,
  BOOK_MAPS = 1,       // gat_guard_count_kernel behind the guarded maps GEMM (every chunk)
  BOOK_ONE = 2,        // gat_rerun_small_kernel
  BOOK_GRAPH = 3,      // the graph (or slim) kernel of the last chunk
  BOOK_MEAN = 4        // head_mean_relu_kernel
};

struct RouteOpts {      // the option values, read once per call
  int gat_mfma, gat_split, range_guard, wide_from, gat_pack, chunk_mb;
};

struct RouteIn {
  int B, N, G, F, K, P, mode, concat;
  bool attention;        // the caller wants the attention tensor (A_opt)
  bool y_aligned;        // Y is on a 16-byte boundary
  bool tail;             // a skinny layer was handed over (magat_gat_forward_tail_f32) and magat_skinny_params accepts it ...
  int tail_cout, tail_m, tail_k;      // ... with Cout outputs over M rows of Cin + C2 inputs
  RouteOpts opt;
  bool conv_direct;      // magat_conv_direct_enabled()
  int cus;               // compute units of the current device
};

// the form of a one-launch kernel, decided here and handed to gat_mfma.hip / gat_small.hip / gat_mid.hip
struct OneLaunch {
  int cls;               // ONE_MFMA: shape class (MT, KSI) = 0: (1, 2) N <= 32, 1: (2, 4) N <= 64, 2: (4, 7) N <= 102
  bool pack;             // ONE_MFMA: four instances per pass, one workgroup per pack, every head in it
  bool hsplit;           // ONE_MFMA, ONE_MID: a workgroup per (instance, head)
  bool persist;          // ONE_MFMA: fewer workgroups than units, they walk
  int grid;              // ONE_MFMA: workgroups
  int cus;               // ONE_SMALL, ONE_MID size their grids by it and by their kernels' LDS
};

// ---- sizes -------------------------------------------------------------------------------------------------------------------
// feature widths the graph kernels are instantiated for
inline bool supported_width(int w) { return w == 16 || w == 32 || w == 64 || w == 128 || w == 256; }

// gat_dense_kernel: LDS bytes and workgroup size
inline size_t gat_lds_bytes(int N, int G, int F, int nwaves) {
  const int RW = G > F ? G : F;
  const int lda = N | 1;
  return sizeof(float) * (2 * (size_t)N * RW + (size_t)N * lda + 2 * ((N + 3) & ~3)) +
         sizeof(int) * 128 * (size_t)nwaves + sizeof(unsigned) * 4 * (size_t)N + 16;
}
inline int gat_block_threads(int N) {
  if (N <= 16) return 128;
  if (N <= 32) return 256;
  if (N <= 64) return 512;
  return 1024;
}

// gat_mfma_kernel: LDS bytes of the unpacked forms, and the shape class
inline size_t gat_mfma_lds(int N, int ksi) {
  const size_t sa = 2 * 16 * (size_t)ksi + 16, r8 = ((size_t)N + 7) & ~(size_t)7;
  return 2 * (size_t)N * 256 + 2 * r8 * sa + 2 * 128 * sa;
}
// shape classes: (MT, KSI) = (1, 2) N <= 32, (2, 4) N <= 64, (4, 7) N <= 102 (the LDS bound)
inline int gat_mfma_class(int N) {
  if (N <= 0) return -1;
  const int c = N <= 32 ? 0 : (N <= 64 ? 1 : 2);
  const int ksi = c == 0 ? 2 : (c == 1 ? 4 : 7);
  return (N <= 16 * ksi && gat_mfma_lds(N, ksi) <= kLdsBytes) ? c : -1;
}

// gat_rerun_small_kernel: LDS bytes; the tail's weights (tail_k x 5 floats, 0 = no tail) share the region
inline size_t gat_rerun_small_lds(int N, int G, int tail_k) {
  const size_t own = sizeof(float) * ((size_t)N * (G + 1) + (size_t)N * (N | 1)), w = (size_t)tail_k * 5 * sizeof(float);
  return w > own ? w : own;
}
inline size_t gat_slim_lds(int N) { return sizeof(float) * ((size_t)N * 129 + (size_t)N * (N | 1)); }

// columns of Bt (= of the hoisted maps Z): gat_pack.h's pack_layout(...).NC takes it from here
inline int pack_columns(int G, int F, int K, int P, int mode) {
  if (mode == MODE_KEYQUERY || mode == MODE_SIMILARITY) return P * G + P * K * F;      // (GAT_Similarity: KeyQuery's layout, P = 1)
  if (mode == MODE_GNN) return (P * K * F + 31) & ~31;      // filter taps only
  return (P * K * F + 2 * P + 31) & ~31;   // multiple of 32: the maps GEMM can always use the matrix-core tiles
}
// row stride of the hoisted-map intermediate Z in the dense path: NC + pad.  NC is a multiple of 128 floats at the
// benchmark shapes (2048 -> 8 KB rows): the tiles a workgroup reads are 512-byte row pieces exactly 8 KB apart, which
// all land in the same HBM channels; a 128-byte skew per row spreads them.
constexpr int kZpad = 32;      // row skew of Z (floats)

// instances per chunk: bounds the hoisted-map intermediate Z (chunk*N*ldz floats).  Measured on MI355X
// (c3, B=512): one big launch beats Infinity-Cache-sized chunks (2.02 TB/s vs 1.85 @96 MB vs 1.23 @32 MB),
// so the cap only limits workspace (option GAT_CHUNK_MB, default 2 GiB).
inline int gat_chunk_instances(int B, int N, int ldz, int chunk_mb) {
  long long per = (long long)N * ldz * 4;
  long long c = (long long)((double)chunk_mb * 1048576.0) / (per > 0 ? per : 1);
  if (c < 8) c = 8;
  if (c > B) c = B;
  return (int)c;
}

constexpr long long kRerunSmallUnits = 64;      // instances x heads up to which the re-run is gat_rerun_small_kernel's one launch
constexpr long long kMidHsMaxWg = 64;           // gat_mid.hip: head split while instances x heads stay below this many workgroups
constexpr int kPlanWalkers = 256;               // persistent graph-kernel workgroups (one per CU)

// the maps GEMM on the f16x3 split kernel (option GAT_SPLIT); magat_gat_maps_gemm asks this too, for the CSR layers
inline bool maps_split(int gat_split, int NC, int G) { return gat_split && NC % 32 == 0 && G % 32 == 0; }

// ---- admission of the one-launch kernels ---------------------------------------------------------------------------------------
inline bool taps_ok(int K) { return K == 2 || K == 3; }
inline bool mfma_admits(int N, int G, int F, int K, int mode) {
  return mode >= MODE_KEYQUERY && mode <= MODE_GAT_ORIGIN && G == 128 && F == 128 && taps_ok(K) && gat_mfma_class(N) >= 0;
}
inline bool small_admits(int N, int G, int F, int K, int mode) {
  return (mode == MODE_KEYQUERY || mode == MODE_SIMILARITY) && N >= 1 && N <= 32 && G == F && (G == 32 || G == 64) && taps_ok(K);
}
inline bool mid_admits(int N, int G, int F, int K, int mode, int wide_from) {
  if ((mode != MODE_KEYQUERY && mode != MODE_SIMILARITY) || G != F || !taps_ok(K) || N > 128) return false;
  // GAT_Similarity at 128 features: the XR form where its float32 re-run exists (gat_dense_kernel's tiles end at 105 agents)
  if (G == 128 && mode == MODE_SIMILARITY) return N >= 97 && N <= 105;
  // (gat_mfma.hip up to 102 agents; option GAT_WIDE_FROM: where this form takes over from the two launches.  The kernel itself
  //  runs any N of the four-row-tile class, 97 .. 128)
  if (G == 128) return N >= (wide_from < 103 ? 103 : wide_from);
  return N >= 33 && (G == 32 || G == 64);
}
// the one-launch form of a shape, TWO_LAUNCH when there is none (options GAT_MFMA, GAT_SPLIT).  GAT_Similarity: the cosine forms
// of gat_small.hip (N <= 32) and gat_mid.hip, and only with the range guard on - a row too small for the f16 planes raises its flag
// and is served by the float32 re-run
inline Form one_launch_form(int N, int G, int F, int K, int mode, const RouteOpts& o) {
  if (!o.gat_mfma || !o.gat_split || (mode == MODE_SIMILARITY && o.range_guard == 0)) return TWO_LAUNCH;
  // (128 features: gat_mfma.hip; 32 / 64 features on graphs of at most 32 agents: gat_small.hip; the rest gat_mid.hip - round 6)
  return mfma_admits(N, G, F, K, mode) ? ONE_MFMA : small_admits(N, G, F, K, mode) ? ONE_SMALL
         : mid_admits(N, G, F, K, mode, o.wide_from) ? ONE_MID : TWO_LAUNCH;
}

struct Route {
  Refusal refusal;
  Form form;
  OneLaunch one;
  Guard guard;
  int rerun_grid;        // GUARD_ONE / GUARD_ONE_TAIL: workgroups
  Maps maps;
  bool prepare;          // gat_cos_prepare_kernel behind the maps GEMM (GAT_Similarity)
  bool slim;             // beyond gat_dense_kernel's tiles
  bool ztiles;           // Z in 128-column tiles
  bool all_fused;        // the graph kernel of every chunk merges the heads itself (head mean)
  bool head_mean;        // head_mean_relu_kernel follows the chunks
  Book book;
  int N, P, NC, ldz, chunk, nchunks, threads;      // (N, P: for the per-chunk functions below)
  bool wide_heads;       // G >= 64, P > 1 and tiles that allow one workgroup per CU only: hpb() = P in a chunk that fills the chip
  size_t lds;            // gat_dense_kernel

  bool rerun() const { return guard == GUARD_TWO || guard == GUARD_SLIM; }
  bool chunks() const { return form == TWO_LAUNCH || rerun(); }      // the chunk loop runs
  // heads per workgroup: when the LDS tiles allow only one workgroup per CU there is nothing to overlap a
  // workgroup's loads with, so one workgroup walks all P heads of its instance and prefetches the next head's
  // Q tile during the current head's compute; needs enough instances to fill the chip.
  int hpb(int cb) const { return wide_heads && cb >= 256 ? P : 1; }
  long long zts(int cb) const { return ztiles ? (long long)cb * N * 128 : 0; }
  int inst_slots(int cb) const {
    // with one workgroup per CU (hpb == P case) the grid is capped at one workgroup per CU and every workgroup walks
    // several instances, prefetching across the instance boundary as well
    int s = (cb + kXcd - 1) / kXcd * kXcd;
    if (hpb(cb) == P && P > 1 && s > kPlanWalkers) s = kPlanWalkers;
    // the range guard's predicated re-run: a launch that returns at once still pays for every workgroup it dispatches - with one
    // workgroup per (instance, head) that was 4096 dispatches, 76 us per forward at BASELINE config 2 (1024 instances of 20
    // agents; 88 us of a 1.10 ms step went to the guard).  The workgroups walk the instances instead (istride in the kernel)
    if (rerun() && s > 128) s = 128;
    // (capping the ordinary launches the same way was measured at the published shape - 4096 workgroups of the narrow graph
    //  kernel, 21.7 us: 23 / 32 / 55 us with 512 / 256 / 128 slots - they are not dispatch-bound)
    return s;
  }
  int blocks(int cb) const {
    if (slim) return cb * P < 128 ? cb * P : 128;      // (a no-op launch pays for every workgroup it dispatches)
    return inst_slots(cb) * (P / hpb(cb));
  }
};

inline Route route(const RouteIn& in) {
  const RouteOpts& o = in.opt;
  const int B = in.B, N = in.N, G = in.G, F = in.F, K = in.K, P = in.P, mode = in.mode;
  Route r = {};
  r.form = TWO_LAUNCH;
  if (B <= 0 || N <= 0 || G <= 0 || F <= 0 || K <= 0 || P <= 0) { r.refusal = REFUSE_DIMS; return r; }
  const bool cosine = mode == MODE_SIMILARITY;
  if ((mode < MODE_KEYQUERY || mode > MODE_GAT_ORIGIN) && !cosine) { r.refusal = REFUSE_MODE; return r; }
  if (G != F || !supported_width(G) || N > 128 || (cosine && P != 1)) { r.refusal = REFUSE_SHAPE; return r; }
  r.N = N; r.P = P;
  r.threads = gat_block_threads(N);
  r.lds = gat_lds_bytes(N, G, F, r.threads / 64);
  r.NC = pack_columns(G, F, K, P, mode);
  r.ldz = r.NC + kZpad;
  r.chunk = gat_chunk_instances(B, N, r.ldz, o.chunk_mb);
  r.nchunks = (B + r.chunk - 1) / r.chunk;

  // One launch of matrix-core products when the shape allows.  No attention tensor from these kernels, and they store Y in
  // 16-byte pieces: a column block at an odd offset of a wider buffer takes the two-launch form - or, beyond its tiles, is refused
  const Form one = one_launch_form(N, G, F, K, mode, o);
  if (!in.attention && in.y_aligned) r.form = one;
  // beyond gat_dense_kernel's tiles (128 features: N > 105) only the one-launch form of gat_mid.hip exists, with gat_slim_kernel
  // as the range guard's float32 re-run; no attention tensor there (the CSR kernels serve such requests, and GAT_Similarity)
  r.slim = r.lds > kLdsBytes;
  if (r.slim && !(r.form == ONE_MID && G == 128 && mode == MODE_KEYQUERY)) { r.refusal = REFUSE_TILES; return r; }

  if (r.form == ONE_MFMA) {
    const int cus = in.cus;
    r.one.cls = gat_mfma_class(N);
    // N <= 32: four instances per pass once the batch fills the chip that way (option GAT_PACK, default 1; below that a workgroup
    // per instance - or per (instance, head) - has the shorter critical path: the closed-loop step of a single instance).  Packed
    // and unpacked forms produce the same bits for every instance.
    r.one.pack = r.one.cls == 0 && o.gat_pack && (o.gat_pack >= 2 || (long long)B >= 2LL * cus);
    if (r.one.pack) {
      const int packs = (B + 3) / 4;
      r.one.grid = packs < cus ? packs : cus;
    } else {
      // A workgroup per (instance, head) pays the instance prologue once per head (12 k + 36 k cycles per unit against 12 k + 36 k P
      // per instance), but fills a chip that B instances alone leave idle: the cheaper of the two round counts (head mean: through
      // the caller's scratch rows and magat_gat_mean_launch).
      const long long unsplit = (long long)((B + cus - 1) / cus) * (12 + 36 * P);
      const long long split = (long long)(((long long)B * P + cus - 1) / cus) * (12 + 36);
      r.one.hsplit = P > 1 && split < unsplit;
      const long long units = r.one.hsplit ? (long long)B * P : B, cap = (long long)cus * (r.one.hsplit ? P : 1);
      r.one.grid = (int)(units < cap ? units : cap);
      r.one.persist = units > r.one.grid;
    }
  }
  // gat_mid.hip, few instances (the batch-1 step): a workgroup per (instance, head); head-mean through the caller's scratch rows
  if (r.form == ONE_MID) r.one.hsplit = P > 1 && (long long)B * P <= kMidHsMaxWg;
  r.one.cus = in.cus;

  if (r.form != TWO_LAUNCH) {
    // With the range guard on, a float32 form follows in the same stream, every launch of it predicated on the flag the
    // one-launch kernel raises.
    if (o.range_guard == 0) return r;
    if (mode == MODE_KEYQUERY && (G == 32 || G == 64 || G == 128) && (long long)B * P <= kRerunSmallUnits) {
      // few instances: the whole float32 form as ONE predicated launch (final rows straight into Y, the guard's bookkeeping too),
      // and the layer that reads this one's rows (the action head: five outputs) in the same launch, when the caller handed it over
      const bool with_tail = in.tail && in.tail_cout == 5 && in.tail_m == B * N && (size_t)in.tail_k * 5 * sizeof(float) <= 64 * 1024;
      r.guard = with_tail ? GUARD_ONE_TAIL : GUARD_ONE;
      const int tg = (B * N + 15) / 16;      // (B x heads <= 64, N <= 128: at most 512 workgroups)
      r.rerun_grid = with_tail && tg > B ? tg : B;
      r.book = BOOK_ONE;
      return r;
    }
    r.guard = r.slim ? GUARD_SLIM : GUARD_TWO;
  }

  // The chunk loop: maps GEMM, gat_cos_prepare_kernel for GAT_Similarity, graph kernel.
  // GAT_Similarity: float32 MFMA maps - an agent whose features are tiny, |x| ~ 1e-12, is zero in f16 planes, and so would be
  // its q_j, whose DIRECTION is what the cosine score reads; nothing to guard then
  r.maps = r.rerun() || cosine || !maps_split(o.gat_split, r.NC, G) ? MAPS_F32 : o.range_guard != 0 ? MAPS_SPLIT_GUARD : MAPS_SPLIT;
  r.prepare = cosine;
  // Z in 128-column tiles ([tile][cb * N][128]: an instance's Q_p / U_pk tile is ONE contiguous N x 128 run for the
  // LDS-direct loads, and every workgroup of the maps GEMM writes one contiguous region) when the dense kernel with
  // 128-wide features consumes it and the f16x3 direct GEMM produces it.
  r.ztiles = G == 128 && F == 128 && r.NC % 128 == 0 && in.conv_direct && o.gat_split;
  r.wide_heads = G >= 64 && P > 1 && r.lds > 80 * 1024;
  // mean merge fused into the graph kernel when one workgroup sees all heads of an instance (decided for the whole
  // call: every chunk must qualify, otherwise the separate kernel merges everything from Ytmp)
  r.all_fused = !in.concat && G >= 64 && !r.slim;
  for (int b0 = 0; b0 < B && r.all_fused; b0 += r.chunk) r.all_fused = r.hpb(B - b0 < r.chunk ? B - b0 : r.chunk) == P;
  r.head_mean = !in.concat && !r.all_fused;
  // the re-run's last launch does the guard's bookkeeping: the graph kernel of the last chunk, or the head-mean kernel
  // (one chunk is the rule; with several, a clamp in an earlier chunk leaves the flag set only until the next chunk's
  // own GEMM clears it - status[1] still counts every re-run)
  r.book = r.rerun() ? (r.head_mean ? BOOK_MEAN : BOOK_GRAPH) : r.maps == MAPS_SPLIT_GUARD ? BOOK_MAPS : BOOK_NONE;
  return r;
}

}  // namespace magat_gat
