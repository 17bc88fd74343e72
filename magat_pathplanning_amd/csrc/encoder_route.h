// Which kernel forms one chunk of a ResNet-encoder pass (variant 0 / 1) takes: ONE pure function of the descriptor's scalars, the
// pass, the options and three facts about the build, so that the decision can be checked on a CPU
// (tools/host_wave/encoder_route_check.cpp against tests/encoder_route_restatement.py).  Every admission condition stands here
// once.  Plain C++, no HIP.  Only encoder_f32.hip includes it: it reads the Route and launches.
#pragma once
#include <cstddef>

namespace magat_enc {

enum Pass { PASS_FORWARD = 0, PASS_RERUN = 1, PASS_CALIBRATE = 2 };      // split arithmetic; the guard's predicated float32 re-run; absmax
enum Stem {
  STEM_PLAIN = 0,      // conv_first_kernel, then layer1.conv1 as a launch of its own
  STEM_BAND = 1,       // stem + layer1.conv1 as one kernel, 64-agent row bands (layer1_fused.hip)
  STEM_8 = 2,          // ... eight-agent groups (stem8.hip; 11 x 11 maps)
  STEM_LAT = 3         // inside the latency kernel (block_lat.hip): no launch of its own
};
enum Chain {
  CHAIN_LAYERS = 0,    // one launch per convolution
  CHAIN_TWO = 1,       // layer1.conv2 + layer2; then layer3 + pool when the trunk and the pack have it
  CHAIN_ONE = 2,       // layer1.conv2 -> layer2 -> layer3 -> pool, eight agents per workgroup (block_fused.hip)
  CHAIN_LAT = 3        // ... one agent per workgroup (block_lat.hip)
};
enum Head {
  HEAD_F32 = 0,        // float32 MFMA (in the re-run: one more layer of its chained launch)
  HEAD_SPLITK = 1,     // K split by pooled cell on the float32 kernel + a fixed-order sum
  HEAD_LONGK = 2,      // f16x3 split products over the pooled map
  HEAD_LAT = 3         // in the latency kernel's epilogue, compressMLP behind it
};
enum Comp {
  COMP_NONE = 0,       // no compressMLP (n_comp = 0)
  COMP_F32 = 1,        // float32 MFMA, a launch of its own
  COMP_CHAINED = 2,    // one more layer of the re-run's chained launch
  COMP_F16 = 3,        // f16x3 split products, a launch of its own
  COMP_LAT = 4         // in the latency kernel's epilogue
};
enum Guard { GUARD_NONE = 0, GUARD_LAT = 1, GUARD_RERUN = 2 };      // nobody; the latency kernel itself; a predicated re-run
enum Bf16 {
  BF16_NONE = 0,
  BF16_CAST = 1,       // one cast pass over the chunk's rows
  BF16_EPILOGUE = 2    // by the head's epilogue together with comp (a cast pass when the kernel declines)
};

struct RouteOpts {      // the option values, read once per call
  int conv_split, range_guard, conv_pchain, l1_fused, block_fused, head_splitk, head_f16, head_compress, lat_agents;
};

struct RouteIn {
  int variant, H, W, n_feat, n_comp, form_agents;
  bool f16[3];           // BasicBlock l + 1 has both of its f16 weight planes
  bool permuted;         // ... and the pack their K-permuted copies
  bool chain, chain3, head16, comp16, scaled, l1frag, headfrag, compfrag;      // the descriptor's *_off fields are non-zero
  bool comp, comp_bf16;  // the caller passed comp / desc.comp_bf16
  int M, mm;             // agents of the call, of this chunk
  Pass pass;
  RouteOpts opt;
  bool conv_direct, l1_lds, full_out_gl;      // magat_conv_direct_enabled(), magat_layer1_fused_lds(W) != 0, magat_block_full_out_gl()
  size_t buf_floats;     // floats per agent of one activation buffer (the split-K head's partial sums must fit one)
};

struct Route {
  int split;             // bit l: BasicBlock l + 1 on the split-MFMA kernels
  int Mform;             // the agent count the batch-size-dependent forms are chosen on
  int lay;               // activations between the layers: 0 row-major, 1 float32 granules, 2 f16 plane granules
  Stem stem;
  Chain chain;
  int first_loop_block;  // first BasicBlock left to the layer-by-layer loop
  bool pooled;           // the head's input is the 2 x 2-pooled map (else it pools on load)
  bool scaled_chain;     // stem and chain read the activation-scale block
  Head head;
  bool head_gl;          // the pooled map goes to the head granule-major
  bool comp_epilogue;    // compressMLP is attempted in the head's epilogue; `comp` follows when the kernel declines
  Comp comp;
  Guard guard;
  Bf16 bf16;             // where this chunk's bf16 rows come from ...
  bool bf16_after_guard; // ... and whether a cast predicated on the forward's flag follows the guard
};

// desc.comp_bf16 is served (also by the plain CNNs, which have no Route)
inline bool bf16_rows_wanted(bool comp_bf16, int n_comp) { return comp_bf16 && n_comp > 0 && (n_comp & 3) == 0; }

inline Route route(const RouteIn& in) {
  const RouteOpts& o = in.opt;
  Route r = {};
  const bool rerun = in.pass == PASS_RERUN, fwd = in.pass == PASS_FORWARD;
  const int nblocks = in.variant == 0 ? 3 : 2;
  const int clast = in.variant == 0 ? 128 : 64;
  const int Ho = (in.H + 2 - 3) / 2 + 1, Wo = (in.W + 2 - 3) / 2 + 1;
  const int cells = (Ho / 2) * (Wo / 2);
  // Block convolutions on the split-MFMA kernels (option CONV_SPLIT = bit mask, bit l = layer l + 1; default 7 = all three; 0 keeps
  // every layer on the fp32 MFMA kernel): a layer is in the mask only when the pack carries its f16 weight planes.  The re-run
  // and the calibration pass are float32 throughout.
  if (fwd)
    for (int l = 0; l < 3; ++l)
      if ((o.conv_split >> l & 1) && in.f16[l]) r.split |= 1 << l;
  // (the agent count the forms are chosen on: the whole call's, or - a shard of a larger batch - the global one)
  r.Mform = in.form_agents > 0 ? in.form_agents : in.M;

  // Granule-major activation tiles between the layers when every BasicBlock conv runs on the f16x3 direct kernel; as f16 PLANE
  // granules when the pack carries the K-permuted weight copies (option CONV_PCHAIN = 0 keeps float32 granules).
  const bool gl = r.split == (1 << nblocks) - 1 && in.conv_direct;
  r.lay = !gl ? 0 : (in.permuted && o.conv_pchain) ? 2 : 1;

  // Stem + layer1.conv1 as ONE kernel (option L1_FUSED = 0 keeps the two launches), in eight-agent groups when the map is 11 x 11
  // and the pack holds layer1.conv1 fragment-major (L1_FUSED = 2, the default)
  const bool fused1 = r.lay == 2 && in.l1_lds && o.l1_fused != 0;
  const bool stem8 = fused1 && in.H == 11 && in.W == 11 && in.l1frag && o.l1_fused >= 2;
  // BasicBlock chain kernel (block_fused.hip): layer1.conv2+downsample -> layer2.conv1 -> layer2.conv2+downsample in one
  // launch with the 6x6 maps of an 8-agent group in LDS (3.35 GB of HBM traffic per 51 200 agents become 0.94 GB).
  // Needs the fused stem's plane-granule outputs; option BLOCK_FUSED=0 keeps the layer-by-layer kernels, 2 (the default) makes
  // both chain kernels ONE launch: layer2's output map stays in LDS as layer3's input - the path the activation scales are
  // folded for.
  const bool chain2 = fused1 && in.chain && Ho == 6 && Wo == 6 && nblocks >= 2 && o.block_fused != 0;
  const bool full = chain2 && nblocks == 3 && in.chain3 && o.block_fused >= 2;
  // Latency form of the few agents of a batch-1 step (option LAT_AGENTS, chosen on the global agent count like the head's
  // form): one agent per workgroup (block_lat.hip: the same pooled map bit for bit, 2 460 instead of 13 428 matrix instructions
  // deep) ...
  const bool lat = full && !rerun && r.Mform <= o.lat_agents;
  // ... which then runs the encoder head and compressMLP in its epilogue as well (ABI 8 fragment-major weights): the products
  // of the long-K f16x3 head and of the f16x3 compressMLP in their order - feat / comp bit-identical to the batched forms ...
  const bool lat_head = lat && in.headfrag && in.compfrag && in.n_feat == 128 &&
                        (in.n_comp == 128 || in.n_comp == 64 || in.n_comp == 32) && in.comp && r.split && o.head_f16;
  // ... and then takes the stem along as well, when the call is one chunk
  const bool lat_stem = lat_head && stem8 && in.mm == in.M;

  r.stem = lat_stem ? STEM_LAT : stem8 ? STEM_8 : fused1 ? STEM_BAND : STEM_PLAIN;
  r.chain = lat ? CHAIN_LAT : full ? CHAIN_ONE : chain2 ? CHAIN_TWO : CHAIN_LAYERS;
  r.scaled_chain = full && in.scaled;
  const bool block3 = chain2 && nblocks == 3 && in.chain3;      // layer3 + ReLU + AvgPool2d(2) as a chain kernel
  r.first_loop_block = full ? 3 : chain2 ? (block3 ? 3 : 2) : 0;
  r.pooled = full || block3;

  // Head.  Few agents: K split by pooled cell (option HEAD_SPLITK = largest agent count that takes this form, 0 = never) - the
  // count of the whole call, not of the chunk: the short last chunk of a 70 100-agent batch must sum in the same order as its
  // other chunks, or the batch would differ in the last bit from the same agents presented as shards.  The partials must fit one
  // map buffer.
  const bool splitk = in.pass == PASS_FORWARD && cells > 1 && r.Mform <= o.head_splitk && (clast & 3) == 0 &&
                      (in.n_feat & 3) == 0 && (size_t)cells * in.n_feat <= in.buf_floats;
  // Many agents, pooled input: f16x3 split products like the blocks
  const bool longk = r.pooled && r.split && in.head16 && (clast % 32) == 0 && (in.n_feat % 32) == 0 && o.head_f16;
  r.head = lat_head ? HEAD_LAT : splitk ? HEAD_SPLITK : longk ? HEAD_LONGK : HEAD_F32;
  // The pooled map goes to the head granule-major ([cell][128 / 4][128 agents][4 floats]) when the head is the f16x3 direct
  // GEMM: its loader then reads 512 contiguous bytes per half wave instead of 32 bytes out of every agent's 512-byte row, and
  // the chain kernel stores 128-byte runs instead of 16-byte pieces.  (Not for the few-agent form of the head, which splits K
  // by pooled cell on the float32 kernel.  Decided on the forms the head takes outside the latency kernel.)
  r.head_gl = full && !splitk && longk && in.conv_direct && in.full_out_gl;

  // compressMLP in the long-K head's epilogue (round 5; option HEAD_COMPRESS): the 128-wide feature rows are complete in the
  // workgroup's registers, so the second layer runs on them there - one launch instead of two, bit for bit the same comp.  The
  // kernel declines when CONV_BNFILL narrowed the head's column tile for a small batch.  Else f16x3 split products on the direct
  // kernel when the head's input was pooled (large pooled batches), else float32 MFMA (and always in the guard's re-run)
  r.comp_epilogue = r.head == HEAD_LONGK && in.comp && in.n_comp == 128 && in.n_feat == 128 && in.comp16 && o.head_compress;
  const bool comp_f16 = !rerun && r.pooled && r.split && in.comp16 && (in.n_feat % 32) == 0 && (in.n_comp % 32) == 0 && o.head_f16;
  r.comp = in.n_comp <= 0 ? COMP_NONE : lat_head ? COMP_LAT : comp_f16 ? COMP_F16 : rerun ? COMP_CHAINED : COMP_F32;

  // Range guard (forward pass with split arithmetic, option RANGE_GUARD): inside the latency kernel when that runs the head of
  // the whole call on an 11 x 11 map - a workgroup whose planes clamped (or the stem's did) recomputes its agent in float32 from
  // the raw state maps, the last workgroup does the guard's bookkeeping, no predicated launches behind it - else a predicated
  // float32 re-run
  const bool guarded = fwd && r.split != 0 && o.range_guard != 0;
  r.guard = !guarded ? GUARD_NONE : (lat_head && in.mm == in.M && in.H == 11 && in.W == 11) ? GUARD_LAT : GUARD_RERUN;

  // bf16 rows (ABI 7): the re-run and the calibration pass leave them to their callers
  const bool rows = fwd && bf16_rows_wanted(in.comp_bf16, in.n_comp);
  r.bf16 = !rows ? BF16_NONE : r.comp_epilogue ? BF16_EPILOGUE : BF16_CAST;
  r.bf16_after_guard = rows && r.guard != GUARD_NONE;
  return r;
}

}  // namespace magat_enc
