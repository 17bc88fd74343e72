// The encoder pack's format, named once: the slots of magat_encoder_desc.off[] (encoder.fold_resnet, fold_default_cnn,
// fold_dilated_cnn write them), the layout of the activation-scale block behind magat_encoder_desc.scaled_off
// (encoder.fold_activation_scales), and the one resolver that turns (pack, off, scaled_off) into the pointers the fused path hands
// to its kernels.  Plain C++, no HIP: tools/host_wave/encoder_route_check.cpp prints these constants and
// tests/test_host_encoder_route.py holds them against encoder.py's.
#pragma once
#include <cstdint>

namespace magat_enc {

// ---- slots of off[] (float offsets into the pack) ----
constexpr int STEM_W = 0, STEM_B = 1;                        // conv1 [32][27] (BN folded), bias [32]
constexpr int conv1_w(int l) { return 2 + 4 * l; }           // BasicBlock l = 0..2: conv1 [Cout][9 Cin]
constexpr int conv1_b(int l) { return 3 + 4 * l; }
constexpr int conv2_w(int l) { return 4 + 4 * l; }           // [conv2 | downsample] [Cout][9 Cout + Cin]
constexpr int conv2_b(int l) { return 5 + 4 * l; }           // bias_conv2 + bias_down
constexpr int HEAD_W = 14, HEAD_B = 15;                      // fc (+ Flatten + Linear) folded, x 1/4 of AvgPool2d(2)
constexpr int COMP_W = 16, COMP_B = 17;                      // compressMLP
constexpr int F32_SLOTS = 18;                                // slots 0 .. 17: the float32 BN-folded weights (the latency guard reads them)
constexpr int conv1_f16(int l) { return 24 + 2 * l; }        // the same two weights as f16x2 planes + 2^-e (in_fmt 4); 18 .. 23 are empty
constexpr int conv2_f16(int l) { return 25 + 2 * l; }
constexpr int PERMUTED = 30;                                 // first K-permuted copy of those planes; non-zero = the copies are there
constexpr int TILE16 = 31;                                   // layer3.conv2 in 16-row fragments (encoder.pack_block3_tile16)
constexpr int SLOTS = 32;
// the plain CNNs (variants 2, 3, 4): conv i + 1, i = 0 .. 3; stem, HEAD_W (an identity) and compressMLP as above
constexpr int plain_w(int i) { return 2 + 2 * i; }
constexpr int plain_b(int i) { return 3 + 2 * i; }

// ---- the activation-scale block (floats from pack + scaled_off; magat_hip.h "Activation scales") ----
constexpr int SC_W0 = 0;          // stem weights x 2^s1 [864]
constexpr int SC_B0 = 864;        // stem bias [32]
constexpr int SC_B1 = 896;        // layer1.conv1 bias [32]
constexpr int SC_BA = 928;        // layer1.conv2 + downsample [32]
constexpr int SC_BB = 960;        // layer2.conv1 [64]
constexpr int SC_BC = 1024;       // layer2.conv2 + downsample [64]
constexpr int SC_B31 = 1088;      // layer3.conv1 [128]
constexpr int SC_B32 = 1216;      // layer3.conv2 + downsample [128]
constexpr int SC_SCALES = 1344;   // sA' sB' sC' s31' s32': the five 1 / weight-scale floats with the scale ratios folded in
constexpr int SC_HEAD_IN = 1349;  // in_scale of the head's float32 loader
constexpr int SC_FEAT_IN = 1350;  // ... and of compressMLP's
constexpr int SC_FLOATS = 1352;

// float offset of the K-permuted copy behind an f16 weight block of cout x ktot weights (two planes + one scale float, padded to 4
// floats)
constexpr int64_t permuted_behind(int cout, int ktot) { return ((int64_t)cout * ktot + 1 + 3) & ~(int64_t)3; }

// What the fused path's kernels are handed.  scaled_off > 0: the head's and compressMLP's in_scale come from the block.  The stem's
// and the chain's operands come from it as well when `scaled_chain` (the whole chain in two launches - the path the scales are
// folded for; magat_encoder_stem_block_f32 - every stem of a scaled pack); from the plain pack slots otherwise.
struct FusedPtrs {
  const float* w0; const float* b0; const float* b1;                            // stem weight, bias; layer1.conv1 bias
  const float* bA; const float* bB; const float* bC; const float* b31; const float* b32;      // the chain's biases
  const float* scales;                // the five epilogue scales, or null (each weight block's own 1 / scale then)
  const float* head_in; const float* comp_in;      // in_scale pointers, or null
};

inline FusedPtrs resolve(const float* pack, const int64_t* off, int64_t scaled_off, bool scaled_chain) {
  const float* sp = scaled_off > 0 ? pack + scaled_off : nullptr;
  const float* sc = scaled_chain ? sp : nullptr;
  FusedPtrs p;
  p.w0 = sc ? sc + SC_W0 : pack + off[STEM_W];
  p.b0 = sc ? sc + SC_B0 : pack + off[STEM_B];
  p.b1 = sc ? sc + SC_B1 : pack + off[conv1_b(0)];
  p.bA = sc ? sc + SC_BA : pack + off[conv2_b(0)];
  p.bB = sc ? sc + SC_BB : pack + off[conv1_b(1)];
  p.bC = sc ? sc + SC_BC : pack + off[conv2_b(1)];
  p.b31 = sc ? sc + SC_B31 : pack + off[conv1_b(2)];
  p.b32 = sc ? sc + SC_B32 : pack + off[conv2_b(2)];
  p.scales = sc ? sc + SC_SCALES : nullptr;
  p.head_in = sp ? sp + SC_HEAD_IN : nullptr;
  p.comp_in = sp ? sp + SC_FEAT_IN : nullptr;
  return p;
}

}  // namespace magat_enc
