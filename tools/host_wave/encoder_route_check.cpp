// The encoder's route function and pack constants on the host (tests/test_host_encoder_route.py).
//   encoder_route_check < grid.txt
// Prints "const NAME VALUE" for every slot and scale-block constant of csrc/encoder_pack.h, then, for every line of stdin
// (the 36 integers of a magat_enc::RouteIn in declaration order), one line with the 15 integers of the Route in declaration order.
#include <cstdio>

#include "../../magat_pathplanning_amd/csrc/encoder_pack.h"
#include "../../magat_pathplanning_amd/csrc/encoder_route.h"

namespace enc = magat_enc;

int main() {
#define CONST(name, value) std::printf("const %s %d\n", name, (int)(value))
  CONST("STEM_W", enc::STEM_W); CONST("STEM_B", enc::STEM_B);
  for (int l = 0; l < 3; ++l) {
    char nm[32];
    std::snprintf(nm, sizeof nm, "conv1_w(%d)", l); CONST(nm, enc::conv1_w(l));
    std::snprintf(nm, sizeof nm, "conv1_b(%d)", l); CONST(nm, enc::conv1_b(l));
    std::snprintf(nm, sizeof nm, "conv2_w(%d)", l); CONST(nm, enc::conv2_w(l));
    std::snprintf(nm, sizeof nm, "conv2_b(%d)", l); CONST(nm, enc::conv2_b(l));
    std::snprintf(nm, sizeof nm, "conv1_f16(%d)", l); CONST(nm, enc::conv1_f16(l));
    std::snprintf(nm, sizeof nm, "conv2_f16(%d)", l); CONST(nm, enc::conv2_f16(l));
  }
  for (int i = 0; i < 4; ++i) {
    char nm[32];
    std::snprintf(nm, sizeof nm, "plain_w(%d)", i); CONST(nm, enc::plain_w(i));
    std::snprintf(nm, sizeof nm, "plain_b(%d)", i); CONST(nm, enc::plain_b(i));
  }
  CONST("HEAD_W", enc::HEAD_W); CONST("HEAD_B", enc::HEAD_B); CONST("COMP_W", enc::COMP_W); CONST("COMP_B", enc::COMP_B);
  CONST("F32_SLOTS", enc::F32_SLOTS); CONST("PERMUTED", enc::PERMUTED); CONST("TILE16", enc::TILE16); CONST("SLOTS", enc::SLOTS);
  CONST("SC_W0", enc::SC_W0); CONST("SC_B0", enc::SC_B0); CONST("SC_B1", enc::SC_B1); CONST("SC_BA", enc::SC_BA);
  CONST("SC_BB", enc::SC_BB); CONST("SC_BC", enc::SC_BC); CONST("SC_B31", enc::SC_B31); CONST("SC_B32", enc::SC_B32);
  CONST("SC_SCALES", enc::SC_SCALES); CONST("SC_HEAD_IN", enc::SC_HEAD_IN); CONST("SC_FEAT_IN", enc::SC_FEAT_IN);
  CONST("SC_FLOATS", enc::SC_FLOATS);
  CONST("permuted_behind(32,288)", enc::permuted_behind(32, 288));
  std::printf("routes\n");
  long long v[36];
  for (;;) {
    for (int i = 0; i < 36; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
    enc::RouteIn in = {};
    int k = 0;
    in.variant = (int)v[k++]; in.H = (int)v[k++]; in.W = (int)v[k++]; in.n_feat = (int)v[k++]; in.n_comp = (int)v[k++];
    in.form_agents = (int)v[k++];
    for (int l = 0; l < 3; ++l) in.f16[l] = v[k++] != 0;
    in.permuted = v[k++] != 0;
    in.chain = v[k++] != 0; in.chain3 = v[k++] != 0; in.head16 = v[k++] != 0; in.comp16 = v[k++] != 0; in.scaled = v[k++] != 0;
    in.l1frag = v[k++] != 0; in.headfrag = v[k++] != 0; in.compfrag = v[k++] != 0;
    in.comp = v[k++] != 0; in.comp_bf16 = v[k++] != 0;
    in.M = (int)v[k++]; in.mm = (int)v[k++];
    in.pass = (enc::Pass)v[k++];
    in.opt.conv_split = (int)v[k++]; in.opt.range_guard = (int)v[k++]; in.opt.conv_pchain = (int)v[k++];
    in.opt.l1_fused = (int)v[k++]; in.opt.block_fused = (int)v[k++]; in.opt.head_splitk = (int)v[k++];
    in.opt.head_f16 = (int)v[k++]; in.opt.head_compress = (int)v[k++]; in.opt.lat_agents = (int)v[k++];
    in.conv_direct = v[k++] != 0; in.l1_lds = v[k++] != 0; in.full_out_gl = v[k++] != 0;
    in.buf_floats = (size_t)v[k++];
    const enc::Route r = enc::route(in);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", r.split, r.Mform, r.lay, (int)r.stem, (int)r.chain,
                r.first_loop_block, (int)r.pooled, (int)r.scaled_chain, (int)r.head, (int)r.head_gl, (int)r.comp_epilogue,
                (int)r.comp, (int)r.guard, (int)r.bf16, (int)r.bf16_after_guard);
  }
}
