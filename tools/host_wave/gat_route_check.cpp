// The dense graph layer's route function on the host (tests/test_host_gat_route.py).
//   gat_route_check < grid.txt
// For every line of stdin (the 22 integers of a magat_gat::RouteIn in declaration order) one line: the refusal, and for an
// admitted call the Route's fields in declaration order (N and P left out), then cb, hpb, inst_slots, blocks and zts of the
// first and of the last chunk.
#include <cstdio>

#include "../../magat_pathplanning_amd/csrc/gat_route.h"

namespace gr = magat_gat;

int main() {
  long long v[22];
  for (;;) {
    for (int i = 0; i < 22; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
    gr::RouteIn in = {};
    int k = 0;
    in.B = (int)v[k++]; in.N = (int)v[k++]; in.G = (int)v[k++]; in.F = (int)v[k++]; in.K = (int)v[k++]; in.P = (int)v[k++];
    in.mode = (int)v[k++]; in.concat = (int)v[k++];
    in.attention = v[k++] != 0; in.y_aligned = v[k++] != 0; in.tail = v[k++] != 0;
    in.tail_cout = (int)v[k++]; in.tail_m = (int)v[k++]; in.tail_k = (int)v[k++];
    in.opt.gat_mfma = (int)v[k++]; in.opt.gat_split = (int)v[k++]; in.opt.range_guard = (int)v[k++];
    in.opt.wide_from = (int)v[k++]; in.opt.gat_pack = (int)v[k++]; in.opt.chunk_mb = (int)v[k++];
    in.conv_direct = v[k++] != 0; in.cus = (int)v[k++];
    const gr::Route r = gr::route(in);
    if (r.refusal != gr::REFUSE_NONE) {
      std::printf("%d\n", (int)r.refusal);
      continue;
    }
    std::printf("0 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu", (int)r.form, r.one.cls, (int)r.one.pack,
                (int)r.one.hsplit, (int)r.one.persist, r.one.grid, (int)r.guard, r.rerun_grid, (int)r.maps, (int)r.prepare,
                (int)r.slim, (int)r.ztiles, (int)r.all_fused, (int)r.head_mean, (int)r.book, r.NC, r.ldz, r.chunk, r.nchunks,
                r.threads, r.lds);
    const int cbs[2] = {in.B < r.chunk ? in.B : r.chunk, in.B - (r.nchunks - 1) * r.chunk};
    for (int cb : cbs) std::printf(" %d %d %d %d %lld", cb, r.hpb(cb), r.inst_slots(cb), r.blocks(cb), r.zts(cb));
    std::printf("\n");
  }
}
