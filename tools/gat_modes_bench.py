"""GAT layer (maps GEMM + graph kernel) per attention mode at a benchmark shape: per-tag HIP-event times.

    python tools/gat_modes_bench.py [B N [features]]         # default 512 100 128

The four-head rows of the three rank-1 / KeyQuery modes, then KeyQuery and GAT_Similarity with ONE head side by side (the
reference's GAT_Similarity runs with one head only): the cosine mode's extra work is two norms per agent and one multiply per score."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from magat_pathplanning_amd import (GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin,
                                    GraphFilterBatchSimilarityAttentional, _native as nat)
from magat_pathplanning_amd.graphml import gat_forward_rows
from magat_pathplanning_amd.synthetic import comm_gso
B, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (512, 100)
G = int(sys.argv[3]) if len(sys.argv) > 3 else 128
dev = torch.device("cuda:0")
lib = nat.lib()
X = torch.randn(B, N, G, device=dev)
S = comm_gso(B, N, {100: 50, 20: 28, 10: 20}.get(N, 50), seed=1).to(dev)
CLASSES = {"GAT_origin": GraphFilterBatchAttentional_Origin, "GAT_Similarity": GraphFilterBatchSimilarityAttentional}
for mode, P in (("KeyQuery", 4), ("GAT_modified", 4), ("GAT_origin", 4), ("KeyQuery", 1), ("GAT_Similarity", 1)):
    for concat in (True, False):
        cls = CLASSES.get(mode, GraphFilterBatchAttentional)
        layer = cls(G, G, 3, P, concatenate=concat, attentionMode=mode).to(dev).eval()
        with torch.no_grad():
            for _ in range(3):
                gat_forward_rows(X, S, layer)
            lib.magat_profile_reserve(256); lib.magat_profile_reset(); lib.magat_profile_enable(1)
            for _ in range(10):
                gat_forward_rows(X, S, layer)
            torch.cuda.synchronize(); lib.magat_profile_enable(0); lib.magat_profile_collect()
        out, total = [], 0.0
        for tag in (10, 16, 11, 13, 17, 19, 20):
            c, t = ctypes.c_longlong(0), ctypes.c_double(0)
            lib.magat_profile_read(tag, ctypes.byref(c), ctypes.byref(t))
            if c.value:
                out.append("%s %.1f us" % (nat.TAGS[tag], t.value * 1e3 / 10))
                total += t.value * 1e3 / 10
        print("%-14s P=%d %-6s total %.1f us:   %s" % (mode, P, "concat" if concat else "mean", total, "   ".join(out)))
