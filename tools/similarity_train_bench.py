"""One training step (forward + backward) of the GAT_Similarity layer on the device: the torch composite against the HIP training
kernels (GraphFilterBatchSimilarityAttentional(hip_backward=True)).  Needs a GPU.

    python tools/similarity_train_bench.py [--out table.md]

The two paths alternate in one process: 5 warm-ups each, then 20 timed steps each, interleaved, every step closed by a device
synchronisation; the median is reported.  Peak memory: torch.cuda.max_memory_allocated over the timed steps of a path, above what
was allocated before them (inputs, parameters, the GSO).  No time here is a gate; DESIGN.md section 4.6 holds the table.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magat_pathplanning_amd import GraphFilterBatchSimilarityAttentional  # noqa: E402
from magat_pathplanning_amd.synthetic import comm_gso  # noqa: E402

SHAPES = [(64, 10, 32), (64, 100, 32), (64, 100, 128), (16, 300, 64)]      # (B, N, G)
K, WARMUP, STEPS = 3, 5, 20


def step(layer, x, wgt):
    layer.zero_grad(set_to_none=True)
    x.grad = None
    (layer(x) * wgt).sum().backward()
    torch.cuda.synchronize()


def measure(B, N, G, dev):
    torch.manual_seed(B + N + G)
    base = GraphFilterBatchSimilarityAttentional(G, G, K, 1)
    layers = {}
    for name, hip in (("composite", False), ("hip", True)):
        layer = GraphFilterBatchSimilarityAttentional(G, G, K, 1, hip_backward=hip)
        layer.load_state_dict(base.state_dict())
        layers[name] = layer.to(dev).train()
    S = comm_gso(B, N, max(6, int(4 * N ** 0.5)), seed=N).unsqueeze(1).to(dev)
    for layer in layers.values():
        layer.addGSO(S)
    g = torch.Generator().manual_seed(N)
    x = (torch.randn(B, G, N, generator=g) * 0.6).to(dev).requires_grad_(True)
    wgt = torch.randn(B, G, N, generator=g).to(dev)
    for _ in range(WARMUP):
        for layer in layers.values():
            step(layer, x, wgt)
    times, peak = {n: [] for n in layers}, {n: 0 for n in layers}
    for _ in range(STEPS):
        for name, layer in layers.items():
            torch.cuda.synchronize()
            base_mem = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            step(layer, x, wgt)
            times[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated(dev) - base_mem)
    return {n: {"ms": statistics.median(times[n]), "peak_mb": peak[n] / 2 ** 20} for n in layers}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table (markdown) and the figures (JSON lines) to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["| B x N, G (K = %d) | composite ms | HIP ms | composite peak MB | HIP peak MB |" % K, "|---|---|---|---|---|"]
    rows = []
    for B, N, G in SHAPES:
        r = measure(B, N, G, dev)
        rows.append({"B": B, "N": N, "G": G, **{"%s_%s" % (n, k): round(v, 3) for n, d in r.items() for k, v in d.items()}})
        lines.append("| %d x %d, %d | %.3f | %.3f | %.1f | %.1f |" % (B, N, G, r["composite"]["ms"], r["hip"]["ms"],
                                                                 r["composite"]["peak_mb"], r["hip"]["peak_mb"]))
    text = "\n".join(lines) + "\n" + "\n".join(json.dumps(r) for r in rows) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
