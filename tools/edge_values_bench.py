"""Times the GSO's values on the edge structure (csrc/gso_edge_values.hip) and the graph side of a GNN step on both routes.

    python tools/edge_values_bench.py [--reps 30] [--rounds 5] [--json out.json]

1. the values launch alone (magat_gso_edge_values behind a finished structure build; device events), both norms;
2. the graph side of a DecentralPlannerNet step - the graph from positions, addGSO, the GraphFilterBatch(128, 128, 3) layer - on the
   tensor route (batched_gso -> (B,N,N) float64 -> dense_gso_to_csr -> layer) against valued edges (structure build -> values ->
   layer), host clock around work that ends in a device synchronise, the two routes alternating round by round in one process.
   The tensor route's code is what it was before the edge route existed, so this is the A/B of the two commits' graph sides.
Sizes: 128 x 100, 8 x 1000, 1 x 2048, 1 x 4096 agents (the tensor route stops at 2048) on distinct random cells of a map with about
12 neighbours per agent at radius 7.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magat_pathplanning_amd import GraphFilterBatch, batched_edges, batched_gso  # noqa: E402

SIZES = ((128, 100), (8, 1000), (1, 2048), (1, 4096))
RADIUS = 7.0


def positions(B, N, dev, seed=0):
    rng = np.random.default_rng(seed + N)
    side = max(int(np.ceil(np.sqrt(N * 13.0))), 8)
    pos = np.zeros((B, N, 2), dtype=np.int32)
    for b in range(B):
        cells = rng.permutation(side * side)[:N]
        pos[b, :, 0], pos[b, :, 1] = cells // side, cells % side
    return torch.from_numpy(pos).to(dev)


def launch_time(pos, sym, reps):
    """ms per magat_gso_edge_values launch, the structure built and counted beforehand"""
    edges = batched_edges(pos, RADIUS, values=True, symmetric_norm=sym)
    st, _, lam = edges.values()
    torch.cuda.synchronize()
    for _ in range(3):
        edges._launch_values(st, True)
    torch.cuda.synchronize()
    stream = st.run
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        edges._launch_values(st, True)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, st.exact_nnz(), float(lam.max())


def step_times(pos, sym, reps, rounds, tensor_route):
    B, N, _ = pos.shape
    dev = pos.device
    layer = GraphFilterBatch(128, 128, 3).to(dev).eval()
    x = torch.randn(B, 128, N, device=dev)
    edges = batched_edges(pos, RADIUS, values=True, symmetric_norm=sym)

    def tensor():
        layer.addGSO(batched_gso(pos, RADIUS, symmetric_norm=sym).unsqueeze(1))
        return layer(x)

    def valued():
        layer.addGSO(edges.refresh())
        return layer(x)

    routes = [("edges", valued)] + ([("tensor", tensor)] if tensor_route else [])
    out = {name: [] for name, _ in routes}
    with torch.no_grad():
        for _, fn in routes:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for name, fn in routes:
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                out[name].append((time.perf_counter() - t0) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_values_bench needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    for B, N in SIZES:
        pos = positions(B, N, dev)
        for sym in (False, True):
            ms, nnz, lam = launch_time(pos, sym, args.reps)
            steps = step_times(pos, sym, args.reps, args.rounds, N <= 2048)
            row = dict(B=B, N=N, symmetric_norm=sym, nnz=nnz, lambda_max=lam, values_launch_ms=ms,
                       edges_step_ms=steps["edges"], tensor_step_ms=steps.get("tensor"))
            rows.append(row)
            med = lambda v: None if v is None else float(np.median(v))      # noqa: E731
            print("%4d x %4d %-14s nnz %8d  values launch %8.3f ms   graph side: edges %8.3f ms  tensor %s ms (medians of %d rounds; "
                  "edges %s tensor %s)" % (B, N, "symmetric_norm" if sym else "plain", nnz, ms, med(steps["edges"]),
                                           "%8.3f" % med(steps["tensor"]) if "tensor" in steps else "     n/a", args.rounds,
                                           ["%.3f" % v for v in steps["edges"]],
                                           ["%.3f" % v for v in steps.get("tensor", [])]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
