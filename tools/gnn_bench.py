"""Timings of the bottleneck GNN planners' graph layer and forward (device events after warm-up; needs a GPU).

    python tools/gnn_bench.py [--reps 50] [--out profiles/<dir>/gnn_bench.json]

  layer    GraphFilterBatch at 1 x 10, 64 x 10 and 512 x 100 agents, G = F in {32, 128}, K = 3, float64 GSO: the dense one-launch
           kernel (magat_gnn_forward_dense_f32, ReLU fused) against the CSR route (GraphFilterBatch._forward_hip: GSO -> CSR
           with its host synchronisation, value gather, CSR kernels)
  forward  DecentralPlannerBottleneckNet addGSO + forward (BottomNeck_skipConcat, ResNetLarge_withMLP, bottleneck 32 | 128)
  step     the batch-1 step (1 x 10 agents): eager against the replay of a captured torch.cuda.CUDAGraph
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magat_pathplanning_amd import DecentralPlannerBottleneckNet, GraphFilterBatch  # noqa: E402
from magat_pathplanning_amd import _native as nat  # noqa: E402
from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config  # noqa: E402


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps       # us per call


def layer_rows(reps, dev):
    out = []
    for (B, N) in ((1, 10), (64, 10), (512, 100)):
        for G in (32, 128):
            F, K = G, 3
            torch.manual_seed(0)
            layer = GraphFilterBatch(G, F, K).to(dev).eval()
            S = comm_gso(B, N, max(8, int(2.2 * N ** 0.5 * 4)), seed=1, dtype=torch.float64).to(dev)
            X = torch.randn(B * N, G, device=dev)
            Y = torch.empty(B * N, F, device=dev)
            w, b = layer.weight.detach().contiguous(), layer.bias.detach().contiguous()
            stream = nat.current_stream(dev)

            def dense():
                nat.check(nat.lib().magat_gnn_forward_dense_f32(nat.ptr(X), G, nat.ptr(S), 1, nat.ptr(w), nat.ptr(b), nat.ptr(Y), F,
                                                                B, N, N, G, F, K, 1, stream), "magat_gnn_forward_dense_f32")

            xg = X.view(B, N, G).permute(0, 2, 1)
            layer.addGSO(S.unsqueeze(1))

            def csr():
                torch.relu_(layer._forward_hip(xg)[0])

            with torch.no_grad():
                td, tc = timed(dense, reps), timed(csr, reps)
            s_bytes, flop = S.numel() * 8 * (F // 32 if F >= 32 else 1), 2 * B * (K * N * G * F + (K - 1) * N * N * F)
            out.append(dict(leg="layer", B=B, N=N, G=G, F=F, K=K, dense_us=round(td, 2), csr_us=round(tc, 2),
                            speedup=round(tc / td, 2), s_bytes=s_bytes, flop=flop))
            print(json.dumps(out[-1]), flush=True)
    return out


def forward_rows(reps, dev):
    out = []
    for bf in (32, 128):
        for (B, N) in ((1, 10), (64, 10), (512, 100)):
            cfg = make_config(num_agents=N, bottleneckMode="BottomNeck_skipConcat", bottleneckFeature=bf, nGraphFilterTaps=3,
                              device=str(dev))
            torch.manual_seed(1)
            net = DecentralPlannerBottleneckNet(cfg).to(dev).eval()
            x = fov_states(B, N, seed=2).to(dev)
            S = comm_gso(B, N, max(8, int(8.8 * N ** 0.5)), seed=3, dtype=torch.float64).to(dev)

            def step():
                net.addGSO(S)
                net(x)

            with torch.no_grad():
                t = timed(step, reps)
            out.append(dict(leg="forward", bottleneck=bf, B=B, N=N, us=round(t, 2)))
            print(json.dumps(out[-1]), flush=True)
    return out


def step_rows(reps, dev):
    cfg = make_config(num_agents=10, bottleneckMode="BottomNeck_skipConcat", bottleneckFeature=128, nGraphFilterTaps=3,
                      device=str(dev))
    torch.manual_seed(1)
    net = DecentralPlannerBottleneckNet(cfg).to(dev).eval()
    x = fov_states(1, 10, seed=2).to(dev)
    S = comm_gso(1, 10, 20, seed=3, dtype=torch.float64).to(dev)
    with torch.no_grad():
        def eager():
            net.addGSO(S)
            net(x)
        te = timed(eager, reps)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            net.addGSO(S)
            net(x)
        tg = timed(g.replay, reps)
    row = dict(leg="step", B=1, N=10, eager_us=round(te, 2), graph_us=round(tg, 2))
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="layer,forward,step")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    legs = a.legs.split(",")
    if "layer" in legs:
        rows += layer_rows(a.reps, dev)
    if "forward" in legs:
        rows += forward_rows(a.reps, dev)
    if "step" in legs:
        rows += step_rows(a.reps, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
