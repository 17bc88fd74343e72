"""Training-step time of DecentralPlannerGATNet (forward + cross-entropy + backward + SGD step, train mode) with the HIP
convolution backend (train_cnn.py: magat_conv_gemm_f32 forward / input gradient, magat_conv_wgrad_f32 weight gradient) and with
torch's own convolutions (MAGAT_TRAIN_CNN=torch: MIOpen); the graph layer trains on the HIP kernels either way.
   python tools/train_step_bench.py [B N] ...
   python tools/train_step_bench.py --training-loss [B N] ...     also the route through net.training_loss (the last Linear of
                                                                  actionsMLP and the loss on csrc/head_loss.hip), alternating
                                                                  with net(x) + tnf.cross_entropy in the same process
   python tools/train_step_bench.py --steps=200 ...                timed steps per measurement (default 20)
   python tools/train_step_bench.py --launches [B N] ...          no timing: kernel launches of ONE step on either route, from
                                                                  a kernel trace (torch.profiler) - a run of its own"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as tnf
from magat_pathplanning_amd import DecentralPlannerGATNet
from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config

args = [a for a in sys.argv[1:] if not a.startswith("--")]
FUSED, LAUNCHES = "--training-loss" in sys.argv, "--launches" in sys.argv
STEPS = max([int(a[8:]) for a in sys.argv if a.startswith("--steps=")] + [0]) or 20
dev = torch.device("cuda:0")
shapes = [(int(args[i]), int(args[i + 1])) for i in range(0, len(args) - 1, 2)] or [(64, 10), (64, 100)]
routes = ("torch", "fused") if FUSED or LAUNCHES else ("torch",)


def launches_of(step, steps=5):
    """kernel launches per step: device kernel events of `steps` steps in a kernel trace"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and
             "memset" not in e.name.lower()]
    return len(names) / steps, sum("head_loss" in n or "action_loss" in n or "loss_finalize" in n for n in names) / steps


for B, N in shapes:
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, bottleneckMode="BottomNeck_skipConcat", device="cuda:0")
    x = fov_states(B, N, seed=5).to(dev)
    S = comm_gso(B, N, 20 if N <= 20 else 50, seed=6).to(dev)
    tgt = torch.randint(0, 5, (B * N,)).to(dev)
    for backend, route in [(b, r) for b in ("hip", "torch", "hip", "torch") for r in routes][:4 if LAUNCHES else None]:
        os.environ["MAGAT_TRAIN_CNN"] = backend
        torch.manual_seed(1)
        net = DecentralPlannerGATNet(cfg).to(dev).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.01)

        def step():
            net.addGSO(S)
            loss = net.training_loss(x, tgt)[0] if route == "fused" else tnf.cross_entropy(net(x), tgt)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        if LAUNCHES:
            per_step, ours = launches_of(step)
            print("B=%d N=%d (%d agents)  convolutions on %-5s  loss on %-5s  %.1f kernel launches / training step (%.1f of "
                  "head_loss.hip)" % (B, N, B * N, backend, route, per_step, ours))
            continue
        t0 = time.perf_counter()
        n = STEPS
        for _ in range(n):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        print("B=%d N=%d (%d agents)  convolutions on %-5s  loss on %-5s  %.2f ms / training step  (%.0f agent-steps/s), loss %.4f" % (
            B, N, B * N, backend, route, dt * 1e3, B * N / dt, float(loss)))
