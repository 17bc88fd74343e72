"""Closed loop entirely on the device: per step  GSO construction -> FOV state tensors -> addGSO + forward -> action decode +
collision shielding + position update, for B independent planning instances (what the reference does per instance on the
host around a batch-1 forward: agents/decentralplannerlocal_OnlineExpert_GAT.py:880-905 -> utils/new_simulator.py).
Reports agent-steps/s of the whole loop next to the forward alone.

    python tools/closed_loop_bench.py [B N size T]
    python tools/closed_loop_bench.py B N size T --graph gso|edges|both [--storage bf16] [--rounds R]

--graph times the step with the graph handed over as the GSO tensor (batched_gso) and / or as the edge structure from the
positions (batched_edges, DESIGN 4.5: the only route above 2048 agents): the legs alternate inside this process, R rounds of T
steps each on the same moving positions, and the median, the smallest and the largest round of each leg are printed - nothing else
of the script runs then."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from magat_pathplanning_amd import DecentralPlannerGATNet
from magat_pathplanning_amd.simulator import batched_fov_states, batched_gso, batched_move
from magat_pathplanning_amd.synthetic import make_config

ARGV = sys.argv[1:]


def flag(name, default):
    if name not in ARGV:
        return default
    i = ARGV.index(name)
    value = ARGV[i + 1]
    del ARGV[i:i + 2]
    return value


GRAPH, STORAGE, ROUNDS = flag("--graph", None), flag("--storage", "fp32"), int(flag("--rounds", "5"))
B, N, size, T = (int(a) for a in (ARGV[:4] + ["512", "100", "50", "20"][len(ARGV):]))
dev = torch.device("cuda:0")
rng = np.random.default_rng(3)
m = (rng.random((size, size)) < 0.08).astype(np.uint8)
free = np.argwhere(m == 0)
pos = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(B)]).astype(np.int32)
goal = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(B)]).astype(np.int32)
dm, dpos, dgoal = torch.from_numpy(m).to(dev), torch.from_numpy(pos).to(dev).contiguous(), torch.from_numpy(goal).to(dev)
cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, bottleneckMode="BottomNeck_skipConcat", device=str(dev))
if STORAGE != "fp32":
    cfg.gat_storage = STORAGE
torch.manual_seed(0)
net = DecentralPlannerGATNet(cfg).to(dev).eval()


def graph_legs():
    """--graph: the step with the GSO tensor against the step with the edge structure, alternating"""
    from magat_pathplanning_amd.simulator import batched_edges
    legs = [g for g in ("gso", "edges") if GRAPH in (g, "both")]
    if not legs:
        raise SystemExit("--graph takes gso, edges or both")
    edges = batched_edges(dpos, 7.0)              # over dpos itself: refreshed behind every move, its arrays reused

    def one(leg):
        with torch.no_grad():
            net.addGSO(edges.refresh() if leg == "edges" else batched_gso(dpos, 7.0))
            logits = net(batched_fov_states(dm, dpos, dgoal, 9))
        return batched_move(dm, dpos, logits=logits, goal=dgoal, wide=True)

    def box_clock():
        """the core clock this box holds under matrix load (the numbers move with it)"""
        import ctypes
        from magat_pathplanning_amd import _native as nat
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        scratch = torch.empty(256 * cus + 4 * cus, dtype=torch.float32, device=dev)
        tf, mhz, per = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        nat.check(nat.lib().magat_mfma_sustained_f16_ex(ctypes.byref(tf), ctypes.byref(mhz), ctypes.byref(per), nat.ptr(scratch), 5,
                                                        nat.current_stream(dev)), "magat_mfma_sustained_f16_ex")
        return mhz.value

    ms = {leg: [] for leg in legs}
    for leg in legs:
        for _ in range(3):
            one(leg)
    for _ in range(ROUNDS):
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(T):
                one(leg)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) / T * 1e3)
    for leg in legs:
        v = sorted(ms[leg])
        print("B %d N %d map %dx%d storage %s graph=%s: closed loop median %.3f ms/step (%.3f .. %.3f over %d rounds of %d steps) = "
              "%.2f M agent-steps/s" % (B, N, size, size, STORAGE, leg, v[len(v) // 2], v[0], v[-1], ROUNDS, T, B * N / v[len(v) // 2] / 1e3))
    print("sustained matrix clock of this box: %.0f MHz" % box_clock())


if GRAPH is not None:
    graph_legs()
    sys.exit(0)


NORMALIZE = True


def step():
    with torch.no_grad():
        net.addGSO(batched_gso(dpos, 7.0, normalize=NORMALIZE))
        logits = net(batched_fov_states(dm, dpos, dgoal, 9))
    return batched_move(dm, dpos, logits=logits, goal=dgoal)


for _ in range(3):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(T):
    out = step()
torch.cuda.synchronize()
loop = (time.perf_counter() - t0) / T
x = batched_fov_states(dm, dpos, dgoal, 9)
S = batched_gso(dpos, 7.0)
torch.cuda.synchronize()
t0 = time.perf_counter()
with torch.no_grad():
    for _ in range(T):
        net.addGSO(S)
        net(x)
torch.cuda.synchronize()
fwd = (time.perf_counter() - t0) / T
print("B %d N %d map %dx%d: closed loop %.3f ms/step = %.2f M agent-steps/s   (forward alone %.3f ms = %.2f M; front/back end %.3f ms)"
      % (B, N, size, size, loop * 1e3, B * N / loop / 1e6, fwd * 1e3, B * N / fwd / 1e6, (loop - fwd) * 1e3))
print("reached goals after %d random-policy steps: %d of %d agents" % (T + 3, int(out["reached"].sum()), B * N))

# The attention layers read the GSO only as an edge mask (|S| > 1e-9, graphML.py:1274): the 1 / lambda_max scaling of the
# reference's GSO (a Lanczos + Sturm eigenvalue per instance, 0.15 ms per batch here) does not reach the logits.  A GAT-only
# closed loop may hand over the 0/1 adjacency instead - same logits bit for bit:
with torch.no_grad():
    net.addGSO(S)
    y_norm = net(x).clone()
    net.addGSO(batched_gso(dpos, 7.0, normalize=False))
    y_adj = net(x).clone()
NORMALIZE = False
for _ in range(3):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(T):
    out = step()
torch.cuda.synchronize()
loop2 = (time.perf_counter() - t0) / T
print("with the 0/1 adjacency as GSO (logits identical: %s): closed loop %.3f ms/step = %.2f M agent-steps/s"
      % (bool(torch.equal(y_norm, y_adj)), loop2 * 1e3, B * N / loop2 / 1e6))

# The same loop through BatchedEpisode: the reference's whole per-case state on the device (step-0 radius growth, reach_goal /
# first_move / end_step, flowtime / makespan), exp_multinorm action sampling from a seeded device generator.
from magat_pathplanning_amd.simulator import BatchedEpisode
gen = torch.Generator(device=dev).manual_seed(11)
ep = BatchedEpisode(dm, torch.from_numpy(pos).to(dev), dgoal, maxstep=10 ** 6, comm_radius=7.0, action_select="exp_multinorm",
                    generator=gen)
torch.cuda.synchronize()
t0 = time.perf_counter()
S0 = ep.gso()                      # includes the radius growth of step 0
torch.cuda.synchronize()
t_first = time.perf_counter() - t0


def ep_step():
    with torch.no_grad():
        net.addGSO(ep.gso())
        return ep.step(net(ep.states()))


for _ in range(3):
    ep_step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(T):
    ep_step()
torch.cuda.synchronize()
loop3 = (time.perf_counter() - t0) / T
print("BatchedEpisode (exp_multinorm, bookkeeping on device): %.3f ms/step = %.2f M agent-steps/s; first getGSO with radius growth %.2f ms "
      "(radii %.2f..%.2f); agents at their goals after %d steps: %d"
      % (loop3 * 1e3, B * N / loop3 / 1e6, t_first * 1e3, float(ep.radii.min()), float(ep.radii.max()), T + 3, int(ep.reach_goal.sum())))
