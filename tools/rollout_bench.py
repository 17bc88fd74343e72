"""Cases per second of the closed-loop evaluation (magat_pathplanning_amd/rollout.py: evaluate_cases over an EpisodePool, DESIGN
4.13) against the same cases in fixed batches of BatchedEpisode, each batch stepped to its largest maxstep, on the same build:

    512 cases of 20 x 20 / 10 agents          128 cases of 50 x 50 / 100 agents

Cases from generate_cases (maze, density 0.1, complexity 0.01), every case's limit reference_maxstep(expert makespan, N, 2) from
solve_cases (an unsolved case gets the set's largest).  The policy is a STAND-IN, not a trained model: the states are encoded with
guidance 'GlobalG_S' and the logits push every agent onto the neighbour cell that channel 1 - the A* path to its goal - marks,
drawn with exp_multinorm - episodes end at different times, as a trained model's do.  The policy itself costs next to nothing, so
without --forward the numbers are the simulator side's alone (and mostly launch overhead); --forward also runs a randomly
initialised DecentralPlannerGATNet (K = 3, P = 4, skipConcat) every step and throws its logits away, for a step that costs what a
real one does.  The gain to expect is about max(maxstep) / mean(steps) where the episodes end by arrival.  Wall clock around the
whole run with a device synchronisation at both ends, median of --repeats; one JSON line per shape.

    python tools/rollout_bench.py [--forward] [--slots B] [--repeats K] [--poll P] [--graph gso|edges]

--graph edges hands the model the pool's / the episode's edge structure from the positions instead of the GSO tensor (DESIGN 4.5;
it only matters with --forward: the stand-in policy never reads the graph)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (dict(name="20x20_n10", C=512, size=20, N=10, T=64, seed=201, slots=128),
          dict(name="50x50_n100", C=128, size=50, N=100, T=128, seed=202, slots=32))
DENSITY, COMPLEXITY, RATE, COMM_RADIUS = 0.1, 0.01, 2, 7.0
GUIDANCE = "GlobalG_S"


class StandIn:
    """addGSO + forward with the planner's signatures: x (B,N,3,F,F) -> logits (B,N,5) following channel 1's path."""

    def __init__(self, sharp=4.0, net=None):
        self.sharp, self.net = sharp, net       # net: a planner whose forward is run for its cost alone (--forward)

    def addGSO(self, S):
        if self.net is not None:
            self.net.addGSO(S)

    def __call__(self, x):
        import torch
        c = x.shape[-1] // 2
        g = x[:, :, 1]
        z = torch.stack([g[..., c - 1, c], g[..., c, c - 1], g[..., c + 1, c], g[..., c, c + 1]], dim=-1)      # up, left, down, right
        stop = 2.0 * (z.sum(-1, keepdim=True) == 0).float()
        z = torch.cat([z, stop], dim=-1) * self.sharp
        if self.net is not None:
            y = self.net(x).reshape(z.shape)
            z = z + 0.0 * torch.where(torch.isfinite(y), y, torch.zeros_like(y))
        return z


def timed(fn, repeats):
    import torch
    out, secs = None, []
    for _ in range(repeats + 1):                  # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    secs = sorted(secs[1:])
    return out, secs[len(secs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=0, help="slots / batch size (default: a quarter of the cases)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--poll", type=int, default=16)
    ap.add_argument("--forward", action="store_true", help="run a randomly initialised DecentralPlannerGATNet every step, for its cost")
    ap.add_argument("--graph", choices=("gso", "edges"), default="gso", help="what addGSO is given: the GSO tensor or the edge structure")
    args = ap.parse_args()
    import torch
    from magat_pathplanning_amd import (BatchedEpisode, DecentralPlannerGATNet, evaluate_cases, generate_cases, reference_maxstep,
                                        solve_cases)
    from magat_pathplanning_amd.synthetic import make_config
    assert torch.cuda.is_available(), "rollout_bench needs a GPU (no fallback)"
    dev = torch.device("cuda:0")
    for sh in SHAPES:
        C, S, N, B = sh["C"], sh["size"], sh["N"], args.slots or sh["slots"]
        net = StandIn()
        if args.forward:
            cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, device="cuda:0", bottleneckMode="BottomNeck_skipConcat")
            net = StandIn(net=DecentralPlannerGATNet(cfg).to(dev).eval())
        cases = generate_cases(C, S, S, N, DENSITY, COMPLEXITY, seed=sh["seed"], device=dev)
        assert bool(cases["valid"].all())
        res = solve_cases(cases["map"], cases["start"], cases["goal"], horizon=sh["T"])
        mk = res["makespan"].clamp(min=1)
        mk = torch.where(res["solved"] != 0, mk, mk.max())
        maxstep = torch.from_numpy(reference_maxstep(mk, N, RATE)).to(dev)
        kw = dict(action_select="exp_multinorm", seed=sh["seed"], guidance=GUIDANCE)

        def pool():
            return evaluate_cases(net, cases["map"], cases["start"], cases["goal"], maxstep, B, COMM_RADIUS, poll=args.poll,
                                  graph=args.graph, **kw)

        def fixed():
            reached = 0
            with torch.no_grad():
                for lo in range(0, C, B):
                    sl = slice(lo, min(lo + B, C))
                    limit = int(maxstep[sl].max())
                    ep = BatchedEpisode(cases["map"][sl], cases["start"][sl], cases["goal"][sl], limit, COMM_RADIUS,
                                        action_select="exp_multinorm", guidance=GUIDANCE)
                    ep.currentstep = 1
                    for _ in range(limit):
                        net.addGSO(ep.edges() if args.graph == "edges" else ep.gso())
                        ep.step(logits=net(ep.states()))
                    reached += int(ep.done.sum())
            return reached

        r, pool_s = timed(pool, args.repeats)
        reached, fixed_s = timed(fixed, args.repeats)
        steps = r["steps"].float()
        print(json.dumps(dict(shape=sh["name"], forward=bool(args.forward), graph=args.graph, cases=C, agents=N, slots=B, maxstep_max=int(maxstep.max()),
                              maxstep_mean=float(maxstep.float().mean()), steps_mean=float(steps.mean()),
                              all_reach=float(r["all_reach"].float().mean()), expected_gain=float(maxstep.max()) / float(steps.mean()),
                              pool_s=pool_s, pool_cases_per_s=C / pool_s, fixed_s=fixed_s, fixed_cases_per_s=C / fixed_s,
                              fixed_all_reach=reached / C, gain=fixed_s / pool_s)), flush=True)


if __name__ == "__main__":
    main()
