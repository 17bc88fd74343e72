"""Times ONE batched_fov_states call per guidance string on the device: 'Project_G' (the existing kernel, the yardstick) and the
six A*-guided encodings (csrc/sim_guidance.hip), at the closed loop's c3 batch (512 x 100 agents) and at the reference's own
loop size (1 x 100), 50 x 50 map, density 0.1.

    python tools/guidance_bench.py [--out FILE.json] [--reps 50]

Device events around `reps` calls after a warm-up of every shape; the median over 5 such windows is reported, min and max next
to it.  SemiLG is timed on a memory that has seen the positions of the timed call (its steady state inside an episode).
Prints a table and writes the same numbers as JSON (the c3 forward it is compared with in DESIGN.md is bench.py's headline,
taken in the same visit).

    python tools/guidance_bench.py --wide [--wide-reps 3] [--pops 16] [--out FILE.json]

times the wide form instead (csrc/sim_guidance_wide.hip, batched_fov_states(..., wide=True)) the same way - device events around
`wide-reps` calls, the median of 5 windows - at 64 x (65 x 65, 100 agents) GlobalG_SD and SemiLG_SD, 8 x (160 x 160, 1000
agents) GlobalG_SD and 8 x (200 x 200, 1000 agents) GlobalG_SD, density 0.1.  A call there can take a large part of a second,
hence the smaller default.  Next to each row: the pops of the searches of the first `pops` agents of instance 0 (mean, median,
maximum), counted by tests/guidance_restatement.py on the host."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from magat_pathplanning_amd import GUIDANCE_MODES, batched_fov_states, new_agent_view

ORDER = ["Project_G", "LocalG_S", "LocalG_SD", "GlobalG_S", "GlobalG_SD", "SemiLG_S", "SemiLG_SD"]


def scenario(B, N, size, density, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random((size, size)) < density).astype(np.uint8)
    free = np.argwhere(m == 0)
    pos = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(B)]).astype(np.int32)
    goal = np.stack([free[rng.permutation(len(free))[:N]] for _ in range(B)]).astype(np.int32)
    return m, pos, goal


def windows(fn, reps, nwin=5, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return dict(median_ms=out[len(out) // 2], min_ms=out[0], max_ms=out[-1])


WIDE_ROWS = [(64, 100, 65, "GlobalG_SD"), (64, 100, 65, "SemiLG_SD"), (8, 1000, 160, "GlobalG_SD"), (8, 1000, 200, "GlobalG_SD")]


def pop_counts(m, pos, goal, guidance, k):
    """Pops of the first k searches of one instance, by the restatement (the other agents only stand in the way)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import guidance_restatement as gr
    half = 4
    grid_of = np.pad(np.pad((m != 0).astype(np.int64), half, constant_values=1), 1, constant_values=0)
    pops = []
    for n in range(min(k, len(pos))):
        grid = grid_of.copy()
        near = pos[(np.abs(pos - pos[n]) <= half).all(axis=1)]
        grid[near[:, 0] + half + 1, near[:, 1] + half + 1] += 1      # '_SD' (and SemiLG): the agents inside the FOV block
        s, g = tuple(pos[n] + half + 1), tuple(goal[n] + half + 1)
        if grid[g] == 1:
            grid[g] = 0
        pops.append(gr.a_star(grid, s, g)[1])
    return dict(pops_mean=float(np.mean(pops)), pops_median=float(np.median(pops)), pops_max=int(np.max(pops)), pops_agents=len(pops))


def main_wide(args):
    reps = int(args[args.index("--wide-reps") + 1]) if "--wide-reps" in args else 3
    k = int(args[args.index("--pops") + 1]) if "--pops" in args else 16
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), density=0.1, reps=reps, rows=[])
    for B, N, size, g in WIDE_ROWS:
        m, pos, goal = scenario(B, N, size, 0.1, seed=7)
        dm, dp, dg = (torch.from_numpy(a).to(dev) for a in (m, pos, goal))
        view = new_agent_view(B, N, size, size, 9, dev) if g.startswith("SemiLG") else None
        r = windows(lambda: batched_fov_states(dm, dp, dg, 9, guidance=g, agent_view=view, wide=True), reps, warm=1)
        r.update(B=B, N=N, map=size, guidance=g, us_per_agent=r["median_ms"] * 1e3 / (B * N))
        if k:
            r.update(pop_counts(m, pos[0], goal[0], g, k))      # (SemiLG: an upper bound, the full map instead of the remembered one)
        result["rows"].append(r)
        print("B %3d N %4d map %3d  %-10s  %9.3f ms / call  (min %.3f max %.3f)  %8.2f us / agent  pops %s"
              % (B, N, size, g, r["median_ms"], r["min_ms"], r["max_ms"], r["us_per_agent"],
                 "mean %.0f median %.0f max %d over %d agents" % (r["pops_mean"], r["pops_median"], r["pops_max"], r["pops_agents"])
                 if k else "not counted"), flush=True)
        if out_path:      # after every row: a run cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as fh:
                json.dump(result, fh, indent=1)


def main():
    args = sys.argv[1:]
    if "--wide" in args:
        return main_wide(args)
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 50
    assert reps >= 50 or "--quick" in args, "at least 50 repeats per window"
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    assert set(ORDER) == set(GUIDANCE_MODES)
    result = dict(device=torch.cuda.get_device_name(0), map=50, density=0.1, reps=reps, rows=[])
    for B, N in ((512, 100), (1, 100)):
        m, pos, goal = scenario(B, N, 50, 0.1, seed=7)
        dm, dp, dg = (torch.from_numpy(a).to(dev) for a in (m, pos, goal))
        for g in ORDER:
            view = new_agent_view(B, N, 50, 50, 9, dev) if g.startswith("SemiLG") else None
            r = windows(lambda: batched_fov_states(dm, dp, dg, 9, guidance=g, agent_view=view), reps)
            r.update(B=B, N=N, guidance=g, ns_per_agent=r["median_ms"] * 1e6 / (B * N))
            result["rows"].append(r)
            print("B %4d N %4d  %-10s  %8.3f ms / call  (min %.3f max %.3f)  %8.1f ns / agent"
                  % (B, N, g, r["median_ms"], r["min_ms"], r["max_ms"], r["ns_per_agent"]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
