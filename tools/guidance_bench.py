"""Times ONE batched_fov_states call per guidance string on the device: 'Project_G' (the existing kernel, the yardstick) and the
six A*-guided encodings (csrc/sim_guidance.hip), at the closed loop's c3 batch (512 x 100 agents) and at the reference's own
loop size (1 x 100), 50 x 50 map, density 0.1.

    python tools/guidance_bench.py [--out FILE.json] [--reps 50]

Device events around `reps` calls after a warm-up of every shape; the median over 5 such windows is reported, min and max next
to it.  SemiLG is timed on a memory that has seen the positions of the timed call (its steady state inside an episode).
Prints a table and writes the same numbers as JSON (the c3 forward it is compared with in DESIGN.md is bench.py's headline,
taken in the same visit)."""
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


def windows(fn, reps, nwin=5):
    for _ in range(5):
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


def main():
    args = sys.argv[1:]
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
