"""Device time of expert_samples on the two packs the reference transformer is timed on by
tools/make_golden_expert.py --time: 64 cases x 10 agents on a 20 x 20 map and 8 cases x 100 agents on a 50 x 50 map, per
guidance family, dynamic radius; SemiLG_SD twice, on the carried view (one call per step) and with replay=True (one call per
chunk), in the same run.  The schedules come from the same maker and seed with the numpy restatement of the
reference's A* (tests/guidance_restatement.py, pinned against the reference by tests/test_host_guidance.py) in place of the
reference's own; that they are the packs the reference was timed on is asserted through their step counts (STEPS below, the
counts make_golden_expert.py --time prints).  hipEvents around each call,
3 warm-up calls, 10 timed ones, the median and the spread are printed; the pack is on the device before the clock starts.

    python tools/expert_bench.py [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


# (cases, agents, map size, obstacle density) -> steps of the pack, summed over its cases, as the reference's own A* gives them
STEPS = {(64, 10, 20, 0.10): 1866, (8, 100, 50, 0.08): 753}


def main():
    import guidance_restatement as gr
    from make_golden_expert import timing_pack
    from magat_pathplanning_amd import expert_samples, expert_stats, pack_schedules
    astar = lambda grid, s, g: gr.a_star(grid, (int(s[0]), int(s[1])), (int(g[0]), int(g[1])))[0]      # noqa: E731
    dev = torch.device("cuda:0")
    rows = []
    for (C, N, size, density), want in STEPS.items():
        cases = timing_pack(astar, C, N, size, density)
        got = sum(max(len(p) for p in ps) for _, ps, _ in cases)
        assert got == want, "pack %d x %d: %d steps, the reference's A* gives %d: not the pack the reference was timed on" % (
            C, N, got, want)
        pk = pack_schedules([ps for _, ps, _ in cases], [g for _, _, g in cases], device=dev)
        maps = torch.from_numpy(np.stack([m for m, _, _ in cases]).astype(np.uint8)).to(dev)
        steps = int(pk["makespan"].sum().item()) + C
        assert steps == want
        for guidance, replay in (("Project_G", False), ("LocalG_SD", False), ("GlobalG_SD", False), ("SemiLG_SD", False),
                                 ("SemiLG_SD", True)):
            def call():
                s = expert_samples(maps, comm_radius=7.0, dynamic_commR=True, guidance=guidance, replay=replay, **pk)
                expert_stats(s["target"], pk["start"], pk["goal"], s["valid"])
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            ms.sort()
            row = dict(cases=C, agents=N, map=size, guidance=guidance, replay=replay, steps=steps, T=pk["T"], median_ms=ms[len(ms) // 2], min_ms=ms[0],
                       max_ms=ms[-1], us_per_agent_step=1e3 * ms[len(ms) // 2] / (steps * N))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
