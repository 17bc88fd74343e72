"""Device time of ExpertMemory.minibatch(64) beside the only route there was before it: expert_samples on
the cases the batch touches, then flatten_samples and an index.  Two stores: 512 generated cases of 20 x 20 / 10 agents and 128
of 50 x 50 / 100 agents, solved by solve_cases (the unsolved ones are dropped; the counts are printed), guidance Project_G and
SemiLG_SD (a replay memory; the old route is then expert_samples on the carried view), fixed radius 7.  hipEvents around each call, 10 warm-up calls, 50 timed ones, the median and the spread are printed.  The old route is
given the same 64 samples; which cases they touch and where their rows stand in the flattened result is worked out on the host
BEFORE the clock starts, so its time is expert_samples + flatten_samples + index_select alone.

    python tools/memory_bench.py [--out FILE]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORES = ((512, 20, 10), (128, 50, 100))      # cases, map side, agents
M, WARMUP, TIMED = 64, 10, 50


def timed(call):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    from magat_pathplanning_amd import (ExpertMemory, expert_samples, flatten_samples, generate_cases, pack_cases, solve_cases,
                                        solved_pack, valid_cases)
    dev = torch.device("cuda:0")
    rows = []
    for C, side, N, guidance in [s + (g,) for s in STORES for g in ("Project_G", "SemiLG_SD")]:
        cases = valid_cases(generate_cases(C, side, side, N, seed=1, device=dev))
        res = solve_cases(cases["map"], cases["start"], cases["goal"])
        pack = solved_pack(res)
        maps = cases["map"].index_select(0, pack_cases(res))
        K, Lmax = pack["paths"].shape[0], int(pack["lengths"].max().item())
        mem = ExpertMemory(K, N, side, side, Lmax, comm_radius=7.0, guidance=guidance, replay=True, device=dev)
        mem.append(maps, **pack)
        g = torch.Generator(device=dev).manual_seed(2)
        new = timed(lambda: mem.minibatch(M, generator=g))
        mem.check()
        # the old route on one fixed draw
        b = mem.minibatch(M, generator=g)
        touched, place = torch.unique(b["case"].cpu().to(torch.int64), return_inverse=True)
        sub = {key: pack[key].index_select(0, touched.to(dev)) for key in ("paths", "lengths", "goal", "makespan")}
        sub_maps = maps.index_select(0, touched.to(dev))
        steps = (sub["makespan"].cpu().to(torch.int64) + 1)
        firsts = torch.cumsum(steps, 0) - steps
        rows_of = (firsts[place] + b["step"].cpu().to(torch.int64)).to(dev)
        T = int(steps.max())

        def old():
            flat = flatten_samples(expert_samples(sub_maps, comm_radius=7.0, guidance=guidance, T=T, **sub))
            return {key: flat[key].index_select(0, rows_of) for key in ("inputTensor", "target", "GSO", "pos")}

        got = old()
        for key in got:
            assert torch.equal(got[key], b[key]), key      # the two routes give the same batch
        was = timed(old)
        row = dict(cases=K, generated=C, map=side, agents=N, guidance=guidance, samples=len(mem), batch=M, cases_touched=int(touched.numel()), T=T,
                   store_MB=sum(t.numel() * t.element_size() for t in (mem.cells, mem.lengths, mem.goal, mem.makespan, mem.radii,
                                                                       mem.cum, mem.maps)) / 1e6,
                   minibatch=new, expert_samples_route=was)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
