"""Times the case generator (magat_pathplanning_amd/cases.py, csrc/sim_cases.hip) next to the solver on the cases it made, at
the batch shapes of tools/mapf_bench.py, the last two in the wide form (csrc/sim_cases_wide.hip, wide=True):

    512 cases of 20 x 20 / 10 agents / T = 64          128 cases of 50 x 50 / 100 agents / T = 128
    64 cases of 65 x 65 / 100 agents / T = 360         8 cases of 200 x 200 / 1000 agents / T = 1024

Device events around generate_cases (kind "maze" at density 0.1, complexity 0.01 - the reference's defaults - and kind
"uniform" at density 0.1) and around plan_prioritized on the maze cases: 10 warm-ups, median of 50 calls (when one call takes
more than a second: 1 warm-up, median of 5, named in "*_calls").  With
--restatement K the CPU seconds that tests/cases_restatement.py (a per-cell Python restatement; the only comparison there
is) needs for K cases of each shape.  One JSON line per shape.

    python tools/cases_bench.py [--restatement K] [--no-device]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_restatement as cr  # noqa: E402

SHAPES = (dict(name="20x20_n10", C=512, size=20, N=10, T=64, seed=101),
          dict(name="50x50_n100", C=128, size=50, N=100, T=128, seed=102),
          dict(name="wide_65x65_n100", C=64, size=65, N=100, T=360, seed=103, wide=True),
          dict(name="wide_200x200_n1000", C=8, size=200, N=1000, T=1024, seed=104, wide=True))
DENSITY, COMPLEXITY = 0.1, 0.01


def median_ms(fn, warmup, calls):
    import torch
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 1.0:      # a call of more than a second: fewer repeats
        warmup, calls = 1, min(calls, 5)
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return out, ms[len(ms) // 2], ms[0], ms[-1], calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restatement", type=int, default=0, help="time the Python restatement on this many cases per shape")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    for sh in SHAPES:
        C, S, N = sh["C"], sh["size"], sh["N"]
        out = dict(shape=sh["name"], cases=C, agents=N, T=sh["T"])
        if not args.no_device:
            import torch
            from magat_pathplanning_amd import generate_cases, plan_prioritized
            assert torch.cuda.is_available(), "cases_bench needs a GPU (no fallback)"
            wide = sh.get("wide", False)
            maze, ms, lo, hi, n = median_ms(lambda: generate_cases(C, S, S, N, DENSITY, COMPLEXITY, seed=sh["seed"], wide=wide),
                                            args.warmup, args.calls)
            out.update(maze_calls=n, maze_ms_median=ms, maze_ms_min=lo, maze_ms_max=hi, maze_us_per_case=ms * 1e3 / C,
                       maze_valid=float(maze["valid"].float().mean()), maze_free_cells_mean=float(maze["free_cells"].float().mean()))
            uni, ms, lo, hi, n = median_ms(lambda: generate_cases(C, S, S, N, DENSITY, kind="uniform", seed=sh["seed"], wide=wide),
                                           args.warmup, args.calls)
            out.update(uniform_calls=n, uniform_ms_median=ms, uniform_ms_min=lo, uniform_ms_max=hi, uniform_us_per_case=ms * 1e3 / C,
                       uniform_valid=float(uni["valid"].float().mean()), uniform_free_cells_mean=float(uni["free_cells"].float().mean()))
            assert bool(maze["valid"].all()), "the solver is only fed valid cases"
            res, ms, lo, hi, n = median_ms(lambda: plan_prioritized(maze["map"], maze["start"], maze["goal"], horizon=sh["T"],
                                                                    wide=wide), args.warmup, args.calls)
            out.update(plan_calls=n, plan_ms_median=ms, plan_ms_min=lo, plan_ms_max=hi, plan_solved_first_try=float(res["solved"].float().mean()))
        if args.restatement:
            k = min(args.restatement, C)
            t0 = time.perf_counter()
            ref = cr.generate("maze", k, S, S, N, DENSITY, COMPLEXITY, seed=sh["seed"])
            sec = time.perf_counter() - t0
            out.update(restatement_cases=k, restatement_cpu_s=sec, restatement_cpu_s_per_case=sec / k,
                       restatement_valid=float(ref["valid"].mean()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
