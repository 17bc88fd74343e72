"""Times the path-finding expert (magat_pathplanning_amd/mapf.py, csrc/sim_mapf.hip) at two batch shapes, and its wide form
(csrc/sim_mapf_wide.hip, wide=True, the default wide horizon) at two more:

    512 cases of 20 x 20 / 10 agents / T = 64          128 cases of 50 x 50 / 100 agents / T = 128
    64 cases of 65 x 65 / 100 agents / T = 360         8 cases of 200 x 200 / 1000 agents / T = 1024

Device events around plan_prioritized (10 warm-ups, median of 50 calls; when one call takes more than a second, 1 warm-up and
the median of 5, and the line says so in "calls"), the share of cases solved at the first try and after
solve_cases' retries, and - with --restatement K - the CPU seconds that tests/mapf_restatement.py (a per-cell Python
restatement, NOT ECBS; the only comparison there is) needs for the first K cases of each shape.  One JSON line per shape.

Every shape gets a second line, "<shape>_improve": improve_schedules (csrc/sim_mapf_lns.hip, and for the two wide shapes
csrc/sim_mapf_lns_wide.hip with wide=True on solve_cases(..., wide=True)'s result; iterations = 32, neighbourhood = 4) on
solve_cases' result, timed the same way, with the total flowtime of the solved cases going in and coming out and the
free-space lower bound sum(d0 - 1) - every agent planned alone on the empty map: one more plan_prioritized call with C N
one-agent cases; at the wide shapes only the agents of the solved cases, with the longest solved path as the horizon, in
chunks whose workspace stays below 1 GiB.

And a third one, "<shape>_audit": audit_schedules (csrc/sim_mapf_audit.hip, for the two wide shapes csrc/sim_mapf_audit_wide.hip
with wide=True) on solve_cases' result, timed the same way, with what it found: the cases valid / skipped / faulty, the cases
certified at w = 1, 1.05 and 1.25, and the largest flowtime / bound ratio of the valid ones.

The two 64 x 64-form shapes get a fourth one, "<shape>_cbs": cbs_cases (csrc/sim_mapf_cbs.hip, conflict-based search, max_nodes
= 256) on the same batch, timed the same way, with the share of cases proven optimal, the share that ended at the budget, the
mean of flowtime / lower_bound - CBS's flowtime where it proved the optimum, else solve_cases' - over the cases that have both,
and, over the cases CBS proved optimal and solve_cases solved, both total flowtimes.  Beside it stands "<shape>_ecbs": ecbs_cases
(csrc/sim_mapf_ecbs.hip, ECBS with w = 1.5, max_nodes = 256, 4 levels) on the same batch, timed the same way: the time per call,
the share of cases solved, the mean of flowtime / lower_bound over them, and its total flowtime against solve_cases' (over the cases
both solved) and against CBS's (over the cases CBS proved optimal).  None of these figures is a gate.

Last come two rows of the wide ECBS (csrc/sim_mapf_ecbs_wide.hip, ecbs_cases_wide with w = 1.5, max_nodes = 256, 4 levels), on
batches of their own - 32 cases of 65 x 65 / 100 agents and 4 cases of 160 x 160 / 1000 agents, "<shape>_ecbs_wide" - at the
horizon solve_cases(wide=True) used: the time per call, the cases solved, the mean of flowtime / lower_bound over them, and its
total flowtime next to that of solve_cases(wide=True, improve=32) over the cases both solved.  A row whose workspace does not fit
the free device memory says so and times nothing.

    python tools/mapf_bench.py [--restatement K] [--no-device]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mapf_restatement as mr  # noqa: E402

SHAPES = (dict(name="20x20_n10", C=512, size=20, N=10, T=64, density=0.1, seed=101),
          dict(name="50x50_n100", C=128, size=50, N=100, T=128, density=0.1, seed=102),
          dict(name="wide_65x65_n100", C=64, size=65, N=100, T=360, density=0.1, seed=103, wide=True),
          dict(name="wide_200x200_n1000", C=8, size=200, N=1000, T=1024, density=0.1, seed=104, wide=True))


IMPROVE = dict(iterations=32, neighbourhood=4)


def timed(fn, warmup, calls):
    """Device events around fn(): sorted milliseconds of `calls` calls after `warmup` warm-ups, and the last result."""
    import torch
    for _ in range(warmup):
        res = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms), res


def free_lengths_wide(d, ok, horizon):
    """d0 (K,N) of the agents of the cases in `ok`: each planned alone by the wide planner, a chunk of one-agent cases per call."""
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import plan_prioritized
    idx = torch.nonzero(ok).flatten()
    s, g = d[1].index_select(0, idx).reshape(-1, 1, 2), d[2].index_select(0, idx).reshape(-1, 1, 2)
    H, W = d[0].shape[-2], d[0].shape[-1]
    chunk = max(1, (1 << 30) // max(1, int(nat.lib().magat_sim_mapf_wide_workspace_bytes(1, H, W, horizon))))
    lengths = []
    for i in range(0, len(s), chunk):
        alone = plan_prioritized(d[0], s[i:i + chunk].contiguous(), g[i:i + chunk].contiguous(), horizon=horizon, wide=True)
        assert bool(alone["solved"].all())
        lengths.append(alone["lengths"])
    return torch.cat(lengths).reshape(len(idx), -1)


def improve_row(sh, d, full, args):
    import torch
    from magat_pathplanning_amd import improve_schedules, plan_prioritized
    wide = sh.get("wide", False)
    t0 = time.perf_counter()
    improve_schedules(d[0], full, wide=wide, **IMPROVE)
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 1.0
    warmup, calls = (1, min(args.calls, 5)) if slow else (args.warmup, args.calls)
    ms, better = timed(lambda: improve_schedules(d[0], full, wide=wide, **IMPROVE), warmup, calls)
    ok = better["status"] == 0
    if not bool(ok.any()):
        return dict(shape=sh["name"] + "_improve", cases=sh["C"], agents=sh["N"], T=sh["T"], warmup=warmup, calls=calls, **IMPROVE,
                    improve_ms_median=ms[len(ms) // 2], improve_ms_min=ms[0], improve_ms_max=ms[-1], cases_improved_or_unchanged=0)
    if wide:
        lower = int((free_lengths_wide(d, ok, int(full["makespan"][ok].max()) + 1) - 1).sum())
    else:
        alone = plan_prioritized(d[0], d[1].reshape(-1, 1, 2), d[2].reshape(-1, 1, 2), horizon=sh["T"])      # every agent on the empty map
        d0 = alone["lengths"].reshape(sh["C"], sh["N"])
        assert bool(alone["solved"].all())
        lower = int((d0[ok] - 1).sum())
    return dict(shape=sh["name"] + "_improve", cases=sh["C"], agents=sh["N"], T=sh["T"], warmup=warmup, calls=calls, **IMPROVE,
                improve_ms_median=ms[len(ms) // 2], improve_ms_min=ms[0], improve_ms_max=ms[-1],
                cases_improved_or_unchanged=int(ok.sum()), cases_with_an_accepted_iteration=int((better["accepted"] > 0).sum()),
                accepted_iterations=int(better["accepted"].sum()), flowtime_before=int(better["flowtime_before"][ok].sum()),
                flowtime_after=int(better["flowtime_after"][ok].sum()), flowtime_lower_bound=lower,
                makespan_max_before=int(full["makespan"][ok].max()), makespan_max_after=int(better["makespan"][ok].max()))


def audit_row(sh, d, full, args):
    import torch
    from magat_pathplanning_amd import audit_schedules, certified
    wide = sh.get("wide", False)
    t0 = time.perf_counter()
    audit_schedules(d[0], full, wide=wide)
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 1.0
    warmup, calls = (1, min(args.calls, 5)) if slow else (args.warmup, args.calls)
    ms, audit = timed(lambda: audit_schedules(d[0], full, wide=wide), warmup, calls)
    ok = (audit["status"] == 0) & (audit["flowtime_bound"] > 0)
    ratio = (audit["flowtime"][ok].double() / audit["flowtime_bound"][ok].double()) if bool(ok.any()) else None
    return dict(shape=sh["name"] + "_audit", cases=sh["C"], agents=sh["N"], T=sh["T"], warmup=warmup, calls=calls,
                audit_ms_median=ms[len(ms) // 2], audit_ms_min=ms[0], audit_ms_max=ms[-1],
                audit_us_per_case=ms[len(ms) // 2] * 1e3 / sh["C"], cases_valid=int((audit["status"] == 0).sum()),
                cases_skipped=int((audit["status"] == 1).sum()), cases_faulty=int((audit["status"] == 2).sum()),
                certified_1=int(certified(audit, 1).sum()), certified_1_05=int(certified(audit, 1.05).sum()),
                certified_1_25=int(certified(audit, 1.25).sum()), ratio_max=None if ratio is None else float(ratio.max()),
                flowtime=int(audit["flowtime"][ok].sum()), flowtime_bound=int(audit["flowtime_bound"][ok].sum()))


CBS_NODES = 256


def cbs_row(sh, d, full, args):
    import torch
    from magat_pathplanning_amd import cbs_cases
    run = lambda: cbs_cases(*d, horizon=sh["T"], max_nodes=CBS_NODES)      # noqa: E731
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 1.0
    warmup, calls = (1, min(args.calls, 5)) if slow else (args.warmup, args.calls)
    ms, opt = timed(run, warmup, calls)
    proven, solved = opt["status"] == 0, full["solved"] != 0
    flow = (full["lengths"] - 1).sum(1)
    both = proven & solved
    have = (proven | solved) & (opt["lower_bound"] > 0)
    ratio = torch.where(proven, opt["flowtime"], flow)[have].double() / opt["lower_bound"][have].double()
    return dict(shape=sh["name"] + "_cbs", cases=sh["C"], agents=sh["N"], T=sh["T"], warmup=warmup, calls=calls, max_nodes=CBS_NODES,
                cbs_ms_median=ms[len(ms) // 2], cbs_ms_min=ms[0], cbs_ms_max=ms[-1], cbs_us_per_case=ms[len(ms) // 2] * 1e3 / sh["C"],
                proven_optimal=float(proven.float().mean()), at_budget=float((opt["status"] == 1).float().mean()),
                no_schedule=float((opt["status"] >= 2).float().mean()), horizon_hit=int((opt["horizon_hit"] != 0).sum()),
                nodes_mean=float(opt["nodes"].float().mean()), ratio_mean=float(ratio.mean()) if have.any() else None,
                ratio_cases=int(have.sum()), flowtime_cbs=int(opt["flowtime"][both].sum()), flowtime_solve_cases=int(flow[both].sum()),
                solved_only_by_cbs=int((proven & ~solved).sum()))


ECBS = dict(w=1.5, max_nodes=256, levels=4)


def ecbs_row(sh, d, full, args):
    import torch
    from magat_pathplanning_amd import cbs_cases, ecbs_cases
    run = lambda: ecbs_cases(*d, horizon=sh["T"], **ECBS)      # noqa: E731
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 1.0
    warmup, calls = (1, min(args.calls, 5)) if slow else (args.warmup, args.calls)
    ms, sub = timed(run, warmup, calls)
    opt = cbs_cases(*d, horizon=sh["T"], max_nodes=CBS_NODES)      # (not timed here: the _cbs row does)
    done, solved, proven = sub["status"] == 0, full["solved"] != 0, opt["status"] == 0
    flow = (full["lengths"] - 1).sum(1)
    have = done & (sub["lower_bound"] > 0)
    ratio = sub["flowtime"][have].double() / sub["lower_bound"][have].double()
    return dict(shape=sh["name"] + "_ecbs", cases=sh["C"], agents=sh["N"], T=sh["T"], warmup=warmup, calls=calls, **ECBS,
                ecbs_ms_median=ms[len(ms) // 2], ecbs_ms_min=ms[0], ecbs_ms_max=ms[-1], ecbs_us_per_case=ms[len(ms) // 2] * 1e3 / sh["C"],
                solved=float(done.float().mean()), at_budget=float((sub["status"] == 1).float().mean()),
                no_schedule=float((sub["status"] >= 2).float().mean()), horizon_hit=int((sub["horizon_hit"] != 0).sum()),
                nodes_mean=float(sub["nodes"].float().mean()), ratio_mean=float(ratio.mean()) if have.any() else None,
                ratio_max=float(ratio.max()) if have.any() else None,
                flowtime_ecbs_vs_solve_cases=[int(sub["flowtime"][done & solved].sum()), int(flow[done & solved].sum())],
                flowtime_ecbs_vs_cbs=[int(sub["flowtime"][done & proven].sum()), int(opt["flowtime"][done & proven].sum())],
                solved_only_by_ecbs=int((done & ~solved).sum()), solved_by_ecbs_not_proven_by_cbs=int((done & ~proven).sum()))


ECBS_WIDE_SHAPES = (dict(name="wide_65x65_n100", C=32, size=65, N=100, density=0.1, seed=105),
                    dict(name="wide_160x160_n1000", C=4, size=160, N=1000, density=0.1, seed=106))


def ecbs_wide_row(sh, args):
    import torch
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import ecbs_cases_wide, solve_cases
    m, start, goal = mr.random_batch(sh["seed"], sh["C"], sh["size"], sh["size"], sh["N"], sh["density"])
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m, start, goal)]
    full = solve_cases(*d, retries=8, wide=True, improve=IMPROVE["iterations"])
    T = full["paths"].shape[2]
    out = dict(shape=sh["name"] + "_ecbs_wide", cases=sh["C"], agents=sh["N"], T=T, **ECBS)
    need = int(nat.lib().magat_sim_mapf_ecbs_wide_workspace_bytes(sh["C"], sh["size"], sh["size"], sh["N"], T, ECBS["max_nodes"], ECBS["levels"]))
    out.update(workspace_bytes=need)
    if need > torch.cuda.mem_get_info()[0] * 9 // 10:
        out.update(measured=False, why="the workspace does not fit the free device memory")
        return out
    run = lambda: ecbs_cases_wide(*d, horizon=T, **ECBS)      # noqa: E731
    t0 = time.perf_counter()
    sub = run()
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0
    if first_s > 20.0:      # one call is all there is time for: the host clock around it, the code object's load included
        out.update(warmup=0, calls=1, ecbs_ms_median=first_s * 1e3, ecbs_ms_min=first_s * 1e3, ecbs_ms_max=first_s * 1e3)
    else:
        warmup, calls = (0, min(args.calls, 3)) if first_s > 1.0 else (args.warmup, args.calls)
        ms, sub = timed(run, warmup, calls)
        out.update(warmup=warmup, calls=calls, ecbs_ms_median=ms[len(ms) // 2], ecbs_ms_min=ms[0], ecbs_ms_max=ms[-1])
    done, solved = sub["status"] == 0, full["solved"] != 0
    flow = (full["lengths"] - 1).sum(1)
    have = done & (sub["lower_bound"] > 0)
    ratio = sub["flowtime"][have].double() / sub["lower_bound"][have].double()
    out.update(measured=True, solved=int(done.sum()), at_budget=int((sub["status"] == 1).sum()), no_schedule=int((sub["status"] >= 2).sum()),
               horizon_hit=int((sub["horizon_hit"] != 0).sum()), nodes_mean=float(sub["nodes"].float().mean()),
               ratio_mean=float(ratio.mean()) if have.any() else None, ratio_max=float(ratio.max()) if have.any() else None,
               solved_by_solve_cases=int(solved.sum()),
               flowtime_ecbs_vs_solve_cases_improved=[int(sub["flowtime"][done & solved].sum()), int(flow[done & solved].sum())],
               solved_only_by_ecbs=int((done & ~solved).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--restatement", type=int, default=0, help="time the Python restatement on this many cases per shape")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    args = ap.parse_args()
    for sh in SHAPES:
        if args.shapes and sh["name"] not in args.shapes.split(","):
            continue
        m, start, goal = mr.random_batch(sh["seed"], sh["C"], sh["size"], sh["size"], sh["N"], sh["density"])
        out = dict(shape=sh["name"], cases=sh["C"], agents=sh["N"], T=sh["T"])
        if not args.no_device:
            import torch
            from magat_pathplanning_amd import plan_prioritized, solve_cases
            assert torch.cuda.is_available(), "mapf_bench needs a GPU (no fallback)"
            d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (m, start, goal)]
            wide = sh.get("wide", False)
            t0 = time.perf_counter()
            res = plan_prioritized(*d, horizon=sh["T"], wide=wide)
            torch.cuda.synchronize()
            slow = time.perf_counter() - t0 > 1.0      # (the first call of a process also loads the code object)
            warmup, calls = (1, min(args.calls, 5)) if slow else (args.warmup, args.calls)
            out.update(warmup=warmup, calls=calls)
            ms, res = timed(lambda: plan_prioritized(*d, horizon=sh["T"], wide=wide), warmup, calls)
            t0 = time.perf_counter()
            full = solve_cases(*d, horizon=sh["T"], retries=8, wide=wide)
            torch.cuda.synchronize()
            solve_ms = (time.perf_counter() - t0) * 1e3
            solved = full["solved"] != 0
            out.update(plan_ms_median=ms[len(ms) // 2], plan_ms_min=ms[0], plan_ms_max=ms[-1],
                       plan_us_per_case=ms[len(ms) // 2] * 1e3 / sh["C"], solved_first_try=float(res["solved"].float().mean()),
                       solved_after_retries=float(solved.float().mean()), rounds_max=int(full["rounds"].max()),
                       solve_cases_ms_host_clock=solve_ms, makespan_max_solved=int(full["makespan"][solved].max()))
        if args.restatement:
            k = min(args.restatement, sh["C"])
            t0 = time.perf_counter()
            ref = mr.plan_batch(m, start[:k], goal[:k], None, sh["T"])
            sec = time.perf_counter() - t0
            out.update(restatement_cases=k, restatement_cpu_s=sec, restatement_cpu_s_per_case=sec / k,
                       restatement_solved_first_try=float(ref["solved"].mean()))
        print(json.dumps(out), flush=True)
        if not args.no_device:
            print(json.dumps(improve_row(sh, d, full, args)), flush=True)
            print(json.dumps(audit_row(sh, d, full, args)), flush=True)
            if not sh.get("wide", False):
                print(json.dumps(cbs_row(sh, d, full, args)), flush=True)
                print(json.dumps(ecbs_row(sh, d, full, args)), flush=True)
    for sh in ECBS_WIDE_SHAPES:
        if args.no_device or (args.shapes and sh["name"] + "_ecbs_wide" not in args.shapes.split(",")):
            continue
        print(json.dumps(ecbs_wide_row(sh, args)), flush=True)


if __name__ == "__main__":
    main()
