"""Times ONE move step on the device through the two routes of the move step (csrc/sim_frontend.hip): the cell grid in LDS
(magat_sim_move) and in a device workspace (magat_sim_move_wide), both called directly, 8 instances of 1000 agents, density 0.1, random action keys.

    python tools/move_bench.py [--out FILE.json] [--reps 50]

    8 x 160 x 160   both routes (the LDS route takes it: 4 H W + 16 N = 118 KB; the wide entry is called directly)
    8 x 200 x 200   the wide route (176 KB: the LDS route refuses it)
Device events around `reps` calls after a warm-up; the median over 5 such windows, min and max next to it (tools/
guidance_bench.py's way).  Every call starts from the same positions: they are restored by a device copy inside the timed
window, in both routes alike."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from guidance_bench import scenario, windows
from magat_pathplanning_amd import _native as nat


def lds_call(m, pos, keys, out):
    B, N, _ = pos.shape
    H, W = m.shape
    nat.check(nat.lib().magat_sim_move(None, nat.ptr(keys), nat.ptr(m), 0, H, W, nat.ptr(pos), None, nat.ptr(out["a"]),
                                       nat.ptr(out["m"]), None, nat.ptr(out["f"]), B, N, nat.current_stream(pos.device)),
              "magat_sim_move")


def wide_call(m, pos, keys, out, ws):
    B, N, _ = pos.shape
    H, W = m.shape
    nat.check(nat.lib().magat_sim_move_wide(None, nat.ptr(keys), nat.ptr(m), 0, H, W, nat.ptr(pos), None, nat.ptr(out["a"]),
                                            nat.ptr(out["m"]), None, nat.ptr(out["f"]), B, N, nat.ptr(ws), ws.numel(),
                                            nat.current_stream(pos.device)), "magat_sim_move_wide")


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 50
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    B, N = 8, 1000
    result = dict(device=torch.cuda.get_device_name(0), B=B, N=N, density=0.1, reps=reps, rows=[])
    for size, routes in ((160, ("lds", "wide")), (200, ("wide",))):
        m, pos, _ = scenario(B, N, size, 0.1, seed=7)
        dm, start = torch.from_numpy(m).to(dev), torch.from_numpy(pos).to(dev)
        keys = torch.from_numpy(np.random.default_rng(3).integers(0, 5, (B, N)).astype(np.int32)).to(dev)
        cur = start.clone()
        out = dict(a=torch.empty(B, N, dtype=torch.int32, device=dev), m=torch.empty(B, N, 2, dtype=torch.int8, device=dev),
                   f=torch.empty(B, dtype=torch.int32, device=dev))
        ws = torch.empty(int(nat.lib().magat_sim_move_wide_workspace_bytes(B, size, size, N)), dtype=torch.uint8, device=dev)
        for route in routes:
            def call():
                cur.copy_(start)
                if route == "wide":
                    wide_call(dm, cur, keys, out, ws)
                else:
                    lds_call(dm, cur, keys, out)
            r = windows(call, reps)
            r.update(map=size, route=route)
            result["rows"].append(r)
            print("map %3d  %-4s  %8.3f ms / call  (min %.3f max %.3f)" % (size, route, r["median_ms"], r["min_ms"], r["max_ms"]),
                  flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
