"""Does the dense graph layer compute the same bits, through the same launches, under two builds of the library?
  python tools/gat_ab.py LIB_A LIB_B [OUT_DIR]
One fresh child process per library (MAGAT_LIB_PATH set for it) runs the case matrix of tests/gat_route_cases.py under every
option set, the attention, odd-offset and clamping cases of tests/test_gpu_gat_routes.py, and writes per entry the return code, the
SHA-256 of Y (of the attention tensor and of the tail's logits where there are any), the status words, the launch counts per
profiling tag and the form counters.  The parent compares the two files entry by entry and exits non-zero on any difference: these
kernels are deterministic."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import conftest
    import gat_route_cases as grc
    import test_gpu_gat_routes as tgr
    from magat_pathplanning_amd import _native as nat
    dev, tag_counts = torch.device("cuda:0"), conftest._TagCounts
    res = {}

    def options(opts):
        for name in grc.rr.DEFAULT_OPT:
            nat.reset_option("MAGAT_" + name)
        for k, v in opts.items():
            nat.set_option("MAGAT_" + k, int(v))

    def record(key, got):
        res[key] = dict(rc=got["rc"], y=_sha(got["y"]), att=_sha(got["att"]), logits=_sha(got["logits"]), status=got["status"],
                        tail_done=got["tail_done"], tags=got["tags"], forms=got["forms"])

    for shape in grc.SHAPES:
        for c in grc.configs(shape):
            case = grc.Case(c, dev, want_ref=False)
            for opts in grc.OPTION_SETS:
                options(opts)
                record("%s %s %s" % (grc.shape_id(shape), grc.config_id(c), json.dumps(opts, sort_keys=True)), case.run(tag_counts))
    options({})
    for G, N, mode in ((128, 20, 0), (32, 40, 0), (128, 100, 1), (64, 12, 2)):
        case = grc.Case(dict(G=G, N=N, mode=mode, B=3, P=4, K=3, concat=1), dev, want_ref=False)
        record("attention G%d N%d mode %d" % (G, N, mode), case.run(tag_counts, attention=True))
    for G, N, B in ((128, 10, 3), (64, 20, 3), (32, 100, 2), (128, 104, 2), (128, 110, 2)):
        case = grc.Case(dict(G=G, N=N, mode=0, B=B, P=4, K=2, concat=1), dev, want_ref=False)
        record("odd column offset G%d N%d" % (G, N), case.run(tag_counts, odd=True))
    for guard, c, tail in tgr.CLAMP:
        case = grc.Case(c, dev, clamp=True, want_ref=False)
        record("clamping input, re-run %s" % guard, case.run(tag_counts, tail=tail))
        assert res["clamping input, re-run %s" % guard]["status"] == (1, 1)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def main(lib_a, lib_b, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for name, path in (("a", lib_a), ("b", lib_b)):
        out = os.path.join(out_dir, "gat_ab_%s.json" % name)
        env = dict(os.environ, MAGAT_LIB_PATH=os.path.abspath(path))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, timeout=900)
        files.append(out)
    a, b = (json.load(open(f)) for f in files)
    bad = 0
    print("A = %s\nB = %s" % (os.path.relpath(lib_a, ROOT), os.path.relpath(lib_b, ROOT)))
    for key in sorted(set(a) | set(b)):
        same = a.get(key) == b.get(key)
        bad += not same
        print("%s  %s" % ("same     " if same else "DIFFERENT", key))
        if not same:
            print("    A: %s\n    B: %s" % (json.dumps(a.get(key), sort_keys=True), json.dumps(b.get(key), sort_keys=True)))
    routes = sorted({json.dumps([v["rc"], v["tags"], v["forms"]], sort_keys=True) for v in a.values()})
    print("%d entries, %d different; %d distinct (return code, launch counts, form counters) among them" % (len(set(a) | set(b)), bad, len(routes)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) in (3, 4):
        sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) == 4 else "."))
    else:
        sys.exit(__doc__)
