"""Does the CSR graph layer compute the same bits, through the same launches, under two builds of the library?
  python tools/gat_csr_ab.py LIB_A LIB_B [OUT_DIR]
One fresh child process per library (MAGAT_LIB_PATH set for it) runs the case matrix of tests/gat_csr_route_cases.py - every
inference case under every variant (column view brought or not, options), the training cases through the C entries, the refused
calls - and writes per entry the return code, the SHA-256 of Y and of the attention values, the launch counts per profiling tag,
the form counters and the three workspace exports; for a training case the SHA-256 of Ypre, att, Z, T, dZ, dXd and datt.  The
parent compares the two files entry by entry and exits non-zero on any difference: these kernels are deterministic."""
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
    import gat_csr_route_cases as cc
    dev, tag_counts, libopt = torch.device("cuda:0"), conftest._TagCounts, conftest._LibOpt()
    res = {}
    for cid, k in cc.INFER.items():
        case = cc.Infer(cid, dev)
        for csc, opts in k.variants:
            opt = cc.set_options(libopt, opts)
            got = case.run(csc, tag_counts)
            res["%s csc=%d %s" % (cid, csc, json.dumps(opts, sort_keys=True))] = dict(
                rc=0, y=_sha(got["y"]), att=_sha(got["att"]), tags=got["tags"], forms=got["forms"],
                workspace=cc.workspace_exports(cc.route_input(k, case.nnz, csc, opt, dev)))
    libopt.restore()
    for cid in cc.TRAIN:
        got = cc.Train(cid, dev).run(tag_counts)
        res[cid] = dict(rc=got["rc"], rc_backward=got["rc_backward"], tags=got["tags"], forms=got["forms"],
                        **{name: _sha(t) for name, t in got["tensors"].items()})
    ring = cc.Ring(dev)
    for name, entry, change, workspace in cc.refusal_calls():
        rc, launched, _ = ring.call(entry, change, workspace, tag_counts)
        res["refused %s %s %s workspace=%d" % (name, entry, json.dumps(change, sort_keys=True), workspace)] = dict(rc=rc, launched=launched)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def main(lib_a, lib_b, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for name, path in (("a", lib_a), ("b", lib_b)):
        out = os.path.join(out_dir, "gat_csr_ab_%s.json" % name)
        env = dict(os.environ, MAGAT_LIB_PATH=os.path.abspath(path))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, env=env, timeout=600)
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
    routes = sorted({json.dumps([v.get("rc"), v.get("tags"), v.get("forms")], sort_keys=True) for v in a.values()})
    print("%d entries, %d different; %d distinct (return code, launch counts, form counters) among them" % (len(set(a) | set(b)), bad, len(routes)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) in (3, 4):
        sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) == 4 else "."))
    else:
        sys.exit(__doc__)
