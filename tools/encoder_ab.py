"""Does the encoder compute the same bits, through the same launches, under two builds of the library?
  python tools/encoder_ab.py LIB_A LIB_B [OUT_DIR]
One fresh child process per library (MAGAT_LIB_PATH set for it) runs the case matrix of tests/encoder_route_cases.py, one case
whose checkpoint clamps (so that the range guard's re-run really computes: the scaled checkpoint of tests/test_gpu_range.py, in the
latency form and with LAT_AGENTS = 0), the off-size map at the C entry and calibrate(), and writes per entry the SHA-256 of feat,
comp, the logits and the absmax vector, the launch counts per profiling tag and the form counters.  The parent compares the two
files entry by entry and exits non-zero on any difference: these kernels are deterministic."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import conftest
    import encoder_route_cases as erc
    from magat_pathplanning_amd import _native as nat
    lib, dev, tag_counts = nat.lib(), torch.device("cuda:0"), conftest._TagCounts
    res = {}

    def options(opts, chunk=None):
        for name in list(erc.rr.DEFAULT_OPT) + ["ENC_CHUNK"]:
            nat.reset_option(name)
        if chunk:
            nat.set_option("ENC_CHUNK", chunk)
        for k, v in opts.items():
            nat.set_option(k, int(v))

    def record(key, net, x, Sd):
        out, counts, forms, feat, comp = erc.run_forward(net, x, Sd, lib, nat, tag_counts)
        res[key] = dict(logits=_sha(out), feat=_sha(feat), comp=_sha(comp), tags=counts, forms=forms,
                        status={k: v for k, v in net.range_status().items() if k.startswith("encoder")})

    for model in erc.MODELS:
        for size in erc.SIZES:
            (cnn, bneck), (B, N, chunk, form) = model, size
            _, _, net = erc.build(cnn, bneck, N, dev, seed=5 + N + bneck)
            net.form_agents = form
            x, S = erc.inputs(B, N, dev)
            for opts in erc.OPTION_SETS:
                options(opts, chunk)
                record("%s %s %s" % (erc.model_id(model), erc.size_id(size), json.dumps(opts, sort_keys=True)), net, x, S.to(dev))
    options({})
    # the off-size map at the C entry
    d, xd, _, _keep = erc.off_size_case(dev)
    feat, counts, forms = erc.run_entry(d, xd, dev, lib, nat, tag_counts)
    res["off-size 9x9"] = dict(feat=_sha(feat), tags=counts, forms=forms)
    # a checkpoint that clamps: the guard's float32 pass computes (inside the latency kernel; as the predicated re-run)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_range as tgr
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    os.environ["MAGAT_ACT_SCALE"] = "0"
    for opts in ({}, {"LAT_AGENTS": 0}):
        options(opts)
        _, _, net = tgr._scaled_model(dev, 1.0e4, where="stem")
        x, S = fov_states(4, 20, seed=5).to(dev), comm_gso(4, 20, 28, seed=6)
        key = "clamping checkpoint %s" % json.dumps(opts)
        record(key, net, x, S.to(dev))
        assert res[key]["status"]["encoder_rerun"], res[key]
    os.environ.pop("MAGAT_ACT_SCALE")
    options({})
    # calibrate(): the absmax vector of the float32 calibration pass and the exponents folded from it
    for model in erc.MODELS[:3]:
        _, _, net = erc.build(model[0], model[1], 10, dev, seed=3)
        scales = net.calibrate()
        res["calibrate %s" % erc.model_id(model)] = dict(absmax=_sha(torch.tensor(net._cal["absmax"], dtype=torch.float64)),
                                                         scales=json.dumps(scales, sort_keys=True, default=str))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


def main(lib_a, lib_b, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for name, path in (("a", lib_a), ("b", lib_b)):
        out = os.path.join(out_dir, "encoder_ab_%s.json" % name)
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
    routes = sorted({json.dumps([v.get("tags"), v.get("forms")], sort_keys=True) for v in a.values() if "tags" in v})
    print("%d entries, %d different; %d distinct (launch counts, form counters) among them" % (len(set(a) | set(b)), bad, len(routes)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) in (3, 4):
        sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) == 4 else "."))
    else:
        sys.exit(__doc__)
