"""The dense graph layer's dispatch on the CPU: csrc/gat_route.h (compiled for the host by tools/host_wave/gat_route_check.cpp)
against the independent restatement of tests/gat_route_restatement.py over a grid of shapes, batch sizes, flags and options; and
the literals of the admission conditions occur in no csrc/gat_*.hip outside kernel bodies.  No GPU needed."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
import gat_route_restatement as rr

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
OPT_ORDER = ("GAT_MFMA", "GAT_SPLIT", "RANGE_GUARD", "GAT_WIDE_FROM", "GAT_PACK", "GAT_CHUNK_MB")
ROUTE_ORDER = ("form", "cls", "pack", "hsplit", "persist", "grid", "guard", "rerun_grid", "maps", "prepare", "slim", "ztiles",
               "all_fused", "head_mean", "book", "NC", "ldz", "chunk", "nchunks", "threads", "lds")
ENUMS = dict(form=rr.FORMS, guard=rr.GUARDS, maps=rr.MAPS, book=rr.BOOKS)
FLAGS = ("pack", "hsplit", "persist", "prepare", "slim", "ztiles", "all_fused", "head_mean")
WIDTHS = (16, 32, 64, 128, 256, 48)       # 48: a width without kernels
MODES = (0, 1, 2, 3, 4, 7)                # the five modes (GNN is refused by this entry) and one out of range
BATCHES = (1, 3, 16, 17, 511, 512, 4096)
EDGES = (1, 16, 17, 32, 33, 64, 65, 96, 97, 102, 103, 105, 106, 110, 128, 129)      # every N at which a class or a form changes
SMALL_CHUNK_MB = 1                        # 8 instances per chunk at the wide shapes: B = 17 is 8 + 8 + 1


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "gat_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "gat_route_check.cpp"), "-o", exe], check=True)
    return exe


def _variants():
    """each option at every other value, each flag flipped and each build / device fact changed, the rest at their defaults; then
    the pairs a single flip cannot reach"""
    base = dict(opt=dict(rr.DEFAULT_OPT), attention=False, y_aligned=True, tail=False, tail_cout=0, tail_k=0, conv_direct=True,
                cus=256, f_other=False, tail_m_off=0)
    out = [base]
    for name, values in (("GAT_MFMA", (0,)), ("GAT_SPLIT", (0,)), ("RANGE_GUARD", (0,)), ("GAT_WIDE_FROM", (0, 106, 129)),
                         ("GAT_PACK", (0, 2)), ("GAT_CHUNK_MB", (SMALL_CHUNK_MB,))):
        for v in values:
            out.append(dict(base, opt=dict(rr.DEFAULT_OPT, **{name: v})))
    out.append(dict(base, attention=True))
    out.append(dict(base, y_aligned=False))
    out.append(dict(base, tail=True, tail_cout=5, tail_k=128 + 128))           # the action head behind a skip-concat layer
    out.append(dict(base, tail=True, tail_cout=4, tail_k=128))                 # not the five-output head: not taken along
    out.append(dict(base, tail=True, tail_cout=5, tail_k=128, tail_m_off=1))   # not this layer's rows
    out.append(dict(base, tail=True, tail_cout=5, tail_k=4096))                # weights beyond 64 KB
    out.append(dict(base, conv_direct=False))
    out.append(dict(base, cus=64))
    out.append(dict(base, f_other=True))
    # the two-launch form in several chunks: without the guard, with the attention tensor, and as the re-run
    out.append(dict(base, opt=dict(rr.DEFAULT_OPT, GAT_CHUNK_MB=SMALL_CHUNK_MB, RANGE_GUARD=0, GAT_MFMA=0)))
    out.append(dict(base, opt=dict(rr.DEFAULT_OPT, GAT_CHUNK_MB=SMALL_CHUNK_MB), attention=True))
    out.append(dict(base, opt=dict(rr.DEFAULT_OPT, GAT_PACK=2), cus=64))
    return out


def _point(B, N, G, K, P, mode, concat, v):
    return dict(B=B, N=N, G=G, F=G // 2 if v["f_other"] else G, K=K, P=P, mode=mode, concat=concat, attention=v["attention"],
                y_aligned=v["y_aligned"], tail=v["tail"], tail_cout=v["tail_cout"], tail_m=B * N + v["tail_m_off"], tail_k=v["tail_k"],
                opt=v["opt"], conv_direct=v["conv_direct"], cus=v["cus"])


def grid():
    """The issue's axes as two products, no point of either left out:
      - shapes: every N of 1 .. 129 x every width x K x P x every mode x concat x B in {1, 17, 512}, defaults otherwise;
      - options, flags, build and device facts (one at a time, plus four pairs) x every batch size x the N at which a class or a
        form changes x the widths with kernels above 16 x K in {2, 3} x P x {KeyQuery, GAT_modified, GAT_Similarity} x concat;
      - and a call with each dimension in turn at zero."""
    vs = _variants()
    pts = [_point(B, N, G, K, P, mode, concat, vs[0])
           for N, G, K, P, mode, concat, B in itertools.product(range(1, 130), WIDTHS, (1, 2, 3), (1, 4), MODES, (0, 1), (1, 17, 512))]
    pts += [_point(B, N, G, K, P, mode, concat, v)
            for v, B, N, G, K, P, mode, concat in itertools.product(vs[1:], BATCHES, EDGES, (32, 64, 128, 256), (2, 3), (1, 4),
                                                                    (0, 1, 4), (0, 1))]
    for dim in ("B", "N", "G", "F", "K", "P"):
        pts.append(dict(_point(3, 10, 32, 2, 4, 0, 1, vs[0]), **{dim: 0}))
    return pts


def _line(i):
    v = [i["B"], i["N"], i["G"], i["F"], i["K"], i["P"], i["mode"], i["concat"], i["attention"], i["y_aligned"], i["tail"],
         i["tail_cout"], i["tail_m"], i["tail_k"], *(i["opt"][k] for k in OPT_ORDER), i["conv_direct"], i["cus"]]
    assert len(v) == 22
    return " ".join(str(int(x)) for x in v)


def _want(r):
    if r["refusal"] != "none":
        return (rr.REFUSALS.index(r["refusal"]),)
    head = tuple(ENUMS[k].index(r[k]) if k in ENUMS else int(r[k]) for k in ROUTE_ORDER)
    return (0,) + head + tuple(r.get("first", (0,) * 5)) + tuple(r.get("last", (0,) * 5))


@pytest.fixture(scope="module")
def walked(route_check):
    points = grid()
    run = subprocess.run([route_check], input="\n".join(_line(p) for p in points) + "\n", check=True, capture_output=True, text=True)
    got = [tuple(int(x) for x in l.split()) for l in run.stdout.strip().split("\n")]
    return points, [rr.route(p) for p in points], got


def test_route_header_equals_the_restatement_over_the_grid(walked):
    points, want, got = walked
    assert len(got) == len(points) > 300000
    bad = []
    for p, w, g in zip(points, want, got):
        ww = _want(w)
        if w["refusal"] == "none" and w["form"] != "two_launch" and w["guard"] not in ("two", "slim"):
            g = g[:len(ROUTE_ORDER) + 1] + (0,) * 10      # (no chunk loop: the per-chunk figures mean nothing)
        if ww != g and len(bad) < 5:
            bad.append((p, ww, g))
    assert not bad, bad


def test_the_restatement_alone_reaches_every_value(walked):
    """every refusal the dispatcher can answer before a launch, every value of every enum of the Route, both values of every
    flag, every size class, a short last chunk, heads per workgroup 1 and P, and the capped grids"""
    _, want, _ = walked
    assert {w["refusal"] for w in want} == set(rr.REFUSALS)
    ok = [w for w in want if w["refusal"] == "none"]
    for k, names in ENUMS.items():
        assert {w[k] for w in ok} == set(names), k
    for k in FLAGS:
        assert {bool(w[k]) for w in ok} == {False, True}, k
    assert {w["cls"] for w in ok if w["form"] == "one_mfma"} == {0, 1, 2}
    assert {w["form"] for w in ok if w["hsplit"]} == {"one_mfma", "one_mid"}
    chunked = [w for w in ok if "first" in w]
    assert any(w["nchunks"] >= 3 and w["last"][0] < w["first"][0] for w in chunked)
    assert {w["first"][1] for w in chunked} == {1, 4}
    assert any(w["first"][2] == 256 for w in chunked) and any(w["first"][2] == 128 and w["guard"] == "two" for w in chunked)
    assert any(w["guard"] == "one_tail" and w["rerun_grid"] > 1 for w in ok)


def test_exports_say_what_the_route_says():
    """magat_gat_dense_supported / magat_gat_one_launch_supported against the restatement, every N and width (library present)"""
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    for N, G in itertools.product(range(0, 131), WIDTHS):
        assert bool(lib.magat_gat_dense_supported(N, G, G)) == rr.dense_supported(N, G, G), (N, G)
        assert not lib.magat_gat_dense_supported(N, G, G // 2)
        for K, mode in itertools.product((1, 2, 3), MODES):
            assert bool(lib.magat_gat_one_launch_supported(N, G, G, K, mode, 1)) == \
                rr.one_launch_supported(N, G, G, K, mode, rr.DEFAULT_OPT), (N, G, K, mode)


def _host_code(text):
    """the source without comments and without the bodies of __global__ / __device__ functions"""
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out, pos = [], 0
    for m in re.finditer(r"__global__|__device__", text):
        if m.start() < pos:
            continue
        semi, brace = text.find(";", m.end()), text.find("{", m.end())
        if brace < 0 or (0 <= semi < brace):       # a declaration, or a __device__ variable
            continue
        depth, j = 1, brace + 1
        while depth:
            depth += {"{": 1, "}": -1}.get(text[j], 0)
            j += 1
        out.append(text[pos:m.start()])
        pos = j
    out.append(text[pos:])
    return "".join(out)


def test_admission_literals_live_in_the_header_only():
    names = sorted(n for n in os.listdir(CSRC) if n.startswith("gat_") and n.endswith(".hip"))
    assert {"gat_f32.hip", "gat_mfma.hip", "gat_small.hip", "gat_mid.hip"} <= set(names)
    for name in names:
        host = _host_code(open(os.path.join(CSRC, name)).read())
        assert "160 * 1024" not in host and "GAT_RERUN_SMALL_UNITS" not in host, name
        assert not re.findall(r"\bN\s*<=\s*(?:32|64|102|105|128)\b", host), name
        for gone in ("magat_gat_mfma_supported", "magat_gat_small_supported", "magat_gat_mid_supported", "wide_ok"):
            assert gone not in host, (name, gone)
    header = open(os.path.join(CSRC, "gat_route.h")).read()
    assert "160 * 1024" in header and "kRerunSmallUnits = 64" in header
    # the CU count is asked for once per call: by the dispatcher, not by the one-launch files
    counts = {n: open(os.path.join(CSRC, n)).read().count("hipDeviceAttributeMultiprocessorCount")
              for n in ("gat_f32.hip", "gat_mfma.hip", "gat_small.hip", "gat_mid.hip")}
    assert counts == {"gat_f32.hip": 1, "gat_mfma.hip": 0, "gat_small.hip": 0, "gat_mid.hip": 0}, counts
