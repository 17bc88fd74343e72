"""The CSR graph layer's dispatch on the CPU: csrc/gat_csr_route.h (compiled for the host by
tools/host_wave/gat_csr_route_check.cpp) against the independent restatement of tests/gat_csr_route_restatement.py, field by
field, over a grid of shapes, batch sizes, flags, options and passes; the restatement against large_graph_cases.tiled_route; the
header's constants against graphml's.  No GPU needed."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
import gat_csr_route_restatement as cr
import large_graph_cases as lg

NS = (1, 3, 7, 8, 9, 128, 129, 1023, 1024, 1025, 8190, 8191)
WIDTHS = ((16, 16), (32, 32), (64, 64), (128, 128), (256, 256), (48, 48), (32, 64), (128, 16), (30, 32))    # 48: no kernels; G != F
MODES = (0, 1, 2, 3, 4, 7)                 # every mode, GraphFilterBatch among them, and one out of range
EDGES = (1, 7, 8, 1024, 1025, 8190, 8191)     # the N at which a decision flips
BATCHES = (1, 8, 9, 4096, 1 << 20)         # 2^20 instances: beyond an int in B N and in the hop grid at 8190 agents
BOOLS = ("have_csc", "attention", "edge_vals", "y_f32", "x_aligned")
ENUMS = dict(maps=cr.MAPS, scores=cr.GRAPHS, k1=cr.K1S, hop_kind=cr.GRAPHS)
FLAGS = ("fused", "prepare", "cos_train_note", "transpose", "transpose_booked", "head_mean", "act_relu")
ROUTE_ORDER = ("fused", "maps", "prepare", "cos_train_note", "transpose", "transpose_booked", "scores", "k1", "hops", "hop_kind",
               "hop_buffers", "head_mean", "act_relu", "NC") + cr.GRIDS


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "gat_csr_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "gat_csr_route_check.cpp"), "-o", exe], check=True)
    return exe


def _point(B, N, G, F, K, P, mode, concat, esz, pas, v):
    width = P * F if concat else F
    return dict(B=B, N=N, nnz=v["nnz"], G=G, F=F, K=K, P=P, mode=mode, concat=concat, ldy=width + v["ldy_off"], esz=esz,
                have_csc=v["have_csc"], attention=v["attention"], edge_vals=v["edge_vals"], y_f32=v["y_f32"], x_aligned=v["x_aligned"],
                opt=v["opt"], cus=v["cus"], **{"pass": pas})


def _variants():
    """the defaults; each flag flipped, ldy too small and not a multiple of 4, no edges, each option at every other value, other CU
    counts; then the pairs a single flip cannot reach"""
    base = dict(nnz=1000, ldy_off=0, have_csc=False, attention=False, edge_vals=True, y_f32=False, x_aligned=True,
                opt=dict(cr.DEFAULT_OPT), cus=256)
    out = [base]
    out += [dict(base, **{b: not base[b]}) for b in BOOLS]
    out += [dict(base, ldy_off=-4), dict(base, ldy_off=2), dict(base, ldy_off=8), dict(base, nnz=0), dict(base, nnz=0, edge_vals=False)]
    out += [dict(base, opt=dict(cr.DEFAULT_OPT, CSR_TILED=t)) for t in (0, 1, 2)]
    out += [dict(base, have_csc=True, opt=dict(cr.DEFAULT_OPT, CSR_FUSED=f), cus=c) for f, c in ((0, 256), (1, 64), (1, 4), (1, 304))]
    out += [dict(base, have_csc=True, attention=True, y_f32=True),
            dict(base, attention=True, opt=dict(cr.DEFAULT_OPT, CSR_TILED=0)),
            dict(base, attention=True, opt=dict(cr.DEFAULT_OPT, CSR_TILED=2)),
            dict(base, x_aligned=False, ldy_off=-4)]
    return out


def grid():
    """The issue's axes as two products, no point of either left out:
      - shapes: every N x every width pair x K 1..5 x P 1..4 x every mode x concat x storage type x pass x B in {1, 9}, defaults
        otherwise (float32 storage only for the training passes: they have no other);
      - flags, ldy, nnz, options and CU counts (one at a time, plus the pairs of _variants) x every batch size x the N at which a decision flips x the widths
        32 and 128 x K x P in {1, 2, 4} x {KeyQuery, GAT_origin, GraphFilterBatch, GAT_Similarity} x concat x storage type, inference
        (the training passes read none of the flags) - and the batch sizes x N x K once more for the training passes;
      - and a call of every pass with each dimension in turn at zero, nnz at -1."""
    vs = _variants()
    pts = [_point(B, N, G, F, K, P, mode, concat, esz, pas, vs[0])
           for N, (G, F), K, P, mode, concat, (esz, pas), B in itertools.product(
               NS, WIDTHS, range(1, 6), range(1, 5), MODES, (0, 1), ((4, "infer"), (2, "infer"), (4, "train"), (4, "train_cos")), (1, 9))]
    pts += [_point(B, N, G, G, K, P, mode, concat, esz, "infer", v)
            for v, B, N, G, K, P, mode, concat, esz in itertools.product(vs[1:], BATCHES, EDGES, (32, 128), range(1, 6), (1, 2, 4),
                                                                         (0, 2, 3, 4), (0, 1), (4, 2))]
    pts += [_point(B, N, G, G, K, P, mode, 1, 4, pas, vs[0])
            for B, N, G, K, P, mode, pas in itertools.product(BATCHES, NS, (16, 128), range(1, 6), (1, 4), (0, 1, 2, 3), cr.PASSES)]
    for pas, dim in itertools.product(cr.PASSES, ("B", "N", "G", "F", "K", "P")):
        pts.append(dict(_point(3, 10, 32, 32, 2, 4, 0, 1, 4, pas, vs[0]), **{dim: 0}))
    pts += [dict(_point(3, 10, 32, 32, 2, 4, 0, 1, 4, pas, vs[0]), nnz=-1) for pas in cr.PASSES]
    return pts


def _line(i):
    v = [i["B"], i["N"], i["nnz"], i["G"], i["F"], i["K"], i["P"], i["mode"], i["concat"], i["ldy"], i["esz"], *(i[b] for b in BOOLS),
         cr.PASSES.index(i["pass"]), i["opt"]["CSR_TILED"], i["opt"]["CSR_FUSED"], i["cus"]]
    assert len(v) == 20
    return " ".join(str(int(x)) for x in v)


def _want(r):
    head = (cr.REFUSALS.index(r["refusal"]), {cr.OK: 0, cr.BAD_SHAPE: 1, cr.UNSUPPORTED: 2}[cr.CODES[r["refusal"]]])
    if r["refusal"] not in ("none", "bf16_maps"):
        return head
    return head + tuple(ENUMS[k].index(r[k]) if k in ENUMS else int(r[k]) for k in ROUTE_ORDER) + tuple(r["ws"][k] for k in cr.WS_ORDER)


@pytest.fixture(scope="module")
def walked(route_check):
    points = grid()
    run = subprocess.run([route_check], input="\n".join(_line(p) for p in points) + "\n", check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    consts = tuple(int(x) for x in lines[0].split())
    return points, [cr.route(p) for p in points], [tuple(int(x) for x in l.split()) for l in lines[1:]], consts


def test_route_header_equals_the_restatement_over_the_grid(walked):
    points, want, got, _ = walked
    assert len(got) == len(points) > 500000
    bad = [(p, _want(w), g) for p, w, g in zip(points, want, got) if _want(w) != g]
    assert not bad, (len(bad), bad[:5])


def test_the_restatement_alone_reaches_every_value(walked):
    """every refusal and every return code, every value of every enum of the Route, both values of every flag, zero, one and two
    hop buffers, the fused form's grids capped by the CU count and not, a grid beyond an int in inference"""
    points, want, _, _ = walked
    assert {w["refusal"] for w in want} == set(cr.REFUSALS)
    assert {cr.return_code(w) for w in want} == {cr.OK, cr.BAD_SHAPE, cr.UNSUPPORTED}
    ok = [w for w in want if w["refusal"] == "none"]
    for k, names in ENUMS.items():
        assert {w[k] for w in ok} == set(names), k
    for k in FLAGS:
        assert {bool(w[k]) for w in ok} == {False, True}, k
    assert {w["hop_buffers"] for w in ok} == {0, 1, 2}
    assert {w["hops"] for w in ok} == {0, 1, 2, 3, 4}
    for pas in cr.PASSES:
        assert {w["refusal"] for p, w in zip(points, want) if p["pass"] == pas} >= {"none", "dims", "mode", "shape", "agents"}, pas
    fused = [(p, w) for p, w in zip(points, want) if w["refusal"] == "none" and w["fused"]]
    assert {p["P"] for p, _ in fused} == {1, 2, 4}
    assert any(w["grid_fused_scores"] == p["cus"] // 8 * 8 for p, w in fused) and any(w["grid_fused_scores"] == 8 for p, w in fused)
    assert any(w["grid_fused_hop"] == 2 * w["grid_fused_scores"] for _, w in fused)       # (two head pairs, few items)
    assert any(w["grid_hop"] > cr.INT_MAX for w in ok)
    assert any(w["transpose"] and not w["transpose_booked"] for w in ok)
    assert any(w["ws"]["total"] > w["ws"]["xhat"] for w in ok) and all(w["ws"]["xhat"] > w["ws"]["order"] for _, w in fused)


def test_tiled_route_of_the_large_graph_cases_agrees():
    """large_graph_cases.tiled_route (what the inference tests take their expectations from) against the restatement, every case of
    that file under every value of CSR_TILED"""
    modes = {lg.KQ: cr.KQ, lg.GM: cr.GAT_MODIFIED, lg.GO: cr.GAT_ORIGIN, lg.GNN: cr.GNN, lg.SIM: cr.SIMILARITY}
    assert (lg.TILED_MIN_N, lg.TILED_MAX_N, lg.MAX_N) == (8, 1024, cr.MAX_N)
    seen = set()
    for (cid, k), opt in itertools.product(lg.CASES.items(), range(4)):
        i = dict(B=k.B, N=k.N, nnz=5 * k.N, G=k.G, F=k.F, K=k.K, P=k.P, mode=modes[k.mode], concat=int(k.concat) if k.mode != lg.GNN else 1,
                 ldy=lg.out_width(k), esz=2 if k.bf16 else 4, have_csc=False, attention=bool(k.att), edge_vals=True, y_f32=False,
                 x_aligned=True, opt=dict(cr.DEFAULT_OPT, CSR_TILED=opt), cus=256, **{"pass": "infer"})
        r = cr.route(i)
        assert r["refusal"] == "none", cid
        want = lg.tiled_route(opt, k.mode, k.N, k.G, k.F, k.K, k.bf16, k.att)
        assert want == (r["scores"] == "tiled", r["hop_kind"] == "tiled"), (cid, opt)
        seen.add(want)
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_constants_of_the_python_layer_are_the_headers(walked):
    from magat_pathplanning_amd import graphml
    consts = walked[3]
    assert graphml._COS_TRAIN_MAX_N == consts[0] == cr.MAX_N
    assert tuple(graphml._COS_TRAIN_WIDTHS) == consts[1:]


def test_literals_stand_in_the_header_only():
    csrc = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
    for name in ("gat_csr_f32.hip", "gat_csr_fused.hip", "gat_train.hip"):
        text = open(os.path.join(csrc, name)).read()
        for gone in ("8190;", "0x7fffffff", "MAGAT_CSR_DISPATCH", "nnz < 0", "hipDeviceAttributeMultiprocessorCount",
                     "magat_gat_csr_fused_supported"):
            assert gone not in text, (name, gone)
    header = open(os.path.join(csrc, "gat_csr_route.h")).read()
    assert "kCsrMaxN = 8190" in header and "#include <hip" not in header and "magat_common.h" not in header
