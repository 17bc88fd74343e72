"""The CSR graph layer's routes on the GPU: for every case of tests/gat_csr_route_cases.py the launches are predicted from
tests/gat_csr_route_restatement.py (the restatement csrc/gat_csr_route.h is held against on the CPU) and compared with what the
library did - launch counts per profiling tag, the form counters, the return code, the three workspace exports - and the rows are
held against the float64 oracle at the gates these kernels already have (tests/large_graph_cases.py): y 2e-5 of max(1, |want|)
(or four times the float32 composite's own error), the attention as in tests/test_gpu_large_graph.py, bf16 storage at its budgets
(the fused form against the oracle's emulation of its own order, tests/test_gpu_csr_fused.py), training tensors 2e-4.

The tiled and the per-edge kernels share one profiling tag: which of the two ran is pinned by the host test
(tests/test_host_gat_csr_route.py, against large_graph_cases.tiled_route too), not here - both are run and both must be right."""
import pytest
import torch

import gat_csr_route_cases as cc
import gat_csr_route_restatement as cr
import large_graph_cases as lg
import similarity_train_cases as sc
from test_gpu_large_graph import _check_values
from test_gpu_train_graph_shapes import _device_pass

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", list(cc.INFER))
def test_inference_launches_are_the_predicted_ones(gpu_device, libopt, tag_counts, cid):
    case = cc.Infer(cid, gpu_device)
    k, r = case.k, case.r
    seen = set()
    for csc, opts in k.variants:
        opt = cc.set_options(libopt, opts)
        i = cc.route_input(k, case.nnz, csc, opt, gpu_device)
        route, tags, forms = cc.predicted(i)
        assert cc.workspace_exports(i) == cc.workspace_restated(i), (cid, csc, opts)
        got = case.run(csc, tag_counts)
        assert (got["tags"], got["forms"]) == (tags, forms), (cid, csc, opts, got["tags"], got["forms"], tags, forms)
        what = "%s %s" % ("column view" if csc else "in-call transpose", opts)
        if route["fused"]:
            ref, scale = r.want["y"], float(r.want["y"].abs().max())
            e_emul, e_ref = float((got["y"].cpu() - r.emul_fused).abs().max()) / scale, float((got["y"].cpu().double() - ref).abs().max()) / scale
            a_err = float((got["att"].cpu().double() - r.want["att"]).abs().max())
            print("%s [fused, %s]: y %.2e of scale against the emulation, %.2e against float64, attention %.2e" % (cid, what, e_emul, e_ref, a_err))
            assert e_emul <= lg.BF16_EMUL and e_ref <= lg.BF16_FP32 and a_err <= lg.BF16_FP32
        else:
            _check_values(cid, r, got["y"], got["att"], what)
        seen.add((route["fused"], route["scores"], route["hop_kind"], route["k1"], route["hop_buffers"], route["transpose"]))
    libopt.restore()
    if k.bf16 and k.G == 128:
        assert {s[0] for s in seen} == {False, True}
    if k.N == 8:
        assert {s[1:3] for s in seen} == {("tiled", "tiled"), ("edge", "edge"), ("tiled", "edge"), ("edge", "tiled")}


def test_the_matrix_reaches_every_decision(gpu_device):
    """the predictions over all cases: both graph kernel kinds for scores and hops, every place of the K = 1 launch, no / one / two
    hop buffers and K = 5, the transposition in the call and not, the head mean, every maps kind, the fused form, cosine scores"""
    routes = []
    for cid, k in cc.INFER.items():
        for csc, opts in k.variants:
            routes.append(cr.route(cc.route_input(k, 100, csc, dict(cr.DEFAULT_OPT, **opts), gpu_device)))
    routes += [cr.route(cc.route_input(k, 100, False, cr.DEFAULT_OPT, gpu_device, "train_cos" if k.mode == lg.SIM else "train"))
               for k in cc.TRAIN.values()]
    assert all(r["refusal"] == "none" for r in routes)
    for key, values in (("scores", cr.GRAPHS), ("hop_kind", cr.GRAPHS), ("k1", cr.K1S), ("maps", cr.MAPS), ("hop_buffers", (0, 1, 2)),
                        ("hops", (0, 1, 2, 3, 4))):
        assert {r[key] for r in routes} == set(values), key
    for flag in ("fused", "prepare", "cos_train_note", "transpose", "transpose_booked", "head_mean", "act_relu"):
        assert {bool(r[flag]) for r in routes} == {False, True}, flag
    assert any(r["transpose"] and not r["transpose_booked"] for r in routes)


@pytest.mark.parametrize("cid", list(cc.TRAIN))
def test_training_forward_launches_are_the_predicted_ones(gpu_device, tag_counts, cid):
    """magat_gat_train_forward_f32 / _cos_f32 called directly: launches, form counter and return code as predicted, the kept rows
    and attention values against float64; then forward + backward through the module, y, dx and every parameter gradient."""
    case = cc.Train(cid, gpu_device)
    k, r = case.k, case.r
    route, tags, forms = cc.predicted(cc.route_input(k, case.nnz, False, cr.DEFAULT_OPT, gpu_device, "train_cos" if case.cos else "train"))
    got = case.run(tag_counts)
    assert (got["rc"], got["rc_backward"]) == (cr.OK, cr.OK)
    assert (got["tags"], got["forms"]) == (tags, forms), (cid, got["tags"], got["forms"], tags, forms)
    assert ("T" in got["tensors"]) == (k.K > 2)
    y_err = lg.y_error(case.y_of(got["tensors"]["Ypre"]), r.want["y"])
    a_abs, a_sum, _ = lg.attention_errors(got["tensors"]["att"][:, :case.nnz].t(), r.want["att"], r.rowid, k.B * k.N)
    print("%s: y %.2e  attention %.2e, row sums %.2e" % (cid, y_err, a_abs, a_sum))
    assert y_err <= lg.TRAIN_GATE and a_abs <= lg.ATT_ABS and a_sum <= lg.ATT_SUM
    case.layer.addGSO(r.S.unsqueeze(1).to(gpu_device))
    node = "_GatCosTrainFunctionBackward" if case.cos else "_GatTrainFunctionBackward"
    passes = [_device_pass(case.layer, r, gpu_device, node) for _ in range(2)]
    sc.compare(cid, passes[0], {n: t for n, t in r.want.items() if n != "att"}, r.clamped, gate=lg.TRAIN_GATE, again=passes[1])


def test_refused_calls_answer_the_predicted_code_and_launch_nothing(gpu_device, tag_counts):
    """every refusal of the route through the C entries, the workspace check in front of the one that is answered behind it, and
    with them every return code a shape can earn: MAGAT_ERR_BAD_SHAPE, MAGAT_ERR_UNSUPPORTED, MAGAT_ERR_WORKSPACE"""
    ring = cc.Ring(gpu_device)
    codes = set()
    for name, entry, change, workspace in cc.refusal_calls():
        rc, launched, i = ring.call(entry, change, workspace, tag_counts)
        route = cr.route(i)
        assert route["refusal"] == name, (name, entry, route["refusal"])
        assert rc == cr.return_code(route, workspace) != cr.OK and launched == 0, (name, entry, rc, launched)
        codes.add(rc)
    assert codes == {cr.BAD_SHAPE, cr.UNSUPPORTED, cr.WORKSPACE}
    assert {name for name, _, _, _ in cc.refusal_calls()} == set(cr.REFUSALS)
    assert bool((ring.Y == -7.0).all()) and not ring.ws.any() and not ring.scratch.any()
