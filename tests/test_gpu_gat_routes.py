"""The dense graph layer's routes on the GPU: for every case the launches are predicted from tests/gat_route_restatement.py (the same
restatement csrc/gat_route.h is held against on the CPU) and compared with what the library did - launch counts per profiling tag
and the magat_form_count counters - and the rows are held against the float64 oracle at the gates of the existing graph-layer
tests: 1e-5 max(1, |y|) (tests/test_gpu_gat_mid.py, tests/test_gpu_similarity.py), attention 2e-6 (tests/test_gpu_kernels.py),
and for inputs that clamp 1e-4 of each instance's scale (tests/test_gpu_range.py, whose inputs they are).  The reference is
computed once per configuration; the options do not change it."""
import pytest
import torch

import gat_route_cases as grc
import gat_route_restatement as rr

pytestmark = pytest.mark.gpu


def _err(y, ref):
    return float((y.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("shape", grc.SHAPES, ids=[grc.shape_id(s) for s in grc.SHAPES])
def test_launches_are_the_predicted_ones(gpu_device, libopt, tag_counts, shape):
    failures, seen = [], set()
    for c in grc.configs(shape):
        case = grc.Case(c, gpu_device)
        for opts in grc.OPTION_SETS:
            libopt.restore()
            for k, v in opts.items():
                libopt.set("MAGAT_" + k, v)
            route = rr.route(case.call_input(opts))
            got = case.run(tag_counts)
            what = (grc.config_id(c), opts)
            bad = grc.mismatches(route, got)
            if bad:
                failures.append((what, bad, got["tags"], got["forms"]))
            elif route["refusal"] == "none":
                e = _err(got["y"], case.ref)
                print(what, route["form"], route["guard"], "err %.3g" % e)
                if e > 1e-5:
                    failures.append((what, "oracle", e))
            seen.add((route["refusal"], route.get("form"), route.get("guard")))
    libopt.restore()
    assert not failures, failures
    if shape == (256, grc.N256 + 1):
        assert seen == {("tiles", None, None)}, seen
    if shape == (128, 128):
        assert ("none", "one_mid", "slim") in seen or ("none", "one_mid", "one") in seen, seen


def test_every_form_guard_and_counter_was_walked(gpu_device):
    """the matrix hides no route: the predictions over all cases reach every form, every guard, every maps kind and each counter"""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    routes = []
    for shape in grc.SHAPES:
        for c in grc.configs(shape):
            for opts in grc.OPTION_SETS:
                i = dict(B=c["B"], N=c["N"], G=c["G"], F=c["G"], K=c["K"], P=c["P"], mode=c["mode"], concat=c["concat"],
                         attention=False, y_aligned=True, tail=False, tail_cout=0, tail_m=0, tail_k=0,
                         opt=dict(rr.DEFAULT_OPT, **opts), conv_direct=True, cus=cus)
                routes.append(rr.route(i))
    ok = [r for r in routes if r["refusal"] == "none"]
    assert {r["form"] for r in ok} == set(rr.FORMS)
    assert {r["guard"] for r in ok} >= {"none", "one", "two"}       # (one_tail and slim: the cases below)
    assert {r["maps"] for r in ok} == set(rr.MAPS)
    assert {r["cls"] for r in ok if r["form"] == "one_mfma"} == {0, 1, 2}
    for flag in ("pack", "hsplit", "persist", "prepare", "head_mean", "ztiles"):
        assert {bool(r[flag]) for r in ok} == {False, True}, flag
    assert any(r["nchunks"] == 3 for r in ok)


@pytest.mark.parametrize("G,N,mode", [(128, 20, rr.KEYQUERY), (32, 40, rr.KEYQUERY), (128, 100, rr.GAT_MODIFIED), (64, 12, rr.GAT_ORIGIN)])
def test_attention_requested_takes_the_two_launch_form(gpu_device, tag_counts, G, N, mode):
    c = dict(G=G, N=N, mode=mode, B=3, P=4, K=3, concat=1)
    case = grc.Case(c, gpu_device)
    route = rr.route(case.call_input({}, attention=True))
    assert route["form"] == "two_launch"
    got = case.run(tag_counts, attention=True)
    assert not grc.mismatches(route, got), (got["tags"], got["forms"])
    assert _err(got["y"], case.ref) <= 1e-5
    assert float((got["att"].double().reshape(-1) - case.aij.double().reshape(-1)).abs().max()) <= 2e-6


@pytest.mark.parametrize("G,N,B", [(128, 10, 3), (64, 20, 3), (32, 100, 2), (128, 104, 2), (128, 110, 2)])
def test_y_at_an_odd_column_offset(gpu_device, tag_counts, G, N, B):
    """the one-launch kernels store 16-byte pieces: the two-launch form takes such a call - beyond its tiles it is refused"""
    c = dict(G=G, N=N, mode=rr.KEYQUERY, B=B, P=4, K=2, concat=1)
    case = grc.Case(c, gpu_device)
    route = rr.route(case.call_input({}, odd=True))
    assert route["refusal"] == ("tiles" if N == 110 else "none") and route.get("form", "two_launch") == "two_launch"
    got = case.run(tag_counts, odd=True)
    assert not grc.mismatches(route, got), (got["rc"], got["tags"], got["forms"])
    if N != 110:
        assert _err(got["y"], case.ref) <= 1e-5


CLAMP = [("one", dict(G=128, N=10, mode=rr.KEYQUERY, B=1, P=4, K=3, concat=1), False),
         ("one_tail", dict(G=128, N=10, mode=rr.KEYQUERY, B=1, P=4, K=3, concat=1), True),
         ("two", dict(G=64, N=100, mode=rr.KEYQUERY, B=17, P=4, K=2, concat=0), False),
         ("slim", dict(G=128, N=110, mode=rr.KEYQUERY, B=17, P=4, K=3, concat=1), False)]


@pytest.mark.parametrize("guard,c,tail", CLAMP, ids=[g for g, _, _ in CLAMP])
def test_each_rerun_form_does_the_work_when_the_input_clamps(gpu_device, tag_counts, guard, c, tail):
    """An input beyond the f16 planes' range (every seventh instance, as tests/test_gpu_range.py builds it) behind each form of the
    guard's re-run: the predicted launches, the flag raised and the re-run counted once, and the float32 rows - every instance's -
    within 1e-4 of the instance's scale."""
    case = grc.Case(c, gpu_device, clamp=True)
    route = rr.route(case.call_input({}, tail=True if tail else None))
    assert route["guard"] == guard, route
    got = case.run(tag_counts, tail=tail)
    assert not grc.mismatches(route, got), (got["tags"], got["forms"])
    assert got["status"] == (1, 1), got["status"]
    B, N = c["B"], c["N"]
    y, ref = got["y"].double().view(B, N, -1), case.ref.view(B, N, -1)
    assert bool(torch.isfinite(y).all())
    scale = ref.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1.0)
    err = float(((y - ref).abs() / scale).max())
    print(guard, "err %.3g" % err)
    assert err <= 1e-4, err
    if tail:
        assert got["tail_done"] == 1
        W, b = case.tail_w
        logits = case.ref @ W.t() + b
        assert float((got["logits"].double() - logits).abs().max()) <= 1e-4 * max(1.0, float(logits.abs().max()))
