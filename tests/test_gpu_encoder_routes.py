"""The encoder's routes on the GPU: for every case the launches are predicted from tests/encoder_route_restatement.py (the same
restatement csrc/encoder_route.h is held against on the CPU) and compared with what the library did - launch counts per profiling
tag and the magat_form_count counters - and the result is held against the float64 oracle at the planner's gate.  The oracle runs
once per (model, size); the options do not change it."""
import pytest
import torch

import encoder_route_cases as erc

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _gate(got, ref):
    return float((got.cpu().double() - ref.double()).abs().max()) <= TOL * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("size", erc.SIZES, ids=[erc.size_id(s) for s in erc.SIZES])
@pytest.mark.parametrize("model", erc.MODELS, ids=[erc.model_id(m) for m in erc.MODELS])
def test_launches_are_the_predicted_ones(gpu_device, libopt, tag_counts, model, size):
    """Where compressMLP is attempted in the head's epilogue (the long-K head: HEAD_SPLITK = 0, or form_agents above it) the
    kernel may decline - CONV_BNFILL narrows the head's column tile for a small batch - and the prediction accepts either
    outcome (encoder_route_cases.mismatches)."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    (cnn, bneck), (B, N, chunk, form) = model, size
    cfg, sd, net = erc.build(cnn, bneck, N, gpu_device, seed=5 + N + bneck)
    net.form_agents = form
    x, S = erc.inputs(B, N, gpu_device)
    ref = orc.planner_forward(x.cpu(), S.clone(), sd, cfg)
    Sd = S.to(gpu_device)
    failures, seen = [], set()
    for opts in erc.OPTION_SETS:
        libopt.restore()
        if chunk:
            libopt.set("ENC_CHUNK", chunk)
        for k, v in opts.items():
            libopt.set(k, v)
        out, counts, forms, _, _ = erc.run_forward(net, x, Sd, lib, nat, tag_counts)
        call = erc.call_input(net._rt.desc, B * N, opts, form_agents=form)
        bad = erc.mismatches(call, chunk, counts, forms)
        if bad:
            failures.append((opts, bad, counts, forms))
        if not _gate(out, ref):
            failures.append((opts, "oracle", float((out.cpu() - ref).abs().max())))
        seen.add((forms["chain_lat"], forms["stem_lat"], forms["guard_lat"], counts.get("range_guard", 0)))
    libopt.restore()
    assert not failures, failures
    if (cnn, bneck) == ("ResNetLarge_withMLP", 128) and chunk:
        # the route no other test walks: the latency chain per chunk, without its stem and its in-kernel guard, the re-run behind it
        assert (3, 0, 0, 1) in seen, seen
    if (cnn, bneck) == ("ResNetLarge_withMLP", 128) and (B, N, chunk, form) == (1, 10, None, 0):
        assert (1, 1, 1, 0) in seen, seen


def test_off_size_map_takes_the_band_stem_and_the_layerwise_chain(gpu_device, libopt, tag_counts):
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    d, xd, ref, _keep = erc.off_size_case(gpu_device)
    feat, counts, forms = erc.run_entry(d, xd, gpu_device, lib, nat, tag_counts)
    call = erc.call_input(d, xd.shape[0], {}, comp=False)
    assert not erc.mismatches(call, None, counts, forms), (counts, forms)
    assert counts.get("conv_first") == 1 and counts.get("layer1.conv1", 0) == 0 and counts.get("layer3.conv2+ds") == 1, counts
    err = float((feat.double().cpu() - ref).abs().max())
    assert err <= TOL * max(1.0, float(ref.abs().max())), err
