"""Generates tests/golden/gnnbn_*.npz: fixtures of the bottleneck GNN planners made by the REAL reference (its own
graphs/models/decentralplanner_bottleneck{,_SkipConcat,_SkipConcatGNN,_SkipAddGNN}.py classes, imported from the reference
tree through oracle/_ref_import.py; build machine only).  TEST INFRASTRUCTURE.

    python tools/make_golden_gnn_bottleneck.py         # rewrites every gnnbn_* fixture (bit-reproducible)

Same layout as the gnnmodel_* fixtures (oracle/make_golden.py main_gnn_model): x (uint8 state maps), S (the GSO handed to
addGSO), S_after (the caller's tensor after addGSO), logits, cfg, sd/<state_dict key>.  The floating-point parameters are
rounded to bfloat16-representable float32 values before the forward (the files stay under 1 MB with the ResNet trunks; the
values are still the reference's weights, exactly).  skipAddGNN: its state_dict only, plus forward_raises = "TypeError" -
the reference's forward raises there (decentralplanner_bottleneck_SkipAddGNN.py:311).
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle._ref_import import import_reference, make_config  # noqa: E402
from oracle.make_golden import OUT, fov_states, tricky_gso  # noqa: E402

FILES = {"BottomNeck_only": "decentralplanner_bottleneck",
         "BottomNeck_skipConcat": "decentralplanner_bottleneck_SkipConcat",
         "BottomNeck_skipConcatGNN": "decentralplanner_bottleneck_SkipConcatGNN",
         "BottomNeck_skipAddGNN": "decentralplanner_bottleneck_SkipAddGNN"}

# name, config, batch, S float64, keep the NaN entry of tricky_gso (False: replaced by a finite value)
CASES = [
    ("only_large_mlp_k2", dict(bottleneckMode="BottomNeck_only", CNN_mode="ResNetLarge_withMLP", numInputFeatures=32,
                               bottleneckFeature=32, nGraphFilterTaps=2, num_agents=10), 2, True, True),
    ("skipconcat_default_one_k3", dict(bottleneckMode="BottomNeck_skipConcat", CNN_mode="Default", bottleneckFeature=32,
                                       nGraphFilterTaps=3, num_agents=12, GSO_mode="dist_GSO_one"), 2, True, True),
    ("skipconcatgnn_slim_dropout_k2", dict(bottleneckMode="BottomNeck_skipConcatGNN", CNN_mode="ResNetSlim",
                                           numInputFeatures=32, bottleneckFeature=32, nGraphFilterTaps=2, num_agents=9,
                                           use_dropout=True), 2, True, True),
    ("skipconcat_f128_n64_k3", dict(bottleneckMode="BottomNeck_skipConcat", CNN_mode="ResNetSlim", bottleneckFeature=128,
                                    nGraphFilterTaps=3, num_agents=64), 1, False, False),
    ("skipconcatgnn_slim_mlp_k3", dict(bottleneckMode="BottomNeck_skipConcatGNN", CNN_mode="ResNetSlim_withMLP",
                                       numInputFeatures=64, bottleneckFeature=32, nGraphFilterTaps=3, num_agents=11), 2,
     False, True),
]


def reference_class(mode):
    import_reference()
    return importlib.import_module("graphs.models." + FILES[mode]).DecentralPlannerNet


def build_model(cfg, seed):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    model = reference_class(cfg.bottleneckMode)(cfg).eval()
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.2, generator=gen)
                mod.running_var.uniform_(0.5, 1.5, generator=gen)
                mod.bias.normal_(0, 0.1, generator=gen)
        for t in list(model.parameters()) + list(model.buffers()):
            if t.is_floating_point():
                t.copy_(t.to(torch.bfloat16).float())
    return model, gen


def case_fixture(name, kw, B, f64, keep_nan, seed):
    cfg = make_config(**kw)
    model, gen = build_model(cfg, seed)
    N = cfg.num_agents
    x = fov_states(gen, B, N)
    S = tricky_gso(gen, B, N, 0.3 if N <= 20 else 0.08, f64)
    if not keep_nan:
        S[torch.isnan(S)] = 0.25
    S_in = S.clone()
    model.addGSO(S)
    with torch.no_grad():
        logits = model(x)
    out = dict(x=x.numpy().astype(np.uint8), S=S_in.numpy(), S_after=S.numpy(), logits=logits.numpy(),
               cfg=np.array(repr(vars(cfg))))
    for k, v in model.state_dict().items():
        out["sd/" + k] = v.numpy()
    return out


def skipadd_fixture(seed):
    cfg = make_config(bottleneckMode="BottomNeck_skipAddGNN", CNN_mode="Default", bottleneckFeature=32, nGraphFilterTaps=2,
                      num_agents=6)
    model, gen = build_model(cfg, seed)
    x = fov_states(gen, 1, cfg.num_agents)
    S = tricky_gso(gen, 1, cfg.num_agents, 0.3, True)
    model.addGSO(S)
    raised = "none"
    try:
        with torch.no_grad():
            model(x)
    except TypeError:
        raised = "TypeError"
    assert raised == "TypeError", "the reference's SkipAddGNN forward was expected to raise TypeError"
    out = dict(cfg=np.array(repr(vars(cfg))), forward_raises=np.array(raised))
    for k, v in model.state_dict().items():
        out["sd/" + k] = v.numpy()
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for i, (name, kw, B, f64, keep_nan) in enumerate(CASES):
        fx = case_fixture(name, dict(kw), B, f64, keep_nan, seed=12121 + 7 * i)
        path = os.path.join(OUT, "gnnbn_%s.npz" % name)
        np.savez_compressed(path, **fx)
        print("wrote", path, os.path.getsize(path) // 1024, "KB", "NaN logits: %d rows" % int(np.isnan(fx["logits"]).any(1).sum()))
    path = os.path.join(OUT, "gnnbn_skipaddgnn_state_only.npz")
    np.savez_compressed(path, **skipadd_fixture(13131))
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
