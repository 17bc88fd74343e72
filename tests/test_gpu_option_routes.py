"""Routes of the planner that only open outside the default options or across calls: the encoder's latency form under every
option that changes its admission (one chain launch each time, never the latency chain AND the batched one), the step plan
after an option that grows the encoder's workspace, and weight swaps that bypass load_state_dict / the registration hooks.
Every case is held against the float64 oracle at the planner's gate."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
CHAIN = "layer1.conv2+layer2+layer3 (fused, pooled)"
CHAIN2 = ("layer1.conv2+layer2 (fused)", "layer3 (fused, pooled)")
LAYERWISE = ("layer1.conv2+ds", "layer2.conv1", "layer2.conv2+ds", "layer3.conv1", "layer3.conv2+ds")


def _one_chain(tc):
    """the BasicBlock chain ran exactly once, in one of its three forms: the fused chain (one launch), the two-launch chain
    (BLOCK_FUSED = 1; ResNetSlim's trunk: layer1.conv2 + layer2 only), or layer by layer (the strict-float32 form,
    CONV_SPLIT = 0: one launch per convolution; layer3 only in the trunks that have it)"""
    fused, two, layers = tc[CHAIN], [tc[t] for t in CHAIN2], [tc[t] for t in LAYERWISE]
    if fused:
        return fused == 1 and two == [0, 0] and layers == [0] * 5
    if any(two):
        return two[0] == 1 and two[1] <= 1 and layers == [0] * 5
    return layers[:3] == [1, 1, 1] and layers[3] == layers[4] <= 1


def _build(cfg, sd, device):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    cfg.device = str(device)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval()


def _gate(got, ref):
    return float((got.cpu().double() - ref.double()).abs().max()) <= TOL * max(1.0, float(ref.abs().max()))


OPTION_SETS = [{}, {"RANGE_GUARD": 0}, {"HEAD_F16": 0}, {"CONV_SPLIT": 0}, {"HEAD_COMPRESS": 0}, {"L1_FUSED": 1}]
MODELS = [("ResNetLarge_withMLP", 128), ("ResNetLarge_withMLP", 16), ("ResNetSlim_withMLP", 128)]


@pytest.mark.parametrize("cnn,bneck", MODELS, ids=["%s_b%d" % m for m in MODELS])
@pytest.mark.parametrize("B,N", [(1, 10), (3, 37)])
def test_latency_form_launches_the_chain_once(gpu_device, libopt, tag_counts, cnn, bneck, B, N):
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    lib = nat.lib()
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=2, CNN_mode=cnn, bottleneckFeature=bneck,
                      numInputFeatures=bneck, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=5 + N + bneck)
    net = _build(cfg, sd, gpu_device)
    x = fov_states(B, N, seed=N).to(gpu_device)
    S = comm_gso(B, N, 50, seed=N + 1)
    ref = orc.planner_forward(x.cpu(), S.clone(), sd, cfg)
    Sd = S.to(gpu_device)
    failures = []
    for opts in OPTION_SETS:
        libopt.restore()
        for k, v in opts.items():
            libopt.set(k, v)
        with torch.no_grad():
            net.addGSO(Sd.clone())
            net(x)                                      # (the plan and the activation scales of this option set)
            lib.magat_form_reset()
            with tag_counts() as tc:
                net.addGSO(Sd.clone())
                lat = net(x).clone()
            chain_lat = int(lib.magat_form_count(nat.FORMS["chain_lat"]))
            head_lat = int(lib.magat_form_count(nat.FORMS["head_lat"]))
            libopt.set("LAT_AGENTS", 0)
            if head_lat:
                # (the head rode in the chain's epilogue: its batched counterpart is the long-K head, as in test_gpu_latency;
                #  otherwise the same head form runs on both sides)
                libopt.set("HEAD_SPLITK", 0)
            lib.magat_form_reset()
            net.addGSO(Sd.clone())
            batched = net(x).clone()
            assert lib.magat_form_count(nat.FORMS["chain_lat"]) == 0
        what = (opts, tc.counts, chain_lat)
        if not _one_chain(tc):
            failures.append(("chain launches", what))
        default_model = cnn == "ResNetLarge_withMLP" and bneck == 128
        if chain_lat != (1 if tc[CHAIN] == 1 else 0) or (not opts and default_model and chain_lat != 1):
            failures.append(("chain_lat form", what))
        if not _gate(lat, ref):
            failures.append(("oracle", what, float((lat.cpu() - ref).abs().max())))
        if not torch.equal(lat, batched):
            failures.append(("latency != batched", what, float((lat - batched).abs().max())))
    assert not failures, failures


def test_step_plan_survives_an_option_that_grows_the_encoder_workspace(gpu_device, libopt):
    """The step plan holds the encoder workspace it was built with.  An option that grows the encoder's need after that
    (ENC_CHUNK: agents per encoder pass - the plan was built under a small chunk, the chunk then returns to its default) makes
    the encoder answer MAGAT_ERR_WORKSPACE: the plan is dropped and the general path, which resizes the workspace, gives the
    result.  (At a few-agent shape no option grows the need: the chunk is capped by the agent count, LAT_AGENTS does not enter
    it.  Graph workspace: no option grows it at this shape either - GAT_CHUNK_MB only caps the chunk of instances, and four
    instances of 100 agents are one chunk under the default cap - so only the encoder side is exercised here; the graph call's
    MAGAT_ERR_WORKSPACE takes the same branch of _plan_step.)"""
    import ctypes
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    lib = nat.lib()
    B, N = 4, 100
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=3)
    net = _build(cfg, sd, gpu_device)
    x = fov_states(B, N, seed=1).to(gpu_device)
    S = comm_gso(B, N, 50, seed=2).to(gpu_device)
    ref = orc.planner_forward(x.cpu(), S.cpu().clone(), sd, cfg)
    libopt.set("ENC_CHUNK", 128)
    with torch.no_grad():
        net.addGSO(S.clone())
        first = net(x).clone()
        net.addGSO(S.clone())
        net(x)
    rt = net._rt
    assert rt.plan is not None                          # the step plan is built and in use
    desc = ctypes.byref(rt.desc)
    before = lib.magat_encoder_workspace_bytes(desc, B * N)
    assert rt.ws.numel() >= before
    libopt.reset("ENC_CHUNK")
    after = lib.magat_encoder_workspace_bytes(desc, B * N)
    assert after > rt.ws.numel(), (before, after, rt.ws.numel())     # (so that the case below is not vacuous)
    with torch.no_grad():
        net.addGSO(S.clone())
        got = net(x).clone()
    assert _gate(got, ref)
    assert net._rt.ws.numel() >= after
    libopt.set("ENC_CHUNK", 128)                        # (the options the first forward ran under)
    with torch.no_grad():
        net.addGSO(S.clone())
        again = net(x).clone()
    assert torch.equal(again, first)
    libopt.restore()


def _swap_case(gpu_device, swap):
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    B, N = 1, 10
    cfg = make_config(num_agents=N, nGraphFilterTaps=2, nAttentionHeads=2, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=21)
    net = _build(cfg, sd, gpu_device)
    x = fov_states(B, N, seed=3).to(gpu_device)
    S = comm_gso(B, N, 50, seed=4).to(gpu_device)
    with torch.no_grad():
        for _ in range(2):                              # (the second forward runs through the step plan)
            net.addGSO(S.clone())
            old = net(x).clone()
    assert net._rt.plan is not None
    swap(net)
    new_sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    ref = orc.planner_forward(x.cpu(), S.cpu().clone(), new_sd, cfg)
    with torch.no_grad():
        net.addGSO(S.clone())
        got = net(x).clone()
    assert not torch.equal(got, old)
    assert _gate(got, ref), float((got.cpu() - ref).abs().max())


def test_parameter_replaced_in_the_dict_is_seen_at_once(gpu_device):
    def swap(net):
        lin = net.actionsMLP[0]
        g = torch.Generator().manual_seed(9)
        w = lin.weight.detach() + (torch.randn(lin.weight.shape, generator=g) * 0.05).to(lin.weight.device)
        lin._parameters["weight"] = torch.nn.Parameter(w)
    _swap_case(gpu_device, swap)


def test_submodule_conversion_with_overwritten_parameters_is_seen_at_once(gpu_device):
    def swap(net):
        prev = torch.__future__.get_overwrite_module_params_on_conversion()
        torch.__future__.set_overwrite_module_params_on_conversion(True)
        try:
            net.compressMLP.double()
            with torch.no_grad():
                net.compressMLP[0].weight.mul_(1.5)     # new values in the new tensors, not in the ones the plan was folded from
            net.compressMLP.float()
        finally:
            torch.__future__.set_overwrite_module_params_on_conversion(prev)
    _swap_case(gpu_device, swap)
