"""The large-batch form of the one-launch chain kernel (option CHAIN_TILE16): layer3.conv2 on 18 half tiles of 16 rows
(v_mfma_f32_16x16x32_f16, csrc/block_walk.h walk16) instead of nine 32-row tiles.  Another MFMA shape sums a product's k values
in another order, so this form is NOT bit-identical to the 32-row form: it is held against the oracle at the north star's gate,
against the strict float32 encoder with the 32-row form's own distance as the yardstick, and the form counter says which one
ran.  Below the threshold, and with the option off, nothing changes bit for bit.  Agent counts: one group, a partial group, an
agent tile (128) crossed, and a second trip through the persistent loop with a partial last group."""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _build(cfg, sd, device):
    from magat_pathplanning_amd import DecentralPlannerGATNet
    cfg.device = str(device)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval()


def _split(M):
    """M agents as B instances of N <= 128 agents."""
    N = next(n for n in range(128, 0, -1) if M % n == 0)
    return M // N, N


def _cases(device):
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return [8, 13, 129, 8 * cus + 11]


def _forward(net, x, S):
    net.addGSO(S.clone())
    out = net(x).clone()
    M = x.shape[0] * x.shape[1]
    feat = net._buf("feat", (M, net.numFeatureMap), x.device).clone()
    return out, feat


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_tile16_form_against_oracle_float32_and_the_32_row_form(gpu_device, libopt, case):
    """Forced 16-row form (CHAIN_TILE16 = 1; LAT_AGENTS = 0 keeps few agents on the eight-agent-group kernel) with both layouts
    of the pooled map (row-major for the split-K head, granule-major for the long-K head, HEAD_SPLITK = 0): logits within 1e-4 of
    the oracle; the encoder's feature rows at most twice as far from the strict float32 encoder (CONV_SPLIT = 0) as the 32-row
    form's are - both are roundings of the same sums in another order.  (The pooled map itself stays inside the encoder's
    workspace; the feature rows are the head's linear image of it.)  With the option off and under auto below the threshold the
    32-row form runs: form counter 0, logits equal bit for bit."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    M = _cases(gpu_device)[case]
    B, N = _split(M)
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=17 + case)
    net = _build(cfg, sd, gpu_device)
    x = fov_states(B, N, seed=3 + case).to(gpu_device)
    S = comm_gso(B, N, 50, seed=4 + case).to(gpu_device)
    ref = orc.planner_forward(x.cpu(), S.cpu().clone(), sd, cfg)
    lib = nat.lib()
    f16 = nat.FORMS["chain_tile16"]
    libopt.set("MAGAT_LAT_AGENTS", 0)
    with torch.no_grad():
        _forward(net, x, S)                              # (the first forward folds the activation scales)
        libopt.set("MAGAT_CONV_SPLIT", 0)
        _, feat32 = _forward(net, x, S)
        libopt.reset("MAGAT_CONV_SPLIT")
        for splitk in (None, 0):
            if splitk is not None:
                libopt.set("MAGAT_HEAD_SPLITK", splitk)
            libopt.set("MAGAT_CHAIN_TILE16", 0)
            lib.magat_form_reset()
            old, feat_old = _forward(net, x, S)
            assert lib.magat_form_count(f16) == 0
            libopt.set("MAGAT_CHAIN_TILE16", 1)
            new, feat_new = _forward(net, x, S)
            assert lib.magat_form_count(f16) == 1
            d_old = float((feat_old - feat32).abs().max())
            d_new = float((feat_new - feat32).abs().max())
            e_new = float((new.cpu() - ref).abs().max())
            print("M=%d head_splitk=%s: |feat - float32| 32-row %.3e, 16-row %.3e; |logits - oracle| 16-row %.3e, 32-row %.3e"
                  % (M, splitk, d_old, d_new, e_new, float((old.cpu() - ref).abs().max())))
            assert torch.isfinite(new).all()
            assert e_new <= TOL
            assert d_new <= 2.0 * d_old
            if M < 10240:
                libopt.set("MAGAT_CHAIN_TILE16", 2)      # auto: below the threshold the 32-row form
                lib.magat_form_reset()
                auto, _ = _forward(net, x, S)
                assert lib.magat_form_count(f16) == 0
                assert torch.equal(auto, old)
    st = net.range_status()
    assert not st["encoder_rerun"] and not st["gat_rerun"], st


def test_tile16_form_is_chosen_on_the_global_agent_count(gpu_device):
    """Default options, 10 400 agents (above the threshold of 10 240): the 16-row form runs.  The two halves of the batch, each below the
    threshold on its own, run with form_agents = the global count: they take the same form and concatenate to the whole batch's
    logits bit for bit."""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states, make_config
    B, N = 104, 100
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=4, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=5)
    net = _build(cfg, sd, gpu_device)
    x = fov_states(B, N, seed=1).to(gpu_device)
    S = comm_gso(B, N, 50, seed=2).to(gpu_device)
    lib = nat.lib()
    f16 = nat.FORMS["chain_tile16"]
    with torch.no_grad():
        net.addGSO(S.clone())
        net(x)
        lib.magat_form_reset()
        net.addGSO(S.clone())
        whole = net(x).clone()
        assert lib.magat_form_count(f16) == 1
        net.form_agents = B * N
        lib.magat_form_reset()
        parts = []
        for b0, b1 in ((0, 52), (52, B)):
            net.addGSO(S[b0:b1].contiguous())
            parts.append(net(x[b0:b1]).clone())
        net.form_agents = 0
        assert lib.magat_form_count(f16) == 2
    assert torch.equal(torch.cat(parts), whole)
    ref = orc.planner_forward(x[:2].cpu(), S[:2].cpu().clone(), sd, cfg)
    assert float((whole[:2 * N].cpu() - ref).abs().max()) <= TOL


def test_tile16_range_guard_rerun(gpu_device, libopt, monkeypatch):
    """layer2 / layer3 maps ~1e5 with the activation scales off: the 16-row form raises the encoder's flag (conv1's split epilogue
    is the same code) and the predicated float32 re-run produces the logits."""
    from magat_pathplanning_amd import _native as nat
    from test_gpu_range import _run, _scaled_model
    monkeypatch.setenv("MAGAT_ACT_SCALE", "0")
    libopt.set("MAGAT_LAT_AGENTS", 0)
    libopt.set("MAGAT_CHAIN_TILE16", 1)
    cfg, sd, net = _scaled_model(gpu_device, 1.0e5, where="layer2")
    lib = nat.lib()
    lib.magat_form_reset()
    got, ref = _run(net, cfg, sd, gpu_device)
    assert lib.magat_form_count(nat.FORMS["chain_tile16"]) == 1
    st = net.range_status()
    assert st["encoder_rerun"], st
    assert float((got - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


def test_tile16_nan_stays_with_its_agent(gpu_device, libopt):
    """A NaN in one agent's state map: that agent's logits are non-finite as in the reference, every other planning instance keeps
    its parity (the pattern of test_gpu_range.test_non_finite_inputs_are_not_clamped_into_finite_numbers on the 16-row form)."""
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    from oracle import magat_oracle as orc
    from test_gpu_range import _scaled_model
    libopt.set("MAGAT_LAT_AGENTS", 0)
    libopt.set("MAGAT_CHAIN_TILE16", 1)
    cfg, sd, net = _scaled_model(gpu_device, 1.0, where="stem")
    B, N = 4, 20
    x, S = fov_states(B, N, seed=5), comm_gso(B, N, 28, seed=6)
    lib = nat.lib()
    with torch.no_grad():
        net.addGSO(S.clone().to(gpu_device))
        net(x.to(gpu_device))
    x[2, 7, 1, 4, 6] = float("nan")
    ref = orc.planner_forward(x, S.clone(), sd, cfg).view(B, N, 5)
    lib.magat_form_reset()
    with torch.no_grad():
        net.addGSO(S.clone().to(gpu_device))
        got = net(x.to(gpu_device)).cpu().view(B, N, 5)
    assert lib.magat_form_count(nat.FORMS["chain_tile16"]) == 1
    assert torch.isfinite(got[2, 7]).all() == torch.isfinite(ref[2, 7]).all(), (got[2, 7], ref[2, 7])
    keep = [0, 1, 3]
    assert torch.isfinite(got[keep]).all()
    assert float((got[keep] - ref[keep]).abs().max()) <= 1e-4
