"""The case matrix of the encoder's routes on the GPU, shared by tests/test_gpu_encoder_routes.py (launch counts against the
restatement, results against the float64 oracle) and tools/encoder_ab.py (the same cases, bit for bit, under two builds of the
library): the smallest shapes at which a route can go wrong."""
import ctypes

import torch

import encoder_route_restatement as rr

MODELS = [("ResNetLarge_withMLP", 128), ("ResNetLarge_withMLP", 16), ("ResNetSlim_withMLP", 128), ("ResNetLarge", 128)]
# (B, N, ENC_CHUNK or None, form_agents)
SIZES = [(1, 10, None, 0),          # latency form with the stem inside
         (15, 10, None, 0),         # a partial 128-agent tile, batched forms, split-K head
         (3, 100, 128, 0),          # three chunks, the last one short: the latency chain per chunk, without its stem and its guard
         (1, 10, None, 6400)]       # a shard of a large batch: batched forms for a few agents
OPTION_SETS = [{}, {"RANGE_GUARD": 0}, {"HEAD_F16": 0}, {"CONV_SPLIT": 0}, {"HEAD_COMPRESS": 0}, {"L1_FUSED": 1}, {"HEAD_SPLITK": 0},
               {"BLOCK_FUSED": 1}, {"BLOCK_FUSED": 0}, {"CONV_PCHAIN": 0}, {"L1_FUSED": 0}, {"LAT_AGENTS": 0}]


def model_id(m):
    return "%s_b%d" % m


def size_id(s):
    return "%dx%d%s%s" % (s[0], s[1], "_chunk%d" % s[2] if s[2] else "", "_form%d" % s[3] if s[3] else "")


def build(cnn, bneck, N, device, seed):
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import DecentralPlannerGATNet
    from magat_pathplanning_amd.synthetic import make_config
    cfg = make_config(num_agents=N, nGraphFilterTaps=3, nAttentionHeads=2, CNN_mode=cnn, bottleneckFeature=bneck,
                      numInputFeatures=bneck, bottleneckMode="BottomNeck_skipConcat")
    sd = orc.init_state_dict(cfg, seed=seed)
    cfg.device = str(device)
    net = DecentralPlannerGATNet(cfg)
    net.load_state_dict(sd, strict=True)
    return cfg, sd, net.to(device).eval()


def inputs(B, N, device):
    from magat_pathplanning_amd.synthetic import comm_gso, fov_states
    return fov_states(B, N, seed=N).to(device), comm_gso(B, N, 50, seed=N + 1)


def call_input(desc, M, opts, form_agents=0, comp=True, comp_bf16=False):
    """the restatement's input for one magat_encoder_forward_f32 call with this descriptor (an _native.EncoderDesc)"""
    from magat_pathplanning_amd import encoder as enc
    off = desc.off
    opt = dict(rr.DEFAULT_OPT)
    opt.update({k: v for k, v in opts.items() if k in opt})
    return dict(variant=desc.variant, H=desc.H, W=desc.W, n_feat=desc.n_feat, n_comp=desc.n_comp, form_agents=form_agents,
                f16=tuple(off[enc.slot_conv1_f16(l)] > 0 and off[enc.slot_conv2_f16(l)] > 0 for l in range(3)),
                permuted=off[enc.SLOT_PERMUTED] != 0, chain=desc.chain_off > 0, chain3=desc.chain3_off > 0,
                head16=desc.head16_off > 0, comp16=desc.comp16_off > 0, scaled=desc.scaled_off > 0, l1frag=desc.l1frag_off > 0,
                headfrag=desc.headfrag_off > 0, compfrag=desc.compfrag_off > 0, comp=comp, comp_bf16=comp_bf16, M=M, opt=opt,
                conv_direct=True, l1_lds=True, full_out_gl=True, buf_floats=rr.buf_floats_per_agent(desc.variant, desc.H, desc.W))


def read_forms(lib, nat):
    return {k: int(lib.magat_form_count(nat.FORMS[k])) for k in rr.ENCODER_FORMS}


def mismatches(call, enc_chunk, counts, forms):
    """-> list of (what, predicted, seen): the library's launches against the restatement's.  Where compressMLP is attempted in the
    head's epilogue the kernel may decline (CONV_BNFILL narrowed the head's column tile for a small batch): either outcome is
    accepted, chunk by chunk - a count moves between the tag "compressMLP" and the form "head_compress"."""
    tags, want_forms, maybe = rr.launches(call, enc_chunk or 65536)
    bad = []
    taken = forms["head_compress"]
    if not 0 <= taken <= maybe:
        bad.append(("head_compress", (0, maybe), taken))
    tags["compressMLP"] -= taken
    want_forms["head_compress"] = taken
    for k in rr.ENCODER_TAGS:
        if counts.get(k, 0) != tags[k]:
            bad.append((k, tags[k], counts.get(k, 0)))
    for k in rr.ENCODER_FORMS:
        if forms[k] != want_forms[k]:
            bad.append((k, want_forms[k], forms[k]))
    return bad


def run_forward(net, x, Sd, lib, nat, tag_counts):
    """one warm-up forward (the plan and the activation scales of the options at hand), the forward that gives the logits, then
    the planner's encoder call alone under the counters (the graph layer's guard shares the range_guard tag)
    -> (logits, tag counts, form counters, feat, comp)"""
    dev = x.device
    M = x.shape[0] * x.shape[1]
    with torch.no_grad():
        net.addGSO(Sd.clone())
        net(x)
        net.addGSO(Sd.clone())
        out = net(x).clone()
        xr = x.reshape(M, *x.shape[2:]).contiguous()
        lib.magat_form_reset()
        with tag_counts() as tc:
            feat, comp = net._run_encoder(net._rt, xr, M, dev, nat.current_stream(dev))
        forms = read_forms(lib, nat)
    return out, dict(tc.counts), forms, feat, comp


def off_size_case(device, hw=9, M=150, cnn="ResNetLarge"):
    """The encoder C entry on a 9 x 9 map (set-up of test_gpu_model.test_encoder_other_map_sizes): the row-band fused stem and the
    layer-by-layer chain.  -> (desc, x on the device, float64 reference, keep-alive)"""
    from oracle import magat_oracle as orc
    from magat_pathplanning_amd import _native as nat, encoder as enc
    from magat_pathplanning_amd.synthetic import make_config
    cfg = make_config(CNN_mode=cnn)
    sd = orc.init_state_dict(cfg, seed=23)
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(M, 3, hw, hw, generator=g) < 0.3).float() + 0.25 * torch.rand(M, 3, hw, hw, generator=g)
    ref = orc.resnet_forward(x.double(), {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}).flatten(1)
    pack, offs, meta = enc.fold_resnet(sd, hw, hw, "ConvLayers.0", None, None)
    packd = pack.to(device)
    d = nat.EncoderDesc()
    d.variant, d.H, d.W, d.n_feat, d.n_comp, d.pack = meta["variant"], hw, hw, meta["n_feat"], 0, packd.data_ptr()
    for i, o in enumerate(offs):
        d.off[i] = o
    return d, x.to(device), ref, packd


def run_entry(d, xd, device, lib, nat, tag_counts):
    M = xd.shape[0]
    ws = torch.zeros(lib.magat_encoder_workspace_bytes(ctypes.byref(d), M), dtype=torch.uint8, device=device)
    feat = torch.full((M, d.n_feat), float("nan"), device=device)
    lib.magat_form_reset()
    with tag_counts() as tc:
        nat.check(lib.magat_encoder_forward_f32(ctypes.byref(d), nat.ptr(xd), nat.ptr(feat), d.n_feat, None, 0, nat.ptr(ws), ws.numel(),
                                                M, nat.current_stream(device)), "encoder")
    return feat, dict(tc.counts), read_forms(lib, nat)
