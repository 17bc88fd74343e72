"""Which kernel forms the ResNet encoders (variant 0 / 1) take, restated from DESIGN.md's encoder sections and the behaviour of
magat_encoder_forward_f32 / magat_encoder_calibrate_f32: one chunk of agents is walked from the stem to the bf16 rows, and every
decision is taken where the walk reaches it.  tests/test_host_encoder_route.py holds csrc/encoder_route.h against route();
tests/test_gpu_encoder_routes.py holds the library's launch counts against launches().

An input is a dict:
  variant H W n_feat n_comp form_agents          the descriptor's scalars
  f16 (3 bools) permuted chain chain3 head16 comp16 scaled l1frag headfrag compfrag      what the pack carries
  comp comp_bf16                                  the caller passed comp / desc.comp_bf16
  M mm                                            agents of the call / of the chunk
  pass                                            "forward" | "rerun" | "calibrate"
  opt                                             dict of CONV_SPLIT RANGE_GUARD CONV_PCHAIN L1_FUSED BLOCK_FUSED HEAD_SPLITK HEAD_F16
                                                  HEAD_COMPRESS LAT_AGENTS
  conv_direct l1_lds full_out_gl                  three facts about the build
  buf_floats                                      floats per agent of one activation buffer (buf_floats_per_agent)
"""
DEFAULT_OPT = dict(CONV_SPLIT=7, RANGE_GUARD=1, CONV_PCHAIN=1, L1_FUSED=2, BLOCK_FUSED=2, HEAD_SPLITK=5120, HEAD_F16=1,
                   HEAD_COMPRESS=1, LAT_AGENTS=512)
PASSES = ("forward", "rerun", "calibrate")
STEMS = ("plain", "band", "stem8", "lat")
CHAINS = ("layers", "two", "one", "lat")
HEADS = ("f32", "splitk", "longk", "lat")
COMPS = ("none", "f32", "chained", "f16", "lat")
GUARDS = ("none", "lat", "rerun")
BF16S = ("none", "cast", "epilogue")


def buf_floats_per_agent(variant, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return max(H * W * 32, Ho * Wo * (128 if variant == 0 else 64))


def chunk_agents(M, enc_chunk=65536):
    return min(max(enc_chunk, 128), M)


def route(i):
    o = i["opt"]
    large = i["variant"] == 0
    nblocks, clast = (3, 128) if large else (2, 64)
    Ho, Wo = (i["H"] - 1) // 2 + 1, (i["W"] - 1) // 2 + 1
    forward, rerun = i["pass"] == "forward", i["pass"] == "rerun"
    Mform = i["form_agents"] or i["M"]
    whole_call = i["mm"] == i["M"]

    # the split mask: only the forward pass uses split arithmetic, and only for blocks whose f16 planes the pack has
    split = sum(1 << l for l in range(3) if forward and o["CONV_SPLIT"] >> l & 1 and i["f16"][l])
    all_split = split == (1 << nblocks) - 1
    lay = 0
    if all_split and i["conv_direct"]:
        lay = 2 if i["permuted"] and o["CONV_PCHAIN"] else 1

    # stem
    fused_stem = lay == 2 and i["l1_lds"] and o["L1_FUSED"] >= 1
    groups_of_8 = fused_stem and (i["H"], i["W"]) == (11, 11) and i["l1frag"] and o["L1_FUSED"] >= 2
    maps6 = (Ho, Wo) == (6, 6)
    one_launch_chain = fused_stem and i["chain"] and maps6 and large and i["chain3"] and o["BLOCK_FUSED"] >= 2
    few = not rerun and Mform <= o["LAT_AGENTS"]
    head_inside = (one_launch_chain and few and i["headfrag"] and i["compfrag"] and i["n_feat"] == 128 and
                   i["n_comp"] in (32, 64, 128) and i["comp"] and split != 0 and bool(o["HEAD_F16"]))
    if one_launch_chain and few and head_inside and groups_of_8 and whole_call:
        stem = "lat"
    elif groups_of_8:
        stem = "stem8"
    elif fused_stem:
        stem = "band"
    else:
        stem = "plain"

    # chain
    pooled = False
    if one_launch_chain:
        chain, first, pooled = ("lat" if few else "one"), 3, True
    elif fused_stem and i["chain"] and maps6 and o["BLOCK_FUSED"] >= 1:
        chain, first = "two", 2
        if large and i["chain3"]:
            first, pooled = 3, True
    else:
        chain, first = "layers", 0

    # head
    cells = (Ho // 2) * (Wo // 2)
    fits = cells * i["n_feat"] <= i["buf_floats"]
    few_for_splitk = (forward and cells > 1 and Mform <= o["HEAD_SPLITK"] and clast % 4 == 0 and i["n_feat"] % 4 == 0 and fits)
    f16_head = (pooled and split != 0 and i["head16"] and clast % 32 == 0 and i["n_feat"] % 32 == 0 and bool(o["HEAD_F16"]))
    epilogue = False
    if chain == "lat" and head_inside:
        head = "lat"
    elif few_for_splitk:
        head = "splitk"
    elif f16_head:
        head = "longk"
        epilogue = bool(i["comp"] and i["n_comp"] == 128 and i["n_feat"] == 128 and i["comp16"] and o["HEAD_COMPRESS"])
    else:
        head = "f32"
    head_gl = bool(one_launch_chain and f16_head and not few_for_splitk and i["conv_direct"] and i["full_out_gl"])

    # compressMLP when the head did not take it along (for an attempted epilogue: what follows when the kernel declines)
    if i["n_comp"] <= 0:
        comp = "none"
    elif head == "lat":
        comp = "lat"
    elif (not rerun and pooled and split != 0 and i["comp16"] and i["n_feat"] % 32 == 0 and i["n_comp"] % 32 == 0 and
          o["HEAD_F16"]):
        comp = "f16"
    elif rerun:
        comp = "chained"
    else:
        comp = "f32"

    # who guards
    guard = "none"
    if forward and split != 0 and o["RANGE_GUARD"]:
        guard = "lat" if head == "lat" and whole_call and (i["H"], i["W"]) == (11, 11) else "rerun"

    # bf16 rows
    rows = forward and i["comp_bf16"] and i["n_comp"] > 0 and i["n_comp"] % 4 == 0
    bf16 = "none" if not rows else "epilogue" if epilogue else "cast"
    return dict(split=split, Mform=Mform, lay=lay, stem=stem, chain=chain, first_loop_block=first, pooled=pooled,
                scaled_chain=bool(one_launch_chain and i["scaled"]), head=head, head_gl=head_gl, comp_epilogue=epilogue, comp=comp,
                guard=guard, bf16=bf16, bf16_after_guard=bool(rows and guard != "none"))


BLOCK_TAGS = ("layer1.conv1", "layer1.conv2+ds", "layer2.conv1", "layer2.conv2+ds", "layer3.conv1", "layer3.conv2+ds")
ENCODER_TAGS = ("conv_first",) + BLOCK_TAGS + ("head(avgpool+fc+linear)", "compressMLP", "range_guard",
                                              "layer1.conv2+layer2 (fused)", "layer3 (fused, pooled)",
                                              "layer1.conv2+layer2+layer3 (fused, pooled)")
ENCODER_FORMS = ("chain_lat", "head_lat", "head_longk", "head_splitk", "head_compress", "chain_persist", "chain_tile16", "stem_lat",
                 "guard_lat", "guard_one")


def launches(call, enc_chunk=65536):
    """One magat_encoder_forward_f32 call (`call`: an input without mm / pass) -> (tags, forms, maybe): launch counts per
    profiling tag and form counter.  The launches of the guard's re-run are untagged inside ONE range_guard span.  `maybe` counts
    the chunks whose head may or may not take compressMLP along (the kernel declines when CONV_BNFILL narrowed its tile): each
    moves one count from "compressMLP" to the form "head_compress"."""
    tags = dict.fromkeys(ENCODER_TAGS, 0)
    forms = dict.fromkeys(ENCODER_FORMS, 0)
    maybe = 0
    nblocks = 3 if call["variant"] == 0 else 2
    mc = chunk_agents(call["M"], enc_chunk)
    guard = "none"
    for m0 in range(0, call["M"], mc):
        r = route(dict(call, mm=min(mc, call["M"] - m0), **{"pass": "forward"}))
        guard = r["guard"]
        tags["conv_first"] += r["stem"] != "lat"
        if r["chain"] in ("lat", "one"):
            tags["layer1.conv2+layer2+layer3 (fused, pooled)"] += 1
        elif r["chain"] == "two":
            tags["layer1.conv2+layer2 (fused)"] += 1
            tags["layer3 (fused, pooled)"] += r["first_loop_block"] == 3
        for l in range(r["first_loop_block"], nblocks):
            tags[BLOCK_TAGS[2 * l]] += not (l == 0 and r["stem"] != "plain")
            tags[BLOCK_TAGS[2 * l + 1]] += 1
        tags["head(avgpool+fc+linear)"] += r["head"] != "lat"
        tags["compressMLP"] += r["comp"] in ("f32", "f16")
        maybe += r["comp_epilogue"]
        forms["chain_lat"] += r["chain"] == "lat"
        forms["head_lat"] += r["head"] == "lat"
        forms["stem_lat"] += r["stem"] == "lat"
        forms["guard_lat"] += r["guard"] == "lat"
        forms["head_longk"] += r["head"] == "longk"
        forms["head_splitk"] += r["head"] == "splitk"
    tags["range_guard"] = int(guard == "rerun")
    return {k: int(v) for k, v in tags.items()}, {k: int(v) for k, v in forms.items()}, int(maybe)
