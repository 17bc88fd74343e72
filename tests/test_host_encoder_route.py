"""The encoder's dispatch on the CPU: csrc/encoder_route.h (compiled for the host by tools/host_wave/encoder_route_check.cpp) against
the independent restatement of tests/encoder_route_restatement.py over a grid of packs, shapes, passes and options, and the
constants of csrc/encoder_pack.h against encoder.py's.  No GPU needed."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
import encoder_route_restatement as rr

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
# every other value the option's comment in options.hip names (CONV_SPLIT is a bit mask: none, and a partial one)
OPTION_VALUES = dict(CONV_SPLIT=(0, 3), RANGE_GUARD=(0,), CONV_PCHAIN=(0,), L1_FUSED=(1, 0), BLOCK_FUSED=(1, 0), HEAD_SPLITK=(0,),
                     HEAD_F16=(0,), HEAD_COMPRESS=(0,), LAT_AGENTS=(0,))
OPT_ORDER = ("CONV_SPLIT", "RANGE_GUARD", "CONV_PCHAIN", "L1_FUSED", "BLOCK_FUSED", "HEAD_SPLITK", "HEAD_F16", "HEAD_COMPRESS",
             "LAT_AGENTS")
ROUTE_ORDER = ("split", "Mform", "lay", "stem", "chain", "first_loop_block", "pooled", "scaled_chain", "head", "head_gl",
               "comp_epilogue", "comp", "guard", "bf16", "bf16_after_guard")
ENUMS = dict(stem=rr.STEMS, chain=rr.CHAINS, head=rr.HEADS, comp=rr.COMPS, guard=rr.GUARDS, bf16=rr.BF16S)


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("host_wave") / "encoder_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-w", "-x", "c++",
                    os.path.join(ROOT, "tools", "host_wave", "encoder_route_check.cpp"), "-o", exe], check=True)
    return exe


def _packs(variant, H, W, n_feat, n_comp):
    """What fold_resnet puts into a pack of this model and map size (with and without the activation-scale block, which needs the
    one-launch chain's weights), and a pack with nothing optional."""
    large = variant == 0
    maps6 = (H - 1) // 2 + 1 == 6 and (W - 1) // 2 + 1 == 6
    chain3 = maps6 and large
    frag = chain3 and n_comp in (32, 64, 128) and n_feat == 128
    folded = dict(f16=(True, True, large), permuted=True, chain=maps6, chain3=chain3, head16=True, comp16=n_comp > 0,
                  scaled=False, l1frag=(H, W) == (11, 11), headfrag=frag, compfrag=frag)
    out = [folded]
    if chain3:
        out.append(dict(folded, scaled=True))
    out.append(dict(f16=(False, False, False), permuted=False, chain=False, chain3=False, head16=False, comp16=False, scaled=False,
                    l1frag=False, headfrag=False, compfrag=False))
    return out


def _option_sets():
    """each option at every other value, the others at their defaults; then the three build facts, one at a time"""
    sets = [(dict(rr.DEFAULT_OPT), {})]
    for name in OPT_ORDER:
        for v in OPTION_VALUES[name]:
            sets.append((dict(rr.DEFAULT_OPT, **{name: v}), {}))
    for fact in ("conv_direct", "l1_lds", "full_out_gl"):
        sets.append((dict(rr.DEFAULT_OPT), {fact: False}))
    # (two pairs the single flips cannot reach: float32 granules under the band stem's option, the two-launch chain without the
    #  eight-agent stem)
    sets.append((dict(rr.DEFAULT_OPT, CONV_PCHAIN=0, L1_FUSED=1), {}))
    sets.append((dict(rr.DEFAULT_OPT, BLOCK_FUSED=1, L1_FUSED=1), {}))
    return sets


def grid():
    """The issue's grid, pruned to what can occur:
      - comp is passed exactly when n_comp > 0 (the entries refuse n_comp > 0 without it, and nobody passes it otherwise), and
        desc.comp_bf16 only together with it;
      - the pack's optional parts come as fold_resnet makes them for the model and map size, or not at all;
      - a chunk is the whole call or its first 128 agents (ENC_CHUNK's floor), the latter only when M > 128;
      - form_agents = 6400 stands for a shard of a larger batch: only with M < 6400;
      - the re-run and the calibration pass ignore CONV_SPLIT / RANGE_GUARD by construction but are walked under every option
        set all the same;
      - options vary one at a time (plus two pairs), not as a product: every admission condition reads each option once."""
    points = []
    sets = _option_sets()
    for variant, (H, W), n_feat, n_comp in itertools.product((0, 1), ((11, 11), (9, 9), (13, 13)), (128, 1152), (0, 16, 32, 128)):
        for pack, bf16, M, form in itertools.product(_packs(variant, H, W, n_feat, n_comp), (False, True),
                                                     (1, 10, 150, 300, 600, 6400), (0, 6400)):
            if (bf16 and n_comp == 0) or (form and M >= form):
                continue
            for mm in sorted({M, min(M, 128)}):
                base = dict(pack, variant=variant, H=H, W=W, n_feat=n_feat, n_comp=n_comp, form_agents=form, comp=n_comp > 0,
                            comp_bf16=bf16, M=M, mm=mm, buf_floats=rr.buf_floats_per_agent(variant, H, W))
                for opt, facts in sets:
                    for p in rr.PASSES:
                        point = dict(base, opt=opt, conv_direct=True, l1_lds=True, full_out_gl=True)
                        point.update(facts)
                        point["pass"] = p
                        points.append(point)
    return points


def _line(i):
    v = [i["variant"], i["H"], i["W"], i["n_feat"], i["n_comp"], i["form_agents"], *i["f16"], i["permuted"], i["chain"], i["chain3"],
         i["head16"], i["comp16"], i["scaled"], i["l1frag"], i["headfrag"], i["compfrag"], i["comp"], i["comp_bf16"], i["M"], i["mm"],
         rr.PASSES.index(i["pass"]), *(i["opt"][k] for k in OPT_ORDER), i["conv_direct"], i["l1_lds"], i["full_out_gl"], i["buf_floats"]]
    assert len(v) == 36
    return " ".join(str(int(x)) for x in v)


def _want(r):
    return tuple(ENUMS[k].index(r[k]) if k in ENUMS else int(r[k]) for k in ROUTE_ORDER)


@pytest.fixture(scope="module")
def checker_output(route_check):
    points = grid()
    run = subprocess.run([route_check], input="\n".join(_line(p) for p in points) + "\n", check=True, capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    cut = lines.index("routes")
    consts = {l.split()[1]: int(l.split()[2]) for l in lines[:cut]}
    return points, consts, [tuple(int(x) for x in l.split()) for l in lines[cut + 1:]]


def test_route_header_equals_the_restatement_over_the_grid(checker_output):
    points, _, got = checker_output
    assert len(got) == len(points) > 50000
    seen = {k: set() for k in list(ENUMS) + ["lay", "pass", "first_loop_block"]}
    bad = []
    for p, g in zip(points, got):
        want = _want(rr.route(p))
        if want != g and len(bad) < 5:
            bad.append((p, dict(zip(ROUTE_ORDER, want)), dict(zip(ROUTE_ORDER, g))))
        for k in seen:
            seen[k].add(p["pass"] if k == "pass" else g[ROUTE_ORDER.index(k)])
    assert not bad, bad
    # the grid hides no branch: every value of every enum of the route struct is reached
    for k, names in ENUMS.items():
        assert seen[k] == set(range(len(names))), (k, seen[k])
    assert seen["lay"] == {0, 1, 2} and seen["pass"] == set(rr.PASSES) and seen["first_loop_block"] == {0, 2, 3}


def test_every_flag_of_the_route_takes_both_values(checker_output):
    _, _, got = checker_output
    for k in ("pooled", "scaled_chain", "head_gl", "comp_epilogue", "bf16_after_guard"):
        assert {g[ROUTE_ORDER.index(k)] for g in got} == {0, 1}, k


def test_pack_constants_equal_encoder_py(checker_output):
    from magat_pathplanning_amd import encoder as enc
    _, c, _ = checker_output
    want = dict(STEM_W=enc.SLOT_STEM_W, STEM_B=enc.SLOT_STEM_B, HEAD_W=enc.SLOT_HEAD_W, HEAD_B=enc.SLOT_HEAD_B, COMP_W=enc.SLOT_COMP_W,
                COMP_B=enc.SLOT_COMP_B, F32_SLOTS=enc.F32_SLOTS, PERMUTED=enc.SLOT_PERMUTED, TILE16=enc.SLOT_TILE16, SLOTS=enc.SLOTS,
                SC_W0=enc.SC_W0, SC_B0=enc.SC_B0, SC_B1=enc.SC_B1, SC_BA=enc.SC_BA, SC_BB=enc.SC_BB, SC_BC=enc.SC_BC,
                SC_B31=enc.SC_B31, SC_B32=enc.SC_B32, SC_SCALES=enc.SC_SCALES, SC_HEAD_IN=enc.SC_HEAD_IN,
                SC_FEAT_IN=enc.SC_FEAT_IN, SC_FLOATS=enc.SCALED_BLOCK_FLOATS)
    for l in range(3):
        for nm in ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv1_f16", "conv2_f16"):
            want["%s(%d)" % (nm, l)] = getattr(enc, "slot_" + nm)(l)
    for i in range(4):
        want["plain_w(%d)" % i], want["plain_b(%d)" % i] = enc.slot_plain_w(i), enc.slot_plain_b(i)
    want["permuted_behind(32,288)"] = (32 * 288 + 1 + 3) // 4 * 4      # two f16 planes + one scale float, padded to 4 floats
    assert c == want
    assert enc.SCALED_BLOCK_FLOATS == 1352 and enc.SC_FLOATS == 1352
    # the slots are distinct and inside the table, the scale block's segments ascend and fit
    slots = [v for k, v in want.items() if not k.startswith(("SC_", "plain", "F32", "SLOTS", "permuted"))]
    assert len(set(slots)) == len(slots) and max(slots) < enc.SLOTS
    sc = [enc.SC_W0, enc.SC_B0, enc.SC_B1, enc.SC_BA, enc.SC_BB, enc.SC_BC, enc.SC_B31, enc.SC_B32, enc.SC_SCALES, enc.SC_HEAD_IN,
          enc.SC_FEAT_IN, enc.SC_FLOATS]
    assert sc == sorted(sc) and [b - a for a, b in zip(sc, sc[1:])] == [864, 32, 32, 32, 64, 64, 128, 128, 5, 1, 2]


def test_no_bare_slot_number_or_scale_offset_in_the_sources():
    for name in ("encoder_f32.hip", "block_lat.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.findall(r"\boff\[\d", text), name      # (\b: the stem kernel's tap table koff[16] is no pack slot)
        assert not re.findall(r"\bsp \+ \d", text), name
    # and nothing but encoder_f32.hip reads the route
    for name in os.listdir(CSRC):
        if name not in ("encoder_f32.hip", "encoder_route.h") and "encoder_route.h" in open(os.path.join(CSRC, name)).read():
            raise AssertionError(name + " includes encoder_route.h")
