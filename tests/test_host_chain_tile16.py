"""Host-side checks of the chain kernel's 16-row form (option CHAIN_TILE16): the weight pack in 16-row fragments against a NumPy
restatement of its layout, and the half-tile tables of csrc/block_walk.h (read from the header) against the geometry of a
6 x 6 map with a 3 x 3 stencil."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile16_pack_is_a_permutation_of_the_32_row_pack():
    """encoder.pack_block3_tile16: lane l of block (channel tile, k32 step, half, plane) holds, for output channel
    32 ct + 16 half + (l & 15), the 8 halves of k chunk 4 k32 + (l >> 4) - the 16-byte piece that lane
    32 ((l >> 4) & 1) + 16 half + (l & 15) holds in 16-channel step 2 k32 + (l >> 5) of the 32-row pack.  Checked element by
    element on random weights; and through the weights themselves: channel and input column of every piece."""
    from magat_pathplanning_amd import encoder as enc
    g = torch.Generator().manual_seed(7)
    w1 = torch.randn(128, 9 * 64, generator=g) * 0.05
    w2 = torch.randn(128, 9 * 128 + 64, generator=g) * 0.05
    blocks = enc.pack_block3_weights(w1, w2)
    t16 = enc.pack_block3_tile16(blocks).view(torch.int16).numpy()
    assert t16.size * 2 == (4 * 72 + 4 * 80) * 1024
    pos = 0
    for blk, s16 in ((blocks[1], 36), (blocks[2], 40)):
        old = blk[:-4].contiguous().view(torch.int16).numpy().reshape(4, s16, 2, 64, 8)
        new = t16[pos:pos + old.size].reshape(4, s16 // 2, 2, 2, 64, 8)
        pos += old.size
        want = np.empty_like(new)
        for l in range(64):
            col, kq = l & 15, l >> 4
            for half in range(2):
                want[:, :, half, :, l, :] = old.reshape(4, s16 // 2, 2, 2, 64, 8)[:, :, kq >> 1, :, 32 * (kq & 1) + 16 * half + col, :]
        assert np.array_equal(new, want)
        assert np.array_equal(np.sort(new.reshape(-1)), np.sort(old.reshape(-1)))
    assert pos == t16.size
    # ... and from the weights: first plane of block a, tap u, k32 step t, half h, lane l, element i is
    # f16(w 2^e) of output channel 32 ct + 16 h + (l & 15), intermediate channel chain_channel(2 t + (l >> 5), (l >> 4) & 1, i)
    e = round(-np.log2(float(blocks[1][-4])))
    taps = w2[:, :9 * 128].reshape(128, 9, 128)
    a = enc.pack_block3_tile16(blocks).view(torch.int16)[:4 * 36 * 1024].view(torch.float16).reshape(4, 9, 2, 2, 2, 64, 8)
    for ct, u, t, h, l, i in ((0, 0, 0, 0, 0, 0), (3, 8, 1, 1, 63, 7), (1, 4, 0, 1, 37, 5), (2, 7, 1, 0, 18, 2)):
        ch = enc.chain_channel(2 * t + (l >> 5), (l >> 4) & 1, i)
        want = (taps[32 * ct + 16 * h + (l & 15), u, ch] * 2.0 ** e).half()
        assert a[ct, u, t, h, 0, l, i] == want


def _tables():
    src = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "block_walk.h")).read()
    pix = re.search(r"constexpr int HT_PIX\[HT_N\]\[2\] = \{(.*?)\};", src, re.S).group(1)
    pix = re.sub(r"//[^\n]*", "", pix)
    pix = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+),\s*(\d+)\}", pix)]
    taps = re.search(r"constexpr int HT_TAPS\[HT_N\] = \{(.*?)\};", src, re.S).group(1)
    taps = [int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]+", taps)]
    return pix, taps


def _valid(pix, tp):
    y, x = pix // 6 + tp // 3 - 1, pix % 6 + tp % 3 - 1
    return 0 <= y < 6 and 0 <= x < 6


def test_half_tile_items_cover_exactly_the_valid_taps():
    """The item list of walk16 (tap-major over the half tiles whose mask has the tap - h16_seq, restated here): every pixel of the
    6 x 6 map sits in exactly one half tile; every valid (pixel, tap) pair is run exactly once; a half tile runs no tap that is
    invalid for both of its pixels, and only the two corner pairs run a tap that is invalid for one (read as the zero pixel per
    lane); 132 half-tile-taps per channel tile and k step (the nine 32-row tiles: 69 tile-taps = 138)."""
    pix, taps = _tables()
    assert len(pix) == 18 and len(taps) == 18
    assert sorted(p for pair in pix for p in pair) == list(range(36))
    items = [(tp, s) for tp in range(9) for s in range(18) if taps[s] >> tp & 1]
    assert len(items) == 132 and len(set(items)) == 132
    run = {(p, tp) for tp, s in items for p in pix[s]}
    valid = {(p, tp) for p in range(36) for tp in range(9) if _valid(p, tp)}
    assert valid <= run
    corners = [s for s in range(18) if set(pix[s]) <= {0, 5, 30, 35}]
    assert len(corners) == 2
    for tp, s in items:
        v = [_valid(p, tp) for p in pix[s]]
        assert any(v)
        if not all(v):
            assert s in corners
    # the zero reads: 2 corner pairs x 6 taps x 2 pixels = 24 lane-taps, 16 of them valid (4 per corner)
    assert len(run - valid) == 8
    # slots of a half tile hold pixels of opposite parity (conflict-free ds_read_b128) except in the four column-edge tiles
    same = [s for s in range(18) if (pix[s][0] ^ pix[s][1]) & 1 == 0]
    assert all({p % 6 for p in pix[s]} in ({0}, {5}) for s in same) and len(same) == 4


def test_half_tile_slots_pool_in_registers():
    """The pooled epilogue's sums (block_fused.hip): per slot the in-lane sums named there are whole 2 x 2 cells, or halves whose
    other half sits in the other slot of the same half tiles."""
    pix, _ = _tables()
    I1, I2, I3, I4, I5, I6, I7, I8, CT, CB, TA, TB, BA, BB, LA, LB, RA, RB = range(18)
    cell = lambda c: {12 * (c // 3) + 2 * (c % 3) + d for d in (0, 1, 6, 7)}
    for sl in (0, 1):
        e = (RA, RB) if sl else (LA, LB)
        xq = (LA, LB) if sl else (RA, RB)
        assert {pix[s][sl] for s in (CT, I1, TA, e[0])} == cell(2 if sl else 0)
        assert {pix[s][sl] for s in (CB, I2, BA, e[1])} == cell(8 if sl else 6)
        assert {pix[s][sl] for s in (I5, I6) + xq} == cell(3 if sl else 5)
    for c, (a, b) in ((1, (TB, I3)), (7, (BB, I4)), (4, (I7, I8))):
        assert {pix[s][sl] for s in (a, b) for sl in (0, 1)} == cell(c)
