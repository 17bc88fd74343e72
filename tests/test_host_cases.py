"""CPU-only: the host side of the case generator (csrc/sim_cases.hip, magat_pathplanning_amd/cases.py) - header / loader /
build lists / argument checks - and the restatement that the GPU tests compare the kernel with (tests/cases_restatement.py):
properties it was not written from, on every input of the GPU tests, hand maps with known answers, batch independence."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import cases_restatement as cr
from conftest import ROOT

# name -> (kind, C, H, W, N, density, complexity, seed): the inputs of tests/test_gpu_cases.py.  The 5 x 64, 64 x 5 and
# 64 x 64 rows reach bit 63 and lane 63, 9 x 33 has odd sides, c300 has more cases than compute units.  At density 0.25 no
# 6 x 6 case of any seed 0 .. 149 is invalid (its largest component never falls below 4 cells), so c300_dense is added: the
# same shape at density 0.6, where a tenth of the cases is.
TABLE = {
    "maze10": ("maze", 40, 10, 10, 8, 0.1, 0.01, 7),
    "maze20": ("maze", 8, 20, 20, 10, 0.3, 0.05, 11),
    "uni10": ("uniform", 40, 10, 10, 8, 0.2, 0.0, 7),
    "wide5x64": ("uniform", 3, 5, 64, 4, 0.1, 0.0, 31),
    "tall64x5": ("uniform", 3, 64, 5, 4, 0.1, 0.0, 32),
    "w33": ("uniform", 4, 9, 33, 5, 0.15, 0.0, 33),
    "full64": ("uniform", 2, 64, 64, 100, 0.3, 0.0, 35),
    "c300": ("uniform", 300, 6, 6, 3, 0.25, 0.0, 34),
    "c300_dense": ("uniform", 300, 6, 6, 3, 0.6, 0.0, 5),
}
ALL_VALID = ("maze10", "maze20", "uni10", "wide5x64", "tall64x5", "w33", "full64", "c300")      # asserted on the device too
HAND = cr.hand_maps()
HAND_SEED = 3


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's answer for a row of TABLE, made once."""
    kind, C, H, W, N, density, complexity, seed = TABLE[name]
    return cr.generate(kind, C, H, W, N, density, complexity, seed=seed)


@functools.lru_cache(maxsize=None)
def expected_hand(name, batched=False):
    k = HAND[name]
    if batched:      # three cases on three maps: this one between two others
        maps = np.stack([HAND["serpentine"]["map"], k["map"], HAND["corner_obstacle"]["map"]])
        return cr.generate("given", 3, 6, 8, k["N"], seed=HAND_SEED, maps=maps)
    return cr.generate("given", 2, 6, 8, k["N"], seed=HAND_SEED, maps=k["map"])


def test_cases_entry_is_declared_bound_and_built():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import build_native, cases
    import magat_pathplanning_amd as pkg
    hdr = open(os.path.join(ROOT, "include", "magat_hip.h")).read()
    common = open(os.path.join(ROOT, "magat_pathplanning_amd", "csrc", "magat_common.h")).read()
    assert "sim_cases.hip" in build_native.SOURCES and "row_board.h" in build_native.HEADERS
    assert "magat_sim_cases_generate" in nat.EXPORTED_SYMBOLS
    # added at the END of the header, behind the solver
    assert hdr.index("int magat_sim_mapf_plan(") < hdr.index("int magat_sim_cases_generate(")
    assert hdr.index("int magat_sim_cases_generate(") == max(m.start() for m in re.finditer(r"^(int|size_t|long long) magat_", hdr, re.M))
    assert len(nat._SIGNATURES["magat_sim_cases_generate"][1]) == 18
    for name, value in cases.KINDS.items():
        assert int(re.search(r"#define MAGAT_CASES_%s (\d+)" % name.upper(), hdr).group(1)) == value
    # no tag and no form of its own: it counts under the solver's
    assert int(re.search(r"#define MAGAT_PROF_TAGS_ALL (\d+)", common).group(1)) == 29
    assert int(re.search(r"#define MAGAT_FORMS_ALL (\d+)", common).group(1)) == 19
    assert "sim_cases" not in nat.FORMS and "sim_cases" not in nat.TAGS.values()
    # the board helpers have one home
    csrc = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")
    for src in ("sim_mapf.hip", "sim_cases.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "row_board.h"' in text and "wave_shift(u64 v) {" not in text and "typedef unsigned long long u64" not in text
    assert "wave_shift(u64 v) {" in open(os.path.join(csrc, "row_board.h")).read()
    for name in ("generate_cases", "valid_cases"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    lib = nat.lib()                                   # loads without a GPU
    assert lib.magat_abi_version() == 9 and hasattr(lib, "magat_sim_cases_generate")


def test_argument_checks_answer_before_anything_touches_a_device():
    from magat_pathplanning_amd import _native as nat
    lib = nat.lib()
    one = ctypes.c_void_p(16)
    MAZE, UNIFORM, GIVEN = 0, 1, 2

    def call(kind=MAZE, map_in=None, H=20, W=20, aisles=10, walk=2, first=0, map_out=one, start=one, valid=one, C=2, N=4):
        return lib.magat_sim_cases_generate(kind, map_in, 0, H, W, aisles, walk, 1 << 30, 1, first, map_out, start, one, one, valid,
                                            C, N, None)

    before = lib.magat_form_count(nat.FORMS["sim_mapf"])
    assert call(map_out=None) == -5 and call(start=None) == -5 and call(valid=None) == -5
    assert call(kind=GIVEN, map_in=None) == -5                      # map_in is required for `given` only
    assert call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1 and call(N=0) == -1
    assert call(kind=3) == -1 and call(kind=-1) == -1 and call(aisles=-1) == -1 and call(walk=-1) == -1
    assert call(H=65) == -2 and call(W=65) == -2 and call(kind=UNIFORM, H=65) == -2
    assert call(H=3) == -2 and call(W=2) == -2                      # maze: at least 4 x 4
    assert call(H=4, W=4, N=17) == -2                               # more agents than cells
    assert call(first=-1) == -2 and call(first=(1 << 32) - 1) == -2 and call(aisles=4097) == -2 and call(walk=1025) == -2
    assert call(map_out=None, H=0, W=65) == -5 and call(H=0, W=65) == -1 and call(kind=7, W=65) == -1      # null, sizes, limits
    assert lib.magat_form_count(nat.FORMS["sim_mapf"]) == before     # a refused call is not counted as a launch


def test_cpu_tensors_and_devices_raise():
    from magat_pathplanning_amd import _native as nat
    from magat_pathplanning_amd import cases
    with pytest.raises(nat.MagatNativeError):
        cases.generate_cases(2, 10, 10, 3, device="cpu")
    with pytest.raises(nat.MagatNativeError):
        cases.generate_cases(2, 5, 5, 3, obstacle_map=torch.zeros(5, 5, dtype=torch.uint8))
    assert cases.maze_steps(10, 10, 0.1, 0.01) == (2, 1) and cases.maze_steps(20, 20, 0.3, 0.05) == (30, 10)
    assert cases.maze_steps(20, 20, 0.3, 0.05) == cr.maze_steps(20, 20, 0.3, 0.05)
    assert cases.uniform_threshold(0.25) == 1 << 30 and cases.uniform_threshold(1.0) == 1 << 32
    assert cases.uniform_threshold(-1.0) == 0 and cases.uniform_threshold(2.0) == 1 << 32


# ---- the random numbers ------------------------------------------------------------------------------------------------------
def test_the_hash_is_the_splitmix64_finaliser():
    """splitmix64 seeded with 0 steps its state by M and finalises it: its published first outputs."""
    assert [cr.mix(cr.M * k & cr.MASK) for k in (1, 2, 3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert cr.draw(5, 2, 3, 9) == cr.mix(cr.mix(5 + 3 * cr.M) + cr.M * ((3 << 40 | 9) + 1))
    assert cr.draw(cr.MASK, 0, 0, 0) == cr.mix(cr.mix(cr.M - 1) + cr.M)                      # the sums wrap mod 2^64
    assert all(0 <= cr.below(1, 0, 4, i, 7) < 7 for i in range(200))
    assert sorted({cr.below(1, 0, 4, i, 7) for i in range(200)}) == list(range(7))


# ---- the restatement against properties it was not written from, on every input of the GPU tests -------------------------------
def _one_component(cells):
    """Are the cells one 4-connected set?  (union-find over neighbouring pairs: not the restatement's search)"""
    cells = [tuple(c) for c in cells]
    parent = {c: c for c in cells}

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    for r, c in cells:
        for v in ((r + 1, c), (r, c + 1)):
            if v in parent:
                parent[find((r, c))] = find(v)
    return len({find(c) for c in cells}) <= 1


def _largest_other_component(raw, kept_map):
    """Size of the largest component of the raw free cells that are NOT kept, by repeated dilation of a label image."""
    rest = (raw == 0) & (kept_map != 0)
    label = np.where(rest, np.arange(rest.size).reshape(rest.shape) + 1, 0)
    while True:
        big = np.pad(label, 1)
        grown = np.maximum.reduce([big[1:-1, 1:-1], big[:-2, 1:-1], big[2:, 1:-1], big[1:-1, :-2], big[1:-1, 2:]])
        grown = np.where(rest, grown, 0)
        if (grown == label).all():
            break
        label = grown
    return int(np.bincount(label[rest]).max()) if rest.any() else 0


def check_properties(out, N, what):
    C = len(out["map"])
    for c in range(C):
        raw, m = out["raw"][c], out["map"][c]
        kept = np.argwhere(m == 0)
        assert ((raw != 0) <= (m != 0)).all(), (what, c)                      # obstacles: a superset of the raw ones
        assert _one_component(kept), (what, c)
        assert _largest_other_component(raw, m) <= len(kept), (what, c)       # no other component is larger
        assert out["free_cells"][c] == (m == 0).sum(), (what, c)
        s, g = out["start"][c], out["goal"][c]
        if not out["valid"][c]:
            assert (s == -1).all() and (g == -1).all(), (what, c)
            continue
        assert len(kept) >= N + 1
        assert len({tuple(v) for v in s}) == N and len({tuple(v) for v in g}) == N, (what, c)
        assert (s != g).any(axis=1).all(), (what, c)
        assert (m[s[:, 0], s[:, 1]] == 0).all() and (m[g[:, 0], g[:, 1]] == 0).all(), (what, c)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_properties_on_the_gpu_inputs(name):
    kind, C, H, W, N = TABLE[name][:5]
    out = expected(name)
    assert out["map"].shape == (C, H, W) and out["start"].shape == (C, N, 2) and out["start"].dtype == np.int32
    check_properties(out, N, name)
    if name in ALL_VALID:
        assert out["valid"].all(), name       # what tests/test_gpu_cases.py asserts on the device: the restatement alone gives it
    if name == "c300_dense":
        assert 0 < int(out["valid"].sum()) < C and (out["free_cells"] < N + 1).any()
    if kind == "maze":
        aisles, walk = out["aisles"], out["walk"]
        assert (aisles, walk) == ((2, 1) if name == "maze10" else (30, 10))
        for c in range(C):
            tr = out["trace"][c]
            assert len(tr["origins"]) == aisles and all(y % 2 == 0 and x % 2 == 0 for y, x in tr["origins"])
            assert 0 < out["raw"][c].sum() <= aisles * (1 + 2 * walk)
            assert len(tr["steps"]) == aisles * walk
            assert all(n >= 2 and pick < n - 1 for n, pick, _ in tr["steps"])      # the last listed neighbour is never taken
            assert out["raw"][c].sum() <= aisles + 2 * sum(t for _, _, t in tr["steps"])
        assert any(t for c in range(C) for _, _, t in out["trace"][c]["steps"])
    if kind == "uniform":      # the density is what was asked for (3 sigma of a binomial over all cells; c300: 10800 cells)
        p, cells = TABLE[name][5], C * H * W
        assert abs(out["raw"].mean() - p) <= 3 * (p * (1 - p) / cells) ** 0.5, out["raw"].mean()


def test_starts_are_uniform_over_the_region():
    """Every cell of a 12-cell region is the first start about 1 / 12 of the time, and (start 0, start 1) are never equal."""
    m = cr.grid(["....", "....", "...."])
    out = cr.generate("given", 1200, 3, 4, 2, seed=9, maps=m)
    first = out["start"][:, 0, 0] * 4 + out["start"][:, 0, 1]
    counts = np.bincount(first, minlength=12)
    assert out["valid"].all() and counts.min() >= 100 - 3 * 10 and counts.max() <= 100 + 3 * 10, counts      # sigma = 9.6
    check_properties(out, 2, "open 3 x 4")


# ---- hand maps with known answers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_maps(name, batched):
    k = HAND[name]
    out = expected_hand(name, batched)
    c = 1 if batched else 0
    assert out["free_cells"][c] == k["free_cells"] and out["valid"][c] == k["valid"], name
    assert [tuple(v) for v in np.argwhere(out["map"][c] == 0)] == sorted(k["kept"]), name
    check_properties(out, k["N"], name)
    if batched:      # the neighbours are untouched by the map in the middle
        assert out["free_cells"][0] == HAND["serpentine"]["free_cells"] and out["free_cells"][2] == 9
    else:            # one map, two cases: two different draws from the same region
        assert (out["map"][0] == out["map"][1]).all()
        if k["valid"]:
            assert (out["start"][0] != out["start"][1]).any() or (out["goal"][0] != out["goal"][1]).any()


def test_the_corner_map_would_be_empty_under_the_reference_rule():
    k = HAND["corner_obstacle"]
    assert k["map"][0, 0] == 1                      # a flood from (0, 0) keeps nothing: the reference's img_fill
    assert cr.kept_region(k["map"]) == sorted(k["kept"])
    assert cr.kept_region(np.ones((4, 4), dtype=np.uint8)) == []
    out = cr.generate("given", 1, 4, 4, 2, seed=1, maps=np.ones((4, 4), dtype=np.uint8))
    assert out["free_cells"].tolist() == [0] and out["valid"].tolist() == [0] and (out["map"] == 1).all()


def test_a_case_depends_on_its_global_index_only():
    for name in ("maze10", "uni10"):
        kind, C, H, W, N, density, complexity, seed = TABLE[name]
        whole = expected(name)
        a = cr.generate(kind, 20, H, W, N, density, complexity, seed=seed)
        b = cr.generate(kind, 20, H, W, N, density, complexity, seed=seed, first_case=20)
        for key in ("map", "start", "goal", "free_cells", "valid"):
            np.testing.assert_array_equal(np.concatenate([a[key], b[key]]), whole[key], err_msg=key)
        other = cr.generate(kind, 20, H, W, N, density, complexity, seed=seed + 1)
        assert (other["start"] != a["start"]).any() and (other["map"] != a["map"]).any()
