"""CPU-only checks of the source tree itself: the build lists name every file of csrc/, and the shared device helpers
(csrc/f16x3.h) stay the one copy."""
import glob
import os
import re
import time

from conftest import ROOT

CSRC = os.path.join(ROOT, "magat_pathplanning_amd", "csrc")


def _names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, pattern)))


def test_build_lists_name_every_source_and_header():
    from magat_pathplanning_amd import build_native
    assert sorted(build_native.SOURCES) == _names("*.hip")
    assert len(set(build_native.SOURCES)) == len(build_native.SOURCES)
    listed = {os.path.normpath(os.path.join(CSRC, h)) for h in build_native.HEADERS}
    # HEADERS is the staleness list: a header missing from it means edited helpers do not rebuild their users
    for h in _names("*.h"):
        assert os.path.join(CSRC, h) in listed, h
    assert os.path.join(ROOT, "include", "magat_hip.h") in listed
    assert all(os.path.exists(p) for p in listed), listed
    assert set(build_native.SOURCE_FLAGS) <= set(build_native.SOURCES)


def test_a_newer_header_makes_every_object_stale(tmp_path):
    """build() compiles a source when _newer(object, [source] + HEADERS + build_native.py) says so: an object older than one
    header of the list is stale, whichever header it is."""
    from magat_pathplanning_amd import build_native
    obj = tmp_path / "x.o"
    obj.write_bytes(b"")
    past = time.time() - 3600
    deps = []
    for i, h in enumerate(build_native.HEADERS):
        d = tmp_path / ("h%d" % i)
        d.write_text(h)
        os.utime(d, (past, past))
        deps.append(str(d))
    os.utime(obj, (past + 60, past + 60))
    assert not build_native._newer(str(obj), deps)
    for d in deps:
        os.utime(d, (past + 120, past + 120))
        assert build_native._newer(str(obj), deps), d
        os.utime(d, (past, past))


def test_plane_split_and_mfma16_have_one_home():
    """The f16x3 split is the arithmetic the bit-identity of the latency forms rests on: its instruction sequence and mfma16
    are written once, in f16x3.h; a kernel file includes them."""
    for name in _names("*.hip") + _names("*.h"):
        text = open(os.path.join(CSRC, name)).read()
        if name == "f16x3.h":
            assert text.count("asm(\"v_fma_mix_f32") == 2 and len(re.findall(r"\bmfma16\s*\([^;{]*\)\s*\{", text)) == 1
            continue
        assert "v_fma_mix_f32" not in text, name
        assert not re.search(r"\bmfma16\s*\([^;{]*\)\s*\{", text), name      # a definition; calls end in ';'
        for t in ("f16x8", "f16x2", "u32x4"):
            assert not re.search(r"typedef[^;]*\b%s\s+__attribute__" % t, text), (name, t)
