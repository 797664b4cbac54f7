"""The one build procedure behind both back ends (fourierflow_amd/build.py: build_library), with the compiler calls recorded
instead of run: the gfx950 library and the CPU emulator compile the same list, every csrc/*.hip, and nothing when fresh."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fourierflow_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))


def _recorded_builds(monkeypatch, tmp_path):
    """build.build() and build_emu.build() with the compiler calls recorded instead of run, libraries under tmp_path."""
    import build_emu
    from fourierflow_amd import build
    calls = []

    def record(cmd):
        calls.append(cmd)
        open(cmd[cmd.index("-o") + 1], "w").close()

    monkeypatch.setattr(build, "check_call", record)
    monkeypatch.setattr(build, "_hipcc", lambda: "hipcc")
    monkeypatch.setattr(build_emu, "_cxx", lambda: "c++")
    monkeypatch.setattr(build, "LIB", str(tmp_path / "hip" / "libffno_hip.so"))
    monkeypatch.setattr(build_emu, "LIB", str(tmp_path / "emu" / "libffno_emu.so"))

    def compiled(fn):
        del calls[:]
        fn(verbose=False)
        return sorted(c[c.index("-c") + 1] for c in calls if "-c" in c)      # (they run side by side, in any order)
    return build, build_emu, compiled


def test_both_back_ends_compile_every_translation_unit(monkeypatch, tmp_path):
    build, build_emu, compiled = _recorded_builds(monkeypatch, tmp_path)
    want = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert build.source_files() == want and len(want) >= 12
    assert compiled(build.build) == want
    assert compiled(build_emu.build) == want
    assert compiled(build.build) == [] and compiled(build_emu.build) == []       # fresh: nothing to do
    assert build.staleness() == "fresh"


def test_no_sources_is_an_error(monkeypatch, tmp_path):
    build, _, compiled = _recorded_builds(monkeypatch, tmp_path)
    monkeypatch.setattr(build, "CSRC", str(tmp_path))
    with pytest.raises(FileNotFoundError):
        compiled(build.build)
