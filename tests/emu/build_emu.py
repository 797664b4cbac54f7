"""Build the CPU wave-emulator flavour of the kernels (TEST INFRASTRUCTURE).

Compiles the *same* sources as the gfx950 library (fourierflow_amd.build.source_files(), by the same build procedure) with a
host compiler against tests/emu/hip_emu.h and writes tests/emu/_build/libffno_emu.so.  Only tests load it; the package never does.
"""
import glob
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "_build", "libffno_emu.so")
FLAGS = ("-x", "c++", "-std=c++17", "-O2", "-mf16c", "-fPIC", "-Wno-unknown-pragmas", "-Wno-unknown-attributes", "-Wno-psabi")

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from fourierflow_amd import build as ffno_build  # noqa: E402


def _cxx():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("clang++ (ext_vector_type support) not found for the emulator build")


def build(verbose=False):
    # this directory comes first on the include path (its ffno_platform.h replaces the one of csrc/); its headers and this file
    # are inputs of every object
    return ffno_build.build_library(LIB, _cxx, FLAGS, include_first=(HERE,), verbose=verbose,
                                    extra_inputs=sorted(glob.glob(os.path.join(HERE, "*.h"))) + [os.path.abspath(__file__)])


if __name__ == "__main__":
    print(build(verbose=True))
