"""Build the gfx950 C-ABI library (hipcc) in-tree: fourierflow_amd/lib/libffno_hip.so.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build container; the resulting
.so is git-ignored but travels to the GPU box with the working tree.

build_library() is the procedure itself -- stamps, lock, side-by-side compilation, link and rename -- and knows nothing about
hipcc: the CPU wave-emulator flavour of the same sources (tests/emu/build_emu.py) goes through it with its own compiler and flags.
"""
from __future__ import annotations

import fcntl
import glob
import hashlib
import os
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor
from subprocess import check_call

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libffno_hip.so")
ARCH = "gfx950"
FLAGS = (f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-Wno-unused-result")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm >= 7.0 to build the gfx950 F-FNO kernels)")


def source_files():
    """Every translation unit of the library: csrc/*.hip, sorted.  (Experiments and micro-benchmarks keep their .hip files
    under tools/.)"""
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    if not srcs:
        raise FileNotFoundError(f"no *.hip sources in {CSRC}")
    return srcs


def common_inputs():
    """What every object depends on besides its own source: the headers of csrc/ and the ABI header."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(INCLUDE, "ffno.h")]


def _stamp(paths, seed) -> str:
    """The one hash of this build: `seed` (the flags, or the stamp of the common inputs) and the contents of `paths`."""
    h = hashlib.sha256(repr(seed).encode())
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _has_stamp(path, want) -> bool:
    try:
        with open(path + ".stamp") as f:
            return os.path.exists(path) and f.read() == want
    except OSError:
        return False


def build_library(lib, compiler, flags, link_flags=(), include_first=(), extra_inputs=(), force=False, verbose=False) -> str:
    """source_files() -> `lib` with `compiler()` (looked up only when something has to be compiled); `include_first` directories
    come before csrc/ and include/ on the include path and, being places, are no part of the stamps.  Compile + link under an
    exclusive file lock (the ranks of a data-parallel job, or the workers of a parallel test run, may all find the library stale
    at once: one builds, the others wait and find it fresh), into temporary names that are renamed into place: a concurrent
    reader never sees a half-written .so.  Objects are rebuilt only when their own source, a common input or the flags changed
    (per-object stamps), and the translation units compile side by side: a kernel edit costs one file's compile time."""
    sources, outdir = source_files(), os.path.dirname(lib)
    common = _stamp(common_inputs() + list(extra_inputs), tuple(flags))      # (headers are read once, not once per object)
    stamp = _stamp(sources, common)
    if not force and _has_stamp(lib, stamp):       # fresh: no lock, the workers of a parallel test run never queue for it
        return lib
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            # (checked again AFTER the lock was taken: another process may have finished the same build while we waited)
            if not force and _has_stamp(lib, stamp):
                return lib

            def run(cmd):
                if verbose:
                    print("[ffno build]", " ".join(cmd), flush=True)
                check_call(cmd)

            includes = [x for d in (*include_first, CSRC, INCLUDE) for x in ("-I", d)]

            def compile_one(src):
                obj = os.path.join(outdir, os.path.basename(src) + ".o")
                want = _stamp([src], common)
                if force or not _has_stamp(obj, want):
                    if os.path.exists(obj + ".stamp"):
                        os.remove(obj + ".stamp")
                    run([compiler(), *flags, *includes, "-c", src, "-o", obj])
                    with open(obj + ".stamp", "w") as f:
                        f.write(want)
                return obj

            with ThreadPoolExecutor(max_workers=min(len(sources), 16, os.cpu_count() or 4)) as ex:
                objs = list(ex.map(compile_one, sources))
            tag = f".tmp{os.getpid()}"
            run([compiler(), *link_flags, "-shared", "-fPIC", "-o", lib + tag, *objs])
            if os.path.exists(lib + ".stamp"):
                os.remove(lib + ".stamp")          # never a new library beside an old stamp (or the reverse)
            os.replace(lib + tag, lib)
            with open(lib + ".stamp" + tag, "w") as f:
                f.write(stamp)
            os.replace(lib + ".stamp" + tag, lib + ".stamp")
            return lib
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def staleness() -> str:
    """"fresh": the library on disk was built from exactly this tree's sources with the default flags; "stale": from other
    sources or flags (stamp mismatch / no stamp / no library); "unverifiable": the sources or the ABI header are not readable
    here (an installed deployment that ships the prebuilt .so without csrc/ or include/) -- nothing to compare the stamp with."""
    if not os.path.exists(LIB):
        return "stale"
    try:
        want = _stamp(source_files(), _stamp(common_inputs(), FLAGS))
    except OSError:
        return "unverifiable"
    return "fresh" if _has_stamp(LIB, want) else "stale"


def is_stale() -> bool:
    """True when the library on disk is known to come from other sources than the ones in this tree."""
    return staleness() == "stale"


def build(force: bool = False, verbose: bool = True, extra_flags=()) -> str:
    """The gfx950 library; a build with `extra_flags` is stale to staleness(), which knows only the default ones."""
    return build_library(LIB, _hipcc, FLAGS + tuple(extra_flags), link_flags=(f"--offload-arch={ARCH}",), force=force, verbose=verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
