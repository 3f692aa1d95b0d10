"""Build the in-tree HIP extension (gfx950) and the C-ABI shared library."""
from __future__ import annotations

import os
import subprocess

from ._lib import PKG_DIR, REPO_DIR, LIB_PATH

SOURCES = ["csrc/gm_capi.hip", "csrc/gm_calib.hip", "csrc/gm_eval.hip", "csrc/gm_host_model.cpp", "csrc/gm_mjcf.cpp"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-munsafe-fp-atomics",
         "-ffp-contract=off",
         # MachineLICM off: in the outlined substep loop (gm_substep.h substep_loop) it
         # hoists constant materialisations out of the loop and the body then spills
         "-mllvm", "-disable-machine-licm"]


# the same sources with the decoupled Newton point compiled out (csrc/gm_newton.hip): the
# library tests/test_decoupled_point.py compares the default one with, byte for byte
NO_DECOUPLED_LIB = os.path.join(os.path.dirname(LIB_PATH), "libgm_no_decoupled.so")


def _deps():
    csrc = os.path.join(PKG_DIR, "csrc")
    return sorted(os.path.join(PKG_DIR, s) for s in SOURCES) + \
        sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".inc"))) + \
        [os.path.join(REPO_DIR, "include", f) for f in ("gripper_mi355x.h", "gm_settings.def")]


def _build_variant(lib: str, flag: str, verbose: bool) -> str:
    """build(out=lib, extra_flags=[flag]), unless that library is already newer than every source."""
    if os.path.exists(lib):
        t = os.path.getmtime(lib)
        if all(os.path.getmtime(d) <= t for d in _deps()):
            return lib
    return build(verbose=verbose, out=lib, extra_flags=[flag])


def build_no_decoupled(verbose: bool = False) -> str:
    return _build_variant(NO_DECOUPLED_LIB, "-DGM_NO_DECOUPLED_POINT", verbose)


# ... and with the free object's velocity sums back on one lane
# (csrc/gm_rows.h, gm_dynamics.h): the partner of tests/test_object_lanes.py
NO_OBJECT_LANES_LIB = os.path.join(os.path.dirname(LIB_PATH), "libgm_no_object_lanes.so")


def build_no_object_lanes(verbose: bool = False) -> str:
    return _build_variant(NO_OBJECT_LANES_LIB, "-DGM_NO_OBJECT_LANES", verbose)


def build(verbose: bool = False, force: bool = False, out: str | None = None, extra_flags=()) -> str:
    """Compile each translation unit in parallel (the env-step kernel and the calibration
    variant are separate device modules), then link libgm.so (or `out`: developer A/B
    builds, with `extra_flags` added to every compile)."""
    lib_path = out or LIB_PATH
    srcs = [os.path.join(PKG_DIR, s) for s in SOURCES]
    # the device translation units include each other's kernels and headers: every one of
    # them is a dependency, so code moved between files cannot leave a stale object
    csrc = os.path.join(PKG_DIR, "csrc")
    deps = sorted(set(srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".inc"))])) + \
        [os.path.join(REPO_DIR, "include", f) for f in ("gripper_mi355x.h", "gm_settings.def")]
    if not force and out is None and os.path.exists(LIB_PATH):
        t = os.path.getmtime(LIB_PATH)
        if all(os.path.getmtime(d) <= t for d in deps):
            return LIB_PATH
    objdir = os.path.join(os.path.dirname(LIB_PATH), "obj" if out is None else "obj_" + os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    inc = ["-I" + os.path.join(REPO_DIR, "include"), "-I" + os.path.join(PKG_DIR, "csrc")]
    procs, objs = [], []
    headers = [os.path.join(csrc, "gm_state.h")] + \
        [os.path.join(REPO_DIR, "include", f) for f in ("gripper_mi355x.h", "gm_settings.def")]
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        # host-only translation units (.cpp) depend on their source and the shared headers;
        # the device ones on every kernel source
        tu_deps = [src] + headers if src.endswith(".cpp") else deps
        if not force and os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in tu_deps):
            continue
        cmd = [HIPCC, *FLAGS, *extra_flags, *inc, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((subprocess.Popen(cmd), cmd))
    for p, cmd in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    link = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib_path + ".tmp"]
    if verbose:
        print(" ".join(link))
    subprocess.run(link, check=True)
    os.replace(lib_path + ".tmp", lib_path)
    return lib_path
