"""Builds and loads tests/prim_probe.hip, the test-only unit that calls the device's numeric and
lane primitives on their own (tests/test_device_primitives.py).

The probe is compiled with gmx.build's compiler, flags and include directories, so the functions
mean in it what they mean in libgm's units: lib/libgm_prim_probe.so, and lib/libgm_prim_probe_cal.so
from the same source with -DGM_CAL_TU (the calibration unit's selections: correctly rounded rsq_n
and rcp_piv, namespace gmf unfused).  Both are rebuilt when older than the probe source or any
file of csrc.  `csrc=` points the include path at another copy of the headers (a mutated copy: the
check that the tests notice a wrong primitive); such a build goes to `out`, never to lib/.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from gmx._lib import PKG_DIR, REPO_DIR, LIB_PATH
from gmx.build import HIPCC, FLAGS

PROBE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prim_probe.hip")
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(REPO_DIR, "include")
LIB_DIR = os.path.dirname(LIB_PATH)

OPS = ("sqrt_n", "rsq_n", "rcp_n", "rcp_refined", "rcp_piv", "gm_sin", "gm_cos")   # prim_probe.hip's OP_ enum

SLOT_SHR, SLOT_SHL, SLOT_BCAST, SLOT_READLANE, SLOT_TOTALS, SLOT_CHAINS = 0, 4, 8, 24, 88, 89


def lib_path(cal: bool = False) -> str:
    return os.path.join(LIB_DIR, "libgm_prim_probe_cal.so" if cal else "libgm_prim_probe.so")


def _deps(csrc: str):
    return [PROBE_SRC] + [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))] + \
        [os.path.join(INCLUDE, f) for f in ("gripper_mi355x.h", "gm_settings.def")]


def build(cal: bool = False, csrc: str | None = None, out: str | None = None, force: bool = False,
          verbose: bool = False) -> str:
    """Compile the probe (with -DGM_CAL_TU when `cal`) against the headers in `csrc` (default: the
    package's) into `out` (default: lib_path(cal)); skipped when `out` is newer than every source."""
    if csrc is not None and out is None:
        raise ValueError("a build against another copy of the headers needs its own `out`")
    csrc = csrc or CSRC
    out = out or lib_path(cal)
    if not force and os.path.exists(out):
        t = os.path.getmtime(out)
        if all(os.path.getmtime(d) <= t for d in _deps(csrc)):
            return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [HIPCC, *FLAGS, *(["-DGM_CAL_TU"] if cal else []), "-I" + INCLUDE, "-I" + csrc,
           "-shared", PROBE_SRC, "-o", out + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    return out


_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_fp = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_up = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")


class Probe:
    """The probe library's entry points on numpy arrays; a hipError_t other than 0 raises."""

    def __init__(self, path: str):
        self.path = path
        # one HIP runtime per process (gmx._lib.load_library): torch first, so that the probe
        # binds to the runtime torch brings instead of loading a second one that sees no device
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = self.lib = C.CDLL(path)
        for name, args in (("prim_unary", [C.c_int, _dp, _dp, C.c_int]),
                           ("prim_binary", [_dp, _dp, _dp, C.c_int]),
                           ("prim_lanes", [_dp, _dp, _dp]),
                           ("prim_helpers", [_dp, _dp, C.c_int]),
                           ("prim_choose", [_fp, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_uint64,
                                            _ip, _fp, _fp]),
                           ("prim_mix", [_up, _up, C.c_int])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, C.c_int
        lib.host_sincos.argtypes, lib.host_sincos.restype = [_dp, _dp, _dp, C.c_int], None
        assert lib.prim_op_count() == len(OPS)
        cl = (C.c_int * 16)()
        self.chain_lengths = tuple(cl[i] for i in range(lib.prim_chain_lengths(cl)))
        self.n_slots = lib.prim_n_slots()
        assert self.n_slots == SLOT_CHAINS + 2 * len(self.chain_lengths)
        self.helpers_in, self.helpers_out = lib.prim_helpers_in(), lib.prim_helpers_out()
        self.is_cal = bool(lib.prim_is_cal())

    @staticmethod
    def _ok(err, what):
        if err != 0:
            raise RuntimeError(f"{what}: hipError_t {err}")

    def unary(self, op: str, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.empty_like(x)
        self._ok(self.lib.prim_unary(OPS.index(op), x, out, x.size), f"prim_unary({op})")
        return out

    def binary(self, a, b) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        b = np.ascontiguousarray(b, dtype=np.float64).ravel()
        assert a.size == b.size
        out = np.empty_like(a)
        self._ok(self.lib.prim_binary(a, b, out, a.size), "prim_binary")
        return out

    def lanes(self, x, L=None) -> np.ndarray:
        """[n_slots, 64] for the wave's input x[64] and multipliers L[64][16] (zeros by default)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        L = np.zeros((64, 16)) if L is None else np.ascontiguousarray(L, dtype=np.float64)
        assert x.shape == (64,) and L.shape == (64, 16)
        out = np.empty((self.n_slots, 64))
        self._ok(self.lib.prim_lanes(x, L, out), "prim_lanes")
        return out

    def helpers(self, cases) -> np.ndarray:
        cases = np.ascontiguousarray(cases, dtype=np.float64)
        assert cases.ndim == 2 and cases.shape[1] == self.helpers_in
        out = np.empty((cases.shape[0], self.helpers_out))
        self._ok(self.lib.prim_helpers(cases, out, cases.shape[0]), "prim_helpers")
        return out

    def choose(self, logits, eps: float, seed: int, decision: int, gid0: int):
        """(actions[n], q[n][n_out], qbest[n]) of gp_choose on every row, row i with gid0 + i."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        n, n_out = logits.shape
        actions, q, qbest = np.empty(n, np.int32), np.empty((n, n_out), np.float32), np.empty(n, np.float32)
        self._ok(self.lib.prim_choose(logits, n, n_out, eps, seed, decision, gid0, actions, q, qbest), "prim_choose")
        return actions, q, qbest

    def mix(self, z) -> np.ndarray:
        z = np.ascontiguousarray(z, dtype=np.uint64).ravel()
        out = np.empty_like(z)
        self._ok(self.lib.prim_mix(z, out, z.size), "prim_mix")
        return out

    def host_sincos(self, x):
        """(sin, cos) from the host build of gm_sincos: runs without a GPU."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        s, c = np.empty_like(x), np.empty_like(x)
        self.lib.host_sincos(x, s, c, x.size)
        return s, c


_loaded: dict = {}


def load(cal: bool = False, csrc: str | None = None, out: str | None = None) -> Probe:
    path = build(cal=cal, csrc=csrc, out=out)
    if path not in _loaded:
        _loaded[path] = Probe(path)
    return _loaded[path]
