"""Loader of tests/softabs_ref.c, the CPU reference of the SMMALA kernels with the softabs transform of the metric — TEST INFRASTRUCTURE
(never imported by the product).

Compiled at test time with the flags tests/smmala_ref.py uses (gcc -O2 -std=gnu11 -ffp-contract=off, detmath.h for kd_*) against
klara.jl_amd/csrc/klara_softabs.h, the header the device compiles.  The library exports smmala_ref.c's entry points, so `SoftabsRefJob` /
`AdSoftabsRefJob` are smmala_ref.SmmalaRefJob / autodiff_ref.AdSmmalaRefJob driving this library, with klara_desc.smmala_softabs set.
`f`, `softabs`, `limits` and `sweep_stats` expose the header's pieces to tests/test_softabs_host.py.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
from pathlib import Path

import numpy as np

import autodiff_ref
import oracle_ffi as O
import smmala_ref
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
SRC = Path(__file__).resolve().parent / "softabs_ref.c"
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    ora = O.load()
    csrc = ROOT / "klara.jl_amd" / "csrc"
    inputs = [SRC, ROOT / "include" / "klara_hip.h", csrc / "detmath.h", csrc / "klara_softabs.h"]
    key = hashlib.sha1(b"".join(p.read_bytes() for p in inputs)).hexdigest()[:16]
    out = ROOT / "build" / "softabs_ref"
    out.mkdir(parents=True, exist_ok=True)
    so = out / f"softabs_ref_{key}.so"
    if not so.exists():
        tmp = out / f".softabs_ref_{key}.{os.getpid()}.so"
        r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(ROOT / "include"),
                            "-I", str(csrc), "-o", str(tmp), str(SRC), "-lm"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("tests/softabs_ref.c did not compile:\n" + r.stderr)
        tmp.replace(so)
    lib = C.CDLL(str(so))
    vp = C.c_void_p
    lib.sr_bind.argtypes = [vp] * 4
    lib.sr_bind.restype = None
    lib.sr_bind_tensor.argtypes = [vp]
    lib.sr_bind_tensor.restype = None
    lib.sr_check_init.argtypes = [C.POINTER(L.KlaraDesc), C.POINTER(O.KoLayout), vp, vp, vp]
    lib.sr_check_init.restype = C.c_int
    lib.sr_run.argtypes = [C.POINTER(L.KlaraDesc), C.POINTER(O.KoLayout)] + [vp] * 7 + [C.c_int64, C.c_int64] + [vp] * 5 + [C.c_int64, vp, vp, vp]
    lib.sr_run.restype = C.c_int
    lib.sr_metric.argtypes = [C.POINTER(L.KlaraDesc), C.POINTER(O.KoLayout), vp, vp]
    lib.sr_metric.restype = None
    lib.sa_f.argtypes = [C.c_double, C.c_double]
    lib.sa_f.restype = C.c_double
    lib.sa_softabs.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp]
    lib.sa_softabs.restype = C.c_int
    lib.sa_limits.argtypes = [vp]
    lib.sa_limits.restype = None
    lib.sa_sweep_stats.argtypes = [vp]
    lib.sa_sweep_stats.restype = None
    addr = lambda f: C.cast(f, C.c_void_p).value
    lib.sr_bind(addr(ora.ko_transition_normals), addr(ora.ko_eval_target), addr(ora.ko_logistic_rate_score), addr(ora.ko_erf_rate_score))
    _lib = lib
    return lib


def f(lam: float, a: float) -> float:
    """ksa_f: lambda / tanh(a lambda)"""
    return float(load().sa_f(float(lam), float(a)))


def pad_of(d: int) -> int:
    """elements per lane the SMMALA kernels hold a D-vector in (klara_plan.h custom_layout: pow2ceil(max(D, 2)))"""
    return 2 if d <= 2 else 4 if d <= 4 else 8


def softabs(H, a: float, E: int = 0):
    """ksa_softabs_tri on a symmetric D x D matrix (its upper triangle), padded to E elements as the kernels hold it: (T, sweeps)"""
    H = np.ascontiguousarray(H, dtype=np.float64)
    d = H.shape[0]
    T = np.zeros((d, d))
    sw = load().sa_softabs(H.ctypes.data, d, int(E) or pad_of(d), float(a), T.ctypes.data)
    assert sw >= -1
    return T, int(sw)


def limits():
    """(sweep cap, squared threshold, series / exponential crossover, largest entry transformed)"""
    out = np.zeros(4)
    load().sa_limits(out.ctypes.data)
    return int(out[0]), float(out[1]), float(out[2]), float(out[3])


def sweep_stats():
    """(metrics transformed, sum of their sweeps, most sweeps) since the last call"""
    out = np.zeros(3, np.int64)
    load().sa_sweep_stats(out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


class _Softabs:
    def _use_softabs(self, a):
        self.sr = load()
        self.desc.smmala_softabs = float(a)


class SoftabsRefJob(_Softabs, smmala_ref.SmmalaRefJob):
    """SmmalaRefJob (a source with klara_user_tensorlogtarget) whose every metric goes through softabs(., a)"""

    def __init__(self, *, smmala_softabs, **kw):
        super().__init__(**kw)
        self._use_softabs(smmala_softabs)


class AdSoftabsRefJob(_Softabs, autodiff_ref.AdSmmalaRefJob):
    """... on a source with KLARA_USER_AUTODIFF 2: the metric is softabs of the host build's minus-Hessian"""

    def __init__(self, *, smmala_softabs, **kw):
        super().__init__(**kw)
        self._use_softabs(smmala_softabs)
