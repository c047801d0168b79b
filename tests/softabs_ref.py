"""SMMALA with the softabs transform of the metric on the CPU oracle — TEST INFRASTRUCTURE (never imported by the product).

The oracle compiles klara.jl_amd/csrc/klara_softabs.h, the header the device compiles, and puts every metric through it where
klara_desc.smmala_softabs > 0.  `SoftabsRefJob` / `AdSoftabsRefJob` are smmala_ref.SmmalaRefJob / autodiff_ref.AdSmmalaRefJob with that field
set.  `f`, `softabs`, `limits` and `sweep_stats` expose the header's pieces to tests/test_softabs_host.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import autodiff_ref
import oracle_ffi as O
import smmala_ref

_sweeps = np.zeros(3, np.int64)          # what the jobs' ko_init / ko_run calls add up: metrics transformed, their sweeps, the most sweeps


def f(lam: float, a: float) -> float:
    """ksa_f: lambda / tanh(a lambda)"""
    return float(O.load().ko_softabs_f(float(lam), float(a)))


def pad_of(d: int) -> int:
    """elements per lane the SMMALA kernels hold a D-vector in (klara_plan.h custom_layout: pow2ceil(max(D, 2)))"""
    return 2 if d <= 2 else 4 if d <= 4 else 8


def softabs(H, a: float, E: int = 0):
    """ksa_softabs_tri on a symmetric D x D matrix (its upper triangle), padded to E elements as the kernels hold it: (T, sweeps)"""
    H = np.ascontiguousarray(H, dtype=np.float64)
    d = H.shape[0]
    T = np.zeros((d, d))
    sw = O.load().ko_softabs(H.ctypes.data, d, int(E) or pad_of(d), float(a), T.ctypes.data)
    assert sw >= -1
    return T, int(sw)


def limits():
    """(sweep cap, squared threshold, series / exponential crossover, largest entry transformed)"""
    out = np.zeros(4)
    O.load().ko_softabs_limits(out.ctypes.data)
    return int(out[0]), float(out[1]), float(out[2]), float(out[3])


def sweep_stats():
    """(metrics transformed, sum of their sweeps, most sweeps) since the last call"""
    out = tuple(int(v) for v in _sweeps)
    _sweeps[...] = 0
    return out


class _Softabs:
    def __init__(self, *, smmala_softabs, **kw):
        super().__init__(**kw)
        self.desc.smmala_softabs = float(smmala_softabs)

    def _sampler_state(self):
        return C.byref(O.KoSamplerState(softabs_sweeps=_sweeps.ctypes.data))


class SoftabsRefJob(_Softabs, smmala_ref.SmmalaRefJob):
    """SmmalaRefJob (a source with klara_user_tensorlogtarget) whose every metric goes through softabs(., a)"""


class AdSoftabsRefJob(_Softabs, autodiff_ref.AdSmmalaRefJob):
    """... on a source with KLARA_USER_AUTODIFF 2: the metric is softabs of the host build's minus-Hessian"""
