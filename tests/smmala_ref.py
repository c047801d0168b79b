"""The SMMALA sampler on the CPU oracle (oracle/klara_oracle.c ko_smmala) — TEST INFRASTRUCTURE (never imported by the product).

`SmmalaRefJob` is an `oracle_ffi.OracleJob` of sampler id KLARA_SAMPLER_SMMALA, with the oracle's pieces of the sampler that the host tests
probe (`metric`, `inv_chol_t`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L


def inv_chol_t(G):
    """C = L^-T for G = L L' (the kernels' factor, SMMALA deviation 1) and whether G factored"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    d = G.shape[0]
    out = np.zeros((d, d))
    ok = O.load().ko_smmala_inv_chol_t(G.ctypes.data, d, out.ctypes.data)
    return out, bool(ok)


class SmmalaRefJob(O.OracleJob):
    """The SMMALA sampler on the CPU, with OracleJob's constructor, state arrays and accessors."""

    def __init__(self, *, sampler=L.SAMPLER_SMMALA, **kw):
        assert sampler == L.SAMPLER_SMMALA
        assert kw.get("target_kind") in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's SMMALA jobs: logistic or user-defined target"
        super().__init__(sampler=sampler, **kw)

    def metric(self, x):
        """the metric the kernels form at x (logistic: X' diag(r (1 - r)) X, without I / lambda; user-defined: the tensor), D x D"""
        self._bind_user()
        E, D = self.layout.E, self.D
        tri = np.zeros(E * (E + 1) // 2)
        xe = np.ascontiguousarray(x, dtype=np.float64).ravel()
        self.lib.ko_smmala_metric(C.byref(self.desc), C.byref(self.layout), xe.ctypes.data, tri.ctypes.data)
        G = np.zeros((E, E))
        k = 0
        for a in range(E):
            for b in range(a, E):
                G[a, b] = G[b, a] = tri[k]
                k += 1
        return G[:D, :D]
