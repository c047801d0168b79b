"""The AM sampler on the CPU oracle (oracle/klara_oracle.c ko_am) — TEST INFRASTRUCTURE (never imported by the product).

`AmRefJob` is an `oracle_ffi.OracleJob` of sampler id KLARA_SAMPLER_AM that carries every chain's covariance and running means (`.C`,
`.lastmean`, `.secondlastmean`, `.fallbacks`) and hands them to ko_init / ko_run as the oracle's ko_sampler_state.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent


def sanitizer_program() -> Path:
    """tests/am_sanitizer_main.c compiled together with oracle/klara_oracle.c with -fsanitize=address,undefined: a stand-alone host program"""
    srcs = [ROOT / "tests" / "am_sanitizer_main.c", ROOT / "oracle" / "klara_oracle.c"]
    return O.build_c("am_ref_main", ["-O2", "-std=gnu11", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *O.INC],
                     sources=srcs, hashed=[ROOT / "include" / "klara_hip.h", O.CSRC / "detmath.h", O.CSRC / "detmath_tables.h", O.CSRC / "klara_softabs.h"],
                     shared=False)


def pack(Cm):
    """(n, D, D) symmetric matrices -> (n, D (D + 1) / 2) packed upper triangles (ktri(i, j, D) = C_ij, i <= j)"""
    Cm = np.asarray(Cm, dtype=np.float64)
    D = Cm.shape[1]
    return np.ascontiguousarray(np.stack([Cm[:, i, j] for i in range(D) for j in range(i, D)], axis=1))


def unpack(P, D):
    """the inverse of pack: (n, D, D) full symmetric"""
    out = np.zeros((P.shape[0], D, D))
    k = 0
    for i in range(D):
        for j in range(i, D):
            out[:, i, j] = P[:, k]
            out[:, j, i] = P[:, k]
            k += 1
    return out


class AmRefJob(O.OracleJob):
    """The AM sampler on the CPU, with OracleJob's constructor, state arrays and accessors."""

    def __init__(self, *, am_C0=None, am_corescale=1.0, am_minorscale=1.0, am_c=0.05, am_t0=10, sampler=L.SAMPLER_AM, **kw):
        assert sampler == L.SAMPLER_AM
        assert kw.get("target_kind") in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's AM jobs: logistic or user-defined target"
        assert kw.get("tuner", 0) == L.TUNER_VANILLA and kw.get("tuner_mode", 0) == L.TUNE_PER_CHAIN
        super().__init__(sampler=sampler, **kw)
        d = self.desc
        d.am_corescale, d.am_minorscale, d.am_c, d.am_t0 = float(am_corescale), float(am_minorscale), float(am_c), int(am_t0)
        C0 = np.asarray(am_C0, dtype=np.float64)
        C0 = np.diag(C0.ravel()) if C0.ndim < 2 else C0
        assert C0.shape == (self.D, self.D)
        self.C0 = np.triu(C0) + np.triu(C0, 1).T           # the upper triangle is read
        self._P = pack(np.broadcast_to(self.C0, (self.N, self.D, self.D)))
        self.lastmean = np.zeros((self.N, self.D)); self.secondlastmean = np.zeros((self.N, self.D))
        self._fallbacks = np.zeros(1, np.int64)

    @property
    def C(self):
        """the chains' covariances, (nchains, D, D) symmetric (what klara_get_am_state returns)"""
        return unpack(self._P, self.D)

    @property
    def fallbacks(self):
        return int(self._fallbacks[0])

    def _sampler_state(self):
        return C.byref(O.KoSamplerState(am_C=self._p(self._P), am_mean=self._p(self.lastmean), am_mean2=self._p(self.secondlastmean),
                                        am_fallbacks=self._p(self._fallbacks)))

    def _init(self) -> int:
        self._P = pack(np.broadcast_to(self.C0, (self.N, self.D, self.D)))      # AM.jl:238-246, 292-304: C = C0, the means = the start value, count = 0
        self.lastmean[...] = self.X; self.secondlastmean[...] = self.X
        self._fallbacks[0] = 0
        return super()._init()            # log-target, finiteness, tuner state (step = 1, totproposed = period)
