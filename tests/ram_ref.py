"""The RAM sampler on the CPU oracle (oracle/klara_oracle.c ko_ram) — TEST INFRASTRUCTURE (never imported by the product).

`RamRefJob` is an `oracle_ffi.OracleJob` of sampler id KLARA_SAMPLER_RAM that carries every chain's factor (`.S`, `.skipped`,
`set_factor`) and hands it to ko_init / ko_run as the oracle's ko_sampler_state.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L


def pack(S, E):
    """(n, D, D) lower-triangular factors -> (n, E (E + 1) / 2) packed E x E factors, the identity in the padding (ktri(j, i, E) = S_ij)"""
    S = np.asarray(S, dtype=np.float64)
    n, D = S.shape[0], S.shape[1]
    out = np.zeros((n, E * (E + 1) // 2))
    k = 0
    for j in range(E):
        for i in range(j, E):
            out[:, k] = S[:, i, j] if i < D else (1.0 if i == j else 0.0)
            k += 1
    return out


def unpack(P, E, D=None):
    """the inverse of pack: (n, D, D) with zeros above the diagonal (D = E: the padded block too)"""
    D = E if D is None else D
    out = np.zeros((P.shape[0], D, D))
    k = 0
    for j in range(E):
        for i in range(j, E):
            if i < D:
                out[:, i, j] = P[:, k]
            k += 1
    return out


def update_c(S, c, zz, w):
    """ram_update from c on, on one E x E factor: (new factor, 1) or (the factor as it was, 0)"""
    S = np.asarray(S, dtype=np.float64)
    E = S.shape[0]
    P = np.ascontiguousarray(pack(S[None], E)[0])
    w = np.ascontiguousarray(w, dtype=np.float64)
    ok = O.load().ko_ram_update_c(E, float(c), float(zz), w.ctypes.data, P.ctypes.data)
    return unpack(P[None], E)[0], int(ok)


class RamRefJob(O.OracleJob):
    """The RAM sampler on the CPU, with OracleJob's constructor, state arrays and accessors."""

    def __init__(self, *, ram_S0=None, ram_targetrate=0.234, ram_gamma=0.7, sampler=L.SAMPLER_RAM, **kw):
        assert sampler == L.SAMPLER_RAM
        assert kw.get("target_kind") in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's RAM jobs: logistic or user-defined target"
        assert kw.get("tuner", 0) == L.TUNER_VANILLA and kw.get("tuner_mode", 0) == L.TUNE_PER_CHAIN
        super().__init__(sampler=sampler, **kw)
        self.desc.ram_targetrate, self.desc.ram_gamma = float(ram_targetrate), float(ram_gamma)
        S0 = np.asarray(ram_S0, dtype=np.float64)
        S0 = np.diag(S0.ravel()) if S0.ndim < 2 else S0
        assert S0.shape == (self.D, self.D)
        self.S0 = np.tril(S0)
        self.E = int(self.layout.E)
        self._P = pack(np.broadcast_to(self.S0, (self.N, self.D, self.D)), self.E)
        self._skipped = np.zeros(1, np.int64)
        self._before = None

    @property
    def S(self):
        """the chains' factors, (nchains, D, D) lower triangular (what klara_get_ram_factor returns)"""
        return unpack(self._P, self.E, self.D)

    @property
    def S_padded(self):
        """... over all E elements of the lane: (nchains, E, E), the identity block in the padding"""
        return unpack(self._P, self.E)

    @property
    def skipped(self):
        return int(self._skipped[0])

    def set_factor(self, S):
        S = np.broadcast_to(np.asarray(S, dtype=np.float64), (self.N, self.D, self.D))
        self._P = pack(np.tril(S), self.E)

    def _sampler_state(self):
        self._P = np.ascontiguousarray(self._P)
        self._before = (self.t, self.X[-1].copy(), float(self.LT[-1]), self._P[-1].copy())      # (for last_draw)
        return C.byref(O.KoSamplerState(ram_S=self._p(self._P), ram_skipped=self._p(self._skipped)))

    def _init(self) -> int:
        self._P = pack(np.broadcast_to(self.S0, (self.N, self.D, self.D)), self.E)      # RAM.jl:155-162, 201-211: S = S0, count = 0
        self._skipped[0] = 0
        return super()._init()            # log-target, finiteness, tuner state (step = 1, totproposed = period)

    def last_draw(self):
        """(z (E,), c) of the last transition of the last chain: ko_ram_step again over the last run()'s transitions, from that chain's state before it"""
        t0, x, lt, P = self._before
        x, P, lt = x.copy(), P.copy(), C.c_double(lt)
        z = np.zeros(8); c = C.c_double(0.0)
        self._bind_user()
        for t in range(t0, self.t):
            self.lib.ko_ram_step(C.byref(self.desc), C.byref(self.layout), int(self.desc.chain_offset) + self.N - 1, t, x.ctypes.data,
                                 C.byref(lt), P.ctypes.data, z.ctypes.data, C.byref(c))
        return z[:self.E].copy(), c.value
