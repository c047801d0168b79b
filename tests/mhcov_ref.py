"""Random-walk Metropolis with a full proposal covariance, MH(Σ), on the CPU — TEST INFRASTRUCTURE (never imported by the product).

The transition of DESIGN.md section 2 (MH(Σ), C1-C3) in plain Python floats over the primitives the CPU oracle exports through tests/oracle_ffi.py, with no C
of its own: ko_eval_target (the log-target in the device's summation order; the oracle is given a descriptor whose sampler is MH, it does not know id 12),
ko_transition_normals (MH's D normals of a transition and its accept uniform) and ko_math (kd_log_u01).

`MhCovRefJob` carries X, LT, the accept mask `accept` and count `naccept`, the running sums in sojourn form as the group-layout kernels fold them (the state
being left is folded when a proposal is accepted), and the value / log-target history under the save rule.  `factor` may be replaced between runs
(klara_set_mh_factor); reset() puts the job's own back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L

OP_LOG_U01 = 7        # oracle/klara_oracle.c ko_math


def propose(x, factor, z):
    """x' = x + L z, row i as w_i = L_i0 z_0, then w_i = w_i + L_ik z_k for k = 1 .. i ascending (C1): Python floats, one rounding per operation"""
    D = len(x)
    xp = np.empty(D)
    for i in range(D):
        w = float(factor[i, 0]) * float(z[0])
        for k in range(1, i + 1):
            w = w + float(factor[i, k]) * float(z[k])
        xp[i] = float(x[i]) + w
    return xp


def tune_counts(accept, period: int, burnin: int):
    """(accepted, proposed, totproposed) per chain after the transitions of the accept mask under VanillaMCTuner(period, verbose=true), counted as for MH
    (iterate/MH.jl:73-75, 99, 104-110 with tuners.jl:27-32): totproposed starts at the period; while it does not exceed the burn-in, every `period`
    proposals close a report (totproposed += proposed, both counts cleared)"""
    n = accept.shape[1]
    out = np.zeros((3, n), np.int64)
    for c in range(n):
        a, p, tot = 0, 0, int(period)
        for s in range(accept.shape[0]):
            p += 1
            a += int(accept[s, c])
            if tot <= burnin and p % period == 0:
                tot += p; a = 0; p = 0
        out[:, c] = (a, p, tot)
    return out[0], out[1], out[2]


class MhCovRefJob:
    def __init__(self, *, target_kind, nchains, ndims, nsteps, mh_factor, burnin=0, thinning=1, seed=20260927, chain_offset=0, layout=None,
                 want_hist=False, sampler=L.SAMPLER_MH_COV, tuner=L.TUNER_VANILLA, verbose=False, period=100, **target_kw):
        assert sampler == L.SAMPLER_MH_COV and tuner == L.TUNER_VANILLA
        self.N, self.D = int(nchains), int(ndims)
        # the oracle evaluates the target only: an MH descriptor of the same target, layout and data
        self._o = O.OracleJob(sampler=L.SAMPLER_MH, target_kind=target_kind, nchains=1, ndims=ndims, nsteps=nsteps, mh_sigma=np.ones(self.D),
                              seed=seed, layout=layout, want_accept=False, want_sums=False, **target_kw)
        self.lib = self._o.lib
        self.layout = self._o.layout
        self.nsteps, self.burnin, self.thinning = int(nsteps), int(burnin), int(thinning)
        self.chain_offset = int(chain_offset)
        self._seed0, self.epoch, self.seed = int(seed), 0, int(seed)
        f = np.asarray(mh_factor, dtype=np.float64)
        assert f.shape == (self.D, self.D)
        self.factor0 = np.tril(f).copy()
        self.factor = self.factor0.copy()
        self.X = np.zeros((self.N, self.D)); self.LT = np.zeros(self.N)
        self.hist_cols = (self.nsteps - self.burnin - 1) // self.thinning + 1
        self.want_hist = bool(want_hist)
        self._xbuf = np.zeros(self.D); self._gbuf = np.zeros(self.D); self._lt = C.c_double(0.0)
        self._zbuf = np.zeros(self.D); self._u = C.c_double(0.0)
        self._args = (C.byref(self._o.desc), C.byref(self._o.layout), self._xbuf.ctypes.data, C.byref(self._lt), self._gbuf.ctypes.data)

    # -- the oracle's primitives
    def eval(self, x) -> float:
        self._xbuf[:] = x
        st = self.lib.ko_eval_target(*self._args)
        assert st == 0
        return self._lt.value

    def normals(self, chain: int, t: int):
        self.lib.ko_transition_normals(self.seed, chain, t, self.D, self._zbuf.ctypes.data, C.byref(self._u))
        return self._zbuf.copy(), self._u.value

    # -- start states and the factor
    def set_state(self, x) -> int:
        """klara_set_state: the factor is the job's, not a chain's — it stays"""
        self.X[...] = np.asarray(x, dtype=np.float64).reshape(self.N, self.D)
        return self._init()

    def set_factor(self, factor) -> None:
        self.factor = np.tril(np.asarray(factor, dtype=np.float64)).copy()

    def reset(self, x=None) -> int:
        """reset(job[, x]): the next Philox key (include/klara_hip.h klara_reset) and the descriptor's factor again"""
        self.epoch += 1
        self.seed = (self._seed0 + self.epoch * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        self.factor = self.factor0.copy()
        if x is not None:
            self.X[...] = np.asarray(x, dtype=np.float64).reshape(self.N, self.D)
        return self._init()

    def _init(self) -> int:
        self._o._bind_user()
        self.t = 0
        self.naccept = np.zeros(self.N, np.uint64)
        self.accept = np.zeros((0, self.N), np.uint8)
        self._sum = np.zeros((self.N, self.D)); self._sumsq = np.zeros((self.N, self.D)); self.held = np.zeros(self.N, np.int64)
        self.hist = np.zeros((self.hist_cols, self.N, self.D)) if self.want_hist else None
        self.hist_lt = np.zeros((self.hist_cols, self.N)) if self.want_hist else None
        for c in range(self.N):
            self.LT[c] = self.eval(self.X[c])
        return 0 if np.all(np.isfinite(self.LT)) else L.ERR_NONFINITE_INIT

    @property
    def sum(self):
        return self._sum + self.held[:, None].astype(np.float64) * self.X

    @property
    def sumsq(self):
        return self._sumsq + self.held[:, None].astype(np.float64) * (self.X * self.X)

    # -- the transition
    def step(self, c: int, t: int) -> bool:
        """one transition of chain c (local index): iterate/MH.jl:72-124, symmetric normalised branch, with the proposal x + L z"""
        z, u = self.normals(self.chain_offset + c, t)
        with np.errstate(all="ignore"):
            xp = propose(self.X[c], self.factor, z)                # MH.jl:79 with MvNormal(x, Σ)
            ltp = self.eval(xp)                                    # :81
            ratio = ltp - self.LT[c]                               # :83
        acc = bool(ratio > 0.0 or ratio > float(O.math_op(OP_LOG_U01, np.array([u]))[0]))      # :97 (a NaN or -inf ratio fails both: rejected)
        if acc:
            if self.held[c] > 0:                                   # the fold of the state being left (KParams::held)
                hf = float(self.held[c])
                with np.errstate(all="ignore"):                    # (a state of 1e154 has an infinite square: the kernels form it too)
                    self._sum[c] = self._sum[c] + hf * self.X[c]
                    self._sumsq[c] = self._sumsq[c] + hf * (self.X[c] * self.X[c])
                self.held[c] = 0
            self.X[c] = xp; self.LT[c] = ltp                       # :98-100
        return acc

    def run(self, nsteps: int) -> int:
        self._o._bind_user()
        acc = np.zeros((nsteps, self.N), np.uint8)
        for s in range(nsteps):
            t = self.t + s
            i1 = t + 1
            save = i1 > self.burnin and i1 <= self.nsteps and (i1 - self.burnin - 1) % self.thinning == 0
            col = (i1 - self.burnin - 1) // self.thinning
            for c in range(self.N):
                acc[s, c] = self.step(c, t)
                if save:
                    self.held[c] += 1
                    if self.hist is not None and col < self.hist_cols:
                        self.hist[col, c] = self.X[c]; self.hist_lt[col, c] = self.LT[c]
        self.t += nsteps
        self.accept = np.concatenate([self.accept, acc], axis=0)
        self.naccept += acc.sum(axis=0).astype(np.uint64)
        return 0
