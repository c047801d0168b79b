"""Loader of tests/smmala_ref.c, the CPU reference of the SMMALA kernels — TEST INFRASTRUCTURE (never imported by the product).

The C file is compiled at test time with gcc under the oracle's arithmetic contract (-ffp-contract=off, detmath.h for kd_*) into the
git-ignored build/ directory, and bound to the unchanged oracle library's ko_transition_normals / ko_eval_target / rate scores.
`SmmalaRefJob` is an `oracle_ffi.OracleJob` whose descriptor is the job's relabelled as MALA (what ko_eval_target and ko_init are
handed); its set_state / reset / init_state_normal / run step the SMMALA sampler instead.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import subprocess
from pathlib import Path

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
SRC = Path(__file__).resolve().parent / "smmala_ref.c"
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    ora = O.load()
    inputs = [SRC, ROOT / "include" / "klara_hip.h", ROOT / "klara.jl_amd" / "csrc" / "detmath.h"]
    key = hashlib.sha1(b"".join(p.read_bytes() for p in inputs)).hexdigest()[:16]
    out = ROOT / "build" / "smmala_ref"
    out.mkdir(parents=True, exist_ok=True)
    so = out / f"smmala_ref_{key}.so"
    if not so.exists():
        tmp = out / f".smmala_ref_{key}.{__import__('os').getpid()}.so"
        r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(ROOT / "include"),
                            "-I", str(ROOT / "klara.jl_amd" / "csrc"), "-o", str(tmp), str(SRC), "-lm"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("tests/smmala_ref.c did not compile:\n" + r.stderr)
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
    lib.sr_inv_chol_t.argtypes = [vp, C.c_int, vp]
    lib.sr_inv_chol_t.restype = C.c_int
    addr = lambda f: C.cast(f, C.c_void_p).value
    lib.sr_bind(addr(ora.ko_transition_normals), addr(ora.ko_eval_target), addr(ora.ko_logistic_rate_score), addr(ora.ko_erf_rate_score))
    _lib = lib
    return lib


def inv_chol_t(G):
    """C = L^-T for G = L L' (the kernels' factor, SMMALA deviation 1) and whether G factored"""
    G = np.ascontiguousarray(G, dtype=np.float64)
    d = G.shape[0]
    out = np.zeros((d, d))
    ok = load().sr_inv_chol_t(G.ctypes.data, d, out.ctypes.data)
    return out, bool(ok)


class SmmalaRefJob(O.OracleJob):
    """The SMMALA sampler on the CPU, with OracleJob's constructor, state arrays and accessors."""

    def __init__(self, *, layout=None, **kw):
        kw = dict(kw)
        tk = kw.get("target_kind")
        assert tk in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's SMMALA jobs: logistic or user-defined target"
        kw["sampler"] = L.SAMPLER_MALA                       # relabelled: ko_eval_target / ko_init see a MALA job of the same target
        if layout is None:
            nd = int(np.size(kw["logit_y"])) if tk == L.TARGET_LOGISTIC else 0
            layout = O.default_layout(tk, int(kw["ndims"]), nd, sampler=L.SAMPLER_MALA)
        super().__init__(layout=layout, **kw)
        self.sr = load()
        self._tensor = None
        if tk == L.TARGET_CUSTOM:
            self._tensor = C.cast(self._user[0].klara_user_tensorlogtarget, C.c_void_p).value

    def _bind_user(self):
        super()._bind_user()
        self.sr.sr_bind_tensor(self._tensor)

    def _init(self) -> int:
        st = super()._init()              # log-target, gradient, finiteness, tuner state (MALA's: step = driftstep, totproposed = period)
        if st != 0:
            return st
        ok = self.sr.sr_check_init(C.byref(self.desc), C.byref(self.layout), self._p(self.X), self._p(self.G), None)
        return 0 if ok else L.ERR_NONFINITE_INIT

    def run(self, nsteps: int) -> int:
        acc = np.zeros((nsteps, self.N), np.uint8) if self.want_accept else None
        self._bind_user()
        st = self.sr.sr_run(C.byref(self.desc), C.byref(self.layout), self._p(self.X), self._p(self.G), self._p(self.LT),
                            self._p(self.step), self._p(self.accepted), self._p(self.proposed), self._p(self.totproposed),
                            self.t, int(nsteps), self._p(acc), self._p(self._sum), self._p(self._sumsq), self._p(self.naccept),
                            self._p(self.hist), self.hist_cols, self._p(self.hist_lt), self._p(self.hist_g), self._p(self.held))
        self.t += int(nsteps)
        if acc is not None:
            self.accept = np.concatenate([self.accept, acc], axis=0)
        return st

    def metric(self, x):
        """the metric the kernels form at x (logistic: X' diag(r (1 - r)) X, without I / lambda; user-defined: the tensor), D x D"""
        self._bind_user()
        E, D = self.layout.E, self.D
        tri = np.zeros(E * (E + 1) // 2)
        xe = np.ascontiguousarray(x, dtype=np.float64).ravel()
        self.sr.sr_metric(C.byref(self.desc), C.byref(self.layout), xe.ctypes.data, tri.ctypes.data)
        G = np.zeros((E, E))
        k = 0
        for a in range(E):
            for b in range(a, E):
                G[a, b] = G[b, a] = tri[k]
                k += 1
        return G[:D, :D]
