"""Loader of tests/ram_ref.c, the CPU reference of the RAM kernels — TEST INFRASTRUCTURE (never imported by the product).

The C file is compiled at test time with gcc under the oracle's arithmetic contract (-ffp-contract=off, detmath.h for kd_*) into the
git-ignored build/ directory, and bound to the unchanged oracle library's ko_transition_normals / ko_eval_target.  `RamRefJob` is an
`oracle_ffi.OracleJob` whose descriptor is the job's relabelled as MH (what ko_eval_target and ko_init are handed); its set_state /
reset / run step the RAM sampler instead, and it carries every chain's factor (`.S`, `.skipped`, `set_factor`).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
from pathlib import Path

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
SRC = Path(__file__).resolve().parent / "ram_ref.c"
_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    ora = O.load()
    inputs = [SRC, ROOT / "include" / "klara_hip.h", ROOT / "klara.jl_amd" / "csrc" / "detmath.h"]
    key = hashlib.sha1(b"".join(p.read_bytes() for p in inputs)).hexdigest()[:16]
    out = ROOT / "build" / "ram_ref"
    out.mkdir(parents=True, exist_ok=True)
    so = out / f"ram_ref_{key}.so"
    if not so.exists():
        tmp = out / f".ram_ref_{key}.{os.getpid()}.so"
        r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(ROOT / "include"),
                            "-I", str(ROOT / "klara.jl_amd" / "csrc"), "-o", str(tmp), str(SRC), "-lm"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("tests/ram_ref.c did not compile:\n" + r.stderr)
        tmp.replace(so)
    lib = C.CDLL(str(so))
    vp = C.c_void_p
    lib.rr_bind.argtypes = [vp, vp]
    lib.rr_bind.restype = None
    lib.rr_coef.argtypes = [C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.rr_coef.restype = C.c_double
    lib.rr_update_c.argtypes = [C.c_int, C.c_double, C.c_double, vp, vp]
    lib.rr_update_c.restype = C.c_int
    lib.rr_last.argtypes = [vp, vp]
    lib.rr_last.restype = None
    lib.rr_run.argtypes = [C.POINTER(L.KlaraDesc), C.POINTER(O.KoLayout)] + [vp] * 7 + [C.c_int64, C.c_int64] + [vp] * 5 + [C.c_int64, vp, vp]
    lib.rr_run.restype = C.c_int
    addr = lambda f: C.cast(f, C.c_void_p).value
    lib.rr_bind(addr(ora.ko_transition_normals), addr(ora.ko_eval_target))
    _lib = lib
    return lib


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
    ok = load().rr_update_c(E, float(c), float(zz), w.ctypes.data, P.ctypes.data)
    return unpack(P[None], E)[0], int(ok)


class RamRefJob(O.OracleJob):
    """The RAM sampler on the CPU, with OracleJob's constructor, state arrays and accessors."""

    def __init__(self, *, layout=None, ram_S0=None, ram_targetrate=0.234, ram_gamma=0.7, **kw):
        kw = dict(kw)
        tk = kw.get("target_kind")
        assert tk in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's RAM jobs: logistic or user-defined target"
        assert kw.get("tuner", 0) == L.TUNER_VANILLA and kw.get("tuner_mode", 0) == L.TUNE_PER_CHAIN
        kw["sampler"] = L.SAMPLER_MH                         # relabelled: ko_eval_target / ko_init see an MH job of the same target
        kw["mh_sigma"] = 1.0
        if layout is None:
            nd = int(np.size(kw["logit_y"])) if tk == L.TARGET_LOGISTIC else 0
            layout = O.default_layout(tk, int(kw["ndims"]), nd, sampler=L.SAMPLER_MH)
        super().__init__(layout=layout, **kw)
        self.desc.ram_targetrate, self.desc.ram_gamma = float(ram_targetrate), float(ram_gamma)
        self.rr = load()
        S0 = np.asarray(ram_S0, dtype=np.float64)
        S0 = np.diag(S0.ravel()) if S0.ndim < 2 else S0
        assert S0.shape == (self.D, self.D)
        self.S0 = np.tril(S0)
        self.E = int(self.layout.E)
        self._P = pack(np.broadcast_to(self.S0, (self.N, self.D, self.D)), self.E)
        self._skipped = np.zeros(1, np.int64)

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

    def _init(self) -> int:
        st = super()._init()              # log-target, finiteness, tuner state (MH's: step = 1, totproposed = period)
        self._P = pack(np.broadcast_to(self.S0, (self.N, self.D, self.D)), self.E)      # RAM.jl:155-162, 201-211: S = S0, count = 0
        self._skipped[0] = 0
        return st

    def run(self, nsteps: int) -> int:
        acc = np.zeros((nsteps, self.N), np.uint8) if self.want_accept else None
        self._bind_user()
        self._P = np.ascontiguousarray(self._P)
        st = self.rr.rr_run(C.byref(self.desc), C.byref(self.layout), self._p(self.X), self._p(self.LT), self._p(self._P), self._p(self._skipped),
                            self._p(self.accepted), self._p(self.proposed), self._p(self.totproposed),
                            self.t, int(nsteps), self._p(acc), self._p(self._sum), self._p(self._sumsq), self._p(self.naccept),
                            self._p(self.hist), self.hist_cols, self._p(self.hist_lt), self._p(self.held))
        self.t += int(nsteps)
        if acc is not None:
            self.accept = np.concatenate([self.accept, acc], axis=0)
        return st

    def last_draw(self):
        """(z (E,), c) of the last transition of the last chain stepped"""
        z = np.zeros(8); c = C.c_double(0.0)
        self.rr.rr_last(z.ctypes.data, C.byref(c))
        return z[:self.E].copy(), c.value
