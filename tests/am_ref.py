"""Loader of tests/am_ref.c, the CPU reference of the AM kernels — TEST INFRASTRUCTURE (never imported by the product).

The C file is compiled at test time with gcc under the oracle's arithmetic contract (-ffp-contract=off, detmath.h for kd_*) into the
git-ignored build/ directory, and bound to the unchanged oracle library's ko_transition_normals / ko_eval_target.  `AmRefJob` is an
`oracle_ffi.OracleJob` whose descriptor is the job's relabelled as MH (what ko_eval_target and ko_init are handed); its set_state /
reset / run step the AM sampler instead, and it carries every chain's covariance and running means (`.C`, `.lastmean`,
`.secondlastmean`, `.fallbacks`).
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
SRC = Path(__file__).resolve().parent / "am_ref.c"
_lib = None


def _inputs():
    return [SRC, ROOT / "include" / "klara_hip.h", ROOT / "klara.jl_amd" / "csrc" / "detmath.h", ROOT / "klara.jl_amd" / "csrc" / "detmath_tables.h"]


def _compile(out: Path, extra):
    tmp = out.with_name(f".{out.name}.{os.getpid()}")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", *extra, "-I", str(ROOT / "include"),
                        "-I", str(ROOT / "klara.jl_amd" / "csrc"), "-o", str(tmp), str(SRC), "-lm"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("tests/am_ref.c did not compile:\n" + r.stderr)
    tmp.replace(out)


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    ora = O.load()
    key = hashlib.sha1(b"".join(p.read_bytes() for p in _inputs())).hexdigest()[:16]
    out = ROOT / "build" / "am_ref"
    out.mkdir(parents=True, exist_ok=True)
    so = out / f"am_ref_{key}.so"
    if not so.exists():
        _compile(so, ["-fPIC", "-shared"])
    lib = C.CDLL(str(so))
    vp = C.c_void_p
    lib.ar_bind.argtypes = [vp, vp]
    lib.ar_bind.restype = None
    lib.ar_selector.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    lib.ar_selector.restype = C.c_double
    lib.ar_covariance.argtypes = [C.c_int, C.c_int64, vp, vp, vp, vp]
    lib.ar_covariance.restype = None
    lib.ar_factor.argtypes = [C.c_int, C.c_double, vp, vp]
    lib.ar_factor.restype = C.c_int
    lib.ar_run.argtypes = [C.POINTER(L.KlaraDesc), C.POINTER(O.KoLayout)] + [vp] * 9 + [C.c_int64, C.c_int64] + [vp] * 5 + [C.c_int64, vp, vp]
    lib.ar_run.restype = C.c_int
    addr = lambda f: C.cast(f, C.c_void_p).value
    lib.ar_bind(addr(ora.ko_transition_normals), addr(ora.ko_eval_target))
    _lib = lib
    return lib


def sanitizer_program() -> Path:
    """tests/am_ref.c with its own main (AM_REF_MAIN), built with -fsanitize=address,undefined: a stand-alone host program"""
    key = hashlib.sha1(b"".join(p.read_bytes() for p in _inputs())).hexdigest()[:16]
    out = ROOT / "build" / "am_ref"
    out.mkdir(parents=True, exist_ok=True)
    exe = out / f"am_ref_main_{key}"
    if not exe.exists():
        _compile(exe, ["-g", "-DAM_REF_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    return exe


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

    def __init__(self, *, layout=None, am_C0=None, am_corescale=1.0, am_minorscale=1.0, am_c=0.05, am_t0=10, **kw):
        kw = dict(kw)
        tk = kw.get("target_kind")
        assert tk in (L.TARGET_LOGISTIC, L.TARGET_CUSTOM), "the reference covers the device's AM jobs: logistic or user-defined target"
        assert kw.get("tuner", 0) == L.TUNER_VANILLA and kw.get("tuner_mode", 0) == L.TUNE_PER_CHAIN
        kw["sampler"] = L.SAMPLER_MH                         # relabelled: ko_eval_target / ko_init see an MH job of the same target
        kw["mh_sigma"] = 1.0
        if layout is None:
            nd = int(np.size(kw["logit_y"])) if tk == L.TARGET_LOGISTIC else 0
            layout = O.default_layout(tk, int(kw["ndims"]), nd, sampler=L.SAMPLER_MH)
        super().__init__(layout=layout, **kw)
        d = self.desc
        d.am_corescale, d.am_minorscale, d.am_c, d.am_t0 = float(am_corescale), float(am_minorscale), float(am_c), int(am_t0)
        self.ar = load()
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

    def _init(self) -> int:
        st = super()._init()              # log-target, finiteness, tuner state (MH's: step = 1, totproposed = period)
        self._P = pack(np.broadcast_to(self.C0, (self.N, self.D, self.D)))      # AM.jl:238-246, 292-304: C = C0, the means = the start value, count = 0
        self.lastmean[...] = self.X; self.secondlastmean[...] = self.X
        self._fallbacks[0] = 0
        return st

    def run(self, nsteps: int) -> int:
        acc = np.zeros((nsteps, self.N), np.uint8) if self.want_accept else None
        self._bind_user()
        st = self.ar.ar_run(C.byref(self.desc), C.byref(self.layout), self._p(self.X), self._p(self.LT), self._p(self._P), self._p(self.lastmean),
                            self._p(self.secondlastmean), self._p(self._fallbacks),
                            self._p(self.accepted), self._p(self.proposed), self._p(self.totproposed),
                            self.t, int(nsteps), self._p(acc), self._p(self._sum), self._p(self._sumsq), self._p(self.naccept),
                            self._p(self.hist), self.hist_cols, self._p(self.hist_lt), self._p(self.held))
        self.t += int(nsteps)
        if acc is not None:
            self.accept = np.concatenate([self.accept, acc], axis=0)
        return st
