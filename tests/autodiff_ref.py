"""Host build of a forward-mode autodiff source (KLARA_USER_AUTODIFF) — TEST INFRASTRUCTURE (never imported by the product).

`build(src, ndims, chunk)` compiles, with g++ -O2 -std=c++17 -ffp-contract=off, the same user text between the same prelude and glue
(klara.jl_amd/csrc/klara_autodiff.h) the run-time compiler puts around it on the device, and exports klara_user_logtarget,
klara_user_gradlogtarget and (marker value 2) klara_user_tensorlogtarget with C linkage — the closures the CPU oracle takes as function
pointers.  The gradient is swept `chunk` directions at a time (default 1: invariant A2 of the header makes the width
immaterial); klara_ref_dual_value is the value a dual carries through the user's function (invariant A1: the double instantiation's bits).

`AdOracleJob` / `AdSmmalaRefJob` are oracle_ffi.OracleJob / smmala_ref.SmmalaRefJob on such a source: their constructors compile a source
with gcc as C first, so they are handed a stub C source that carries the same form markers, and the pointers are swapped before the
first evaluation."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import oracle_ffi as O
import smmala_ref
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "klara.jl_amd" / "csrc"
_libs = {}

_SIG = "const double* x, int D, const double* data, long long ndata"
_GLUE = r"""
extern "C" {
double klara_user_logtarget(%(sig)s);
void klara_user_gradlogtarget(%(sig)s, double* g);
void klara_user_tensorlogtarget(%(sig)s, double* G);
double klara_user_loglikelihood(%(sig)s);
double klara_user_logprior(%(sig)s);
void klara_user_gradloglikelihood(%(sig)s, double* g);
void klara_user_gradlogprior(%(sig)s, double* g);
double klara_ref_dual_value(%(sig)s);
}
#line 1 "klara_autodiff_glue"
#define KLARA_AUTODIFF_GLUE 1
#include "klara_autodiff.h"
#line 1 "klara_custom_glue"
#include "klara_custom_compose.h"
double klara_ref_dual_value(%(sig)s)
{
    const klara_ad_view<1> view = { x, 0 };
#ifdef KLARA_USER_LIKELIHOOD_PRIOR
    return klara_user_loglikelihood_ad<klara_dual<double, 1> >(view, D, data, ndata).v + klara_user_logprior_ad<klara_dual<double, 1> >(view, D, data, ndata).v;
#else
    return klara_user_logtarget_ad<klara_dual<double, 1> >(view, D, data, ndata).v;
#endif
}
""" % {"sig": _SIG}


def build(src: str, ndims: int, chunk: int = 1, chunk2: int = 1):
    """ctypes library of the host build; `chunk` directions per gradient sweep, `chunk2` inner directions per Hessian sweep"""
    key = (int(ndims), int(chunk), int(chunk2), src)
    if key in _libs:
        return _libs[key]
    text = (f'#include "klara_autodiff.h"\n#define KLARA_D {int(ndims)}\n#define KLARA_USER_FN\n#define KLARA_SMMALA 1\n'
            f'#line 1 "klara_user_target"\n{src}\n'
            f'#undef KLARA_USER_AUTODIFF_CHUNK\n#define KLARA_USER_AUTODIFF_CHUNK {int(chunk)}\n#define KLARA_AD_CHUNK2 {int(chunk2)}\n' + _GLUE)
    so = O.build_c("autodiff_ref", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(CSRC)], text=text, text_suffix=".cpp",
                   hashed=[CSRC / "klara_autodiff.h", CSRC / "detmath.h", CSRC / "klara_custom_compose.h"], libs=(), cc="g++")
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    for name in ("klara_user_logtarget", "klara_ref_dual_value"):
        getattr(lib, name).restype = C.c_double
        getattr(lib, name).argtypes = [dp, C.c_int, dp, C.c_longlong]
    for name in ("klara_user_gradlogtarget", "klara_user_tensorlogtarget"):
        if hasattr(lib, name):
            getattr(lib, name).restype = None
            getattr(lib, name).argtypes = [dp, C.c_int, dp, C.c_longlong, dp]
    _libs[key] = lib
    return lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class HostTarget:
    """value / gradient / minus-Hessian of a host build at a point"""

    def __init__(self, src, ndims, data=None, chunk=1, chunk2=1):
        self.lib, self.d = build(src, ndims, chunk, chunk2), int(ndims)
        self.data = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
        self.nd = 0 if self.data is None else self.data.size

    def value(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        return self.lib.klara_user_logtarget(_dp(x), self.d, _dp(self.data), self.nd)

    def dual_value(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        return self.lib.klara_ref_dual_value(_dp(x), self.d, _dp(self.data), self.nd)

    def grad(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.zeros(self.d)
        self.lib.klara_user_gradlogtarget(_dp(x), self.d, _dp(self.data), self.nd, _dp(g))
        return g

    def tensor(self, x):
        """upper triangle of minus the Hessian, mirrored"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        G = np.zeros((self.d, self.d))
        self.lib.klara_user_tensorlogtarget(_dp(x), self.d, _dp(self.data), self.nd, _dp(G))
        return np.triu(G) + np.triu(G, 1).T


_STUB = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata) { return 0.0; }
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g) { }
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G) { }
"""
_STUB_PARTS = r"""#define KLARA_USER_LIKELIHOOD_PRIOR 1
KLARA_USER_FN double klara_user_loglikelihood(const double* x, int D, const double* data, long long ndata) { return 0.0; }
KLARA_USER_FN double klara_user_logprior(const double* x, int D, const double* data, long long ndata) { return 0.0; }
KLARA_USER_FN void klara_user_gradloglikelihood(const double* x, int D, const double* data, long long ndata, double* g) { }
KLARA_USER_FN void klara_user_gradlogprior(const double* x, int D, const double* data, long long ndata, double* g) { }
"""


def _stub_for(src):
    return _STUB_PARTS if "KLARA_USER_LIKELIHOOD_PRIOR" in src else _STUB


def _pointers(lib):
    ptr = lambda n: C.cast(getattr(lib, n), C.c_void_p)
    return ptr("klara_user_logtarget"), ptr("klara_user_gradlogtarget")


class AdOracleJob(O.OracleJob):
    """OracleJob on an autodiff source: the oracle steps the host build's value and gradient"""

    def __init__(self, *, custom_src, chunk=1, **kw):
        super().__init__(custom_src=_stub_for(custom_src), **kw)
        self.ad = build(custom_src, self.D, chunk)
        lt, grad = _pointers(self.ad)
        self._user = (self.ad, lt, grad, None)


class AdSmmalaRefJob(smmala_ref.SmmalaRefJob):
    """SmmalaRefJob on an autodiff source of order 2: the metric is the host build's minus-Hessian"""

    def __init__(self, *, custom_src, chunk=1, **kw):
        super().__init__(custom_src=_stub_for(custom_src), **kw)
        self.ad = build(custom_src, self.D, chunk)
        lt, grad = _pointers(self.ad)
        self._user = (self.ad, lt, grad, None)
        self._tensor = C.cast(self.ad.klara_user_tensorlogtarget, C.c_void_p)


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    """the CPU reference of an autodiff_cases job"""
    import cases
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    cls = AdSmmalaRefJob if case["sampler"] == L.SAMPLER_SMMALA else AdOracleJob
    if layout is None:
        kw.pop("layout")
    return cls(want_hist=want_hist, **kw)
