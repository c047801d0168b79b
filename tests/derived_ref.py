"""The reference of the derived quantities: the closure's own C text built by gcc through oracle_ffi.build_c with the arithmetic contract of the device
(-O2 -std=gnu11 -ffp-contract=off, detmath.h for kd_*, KLARA_USER_FN empty) and evaluated on host arrays; the sums in the order the contract states;
the geometry of klara.jl_amd/csrc/klara_derived.h restated; the self-test call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
_HDR = (ROOT / "klara.jl_amd" / "csrc" / "klara_derived.h").read_text()


def macro(name):
    return int(re.search(r"#define " + name + r"\s+(\d+)", _HDR).group(1))


LDS_BYTES, MAX_CH, MAX_COLS = macro("KLARA_DERIVED_LDS_BYTES"), macro("KLARA_DERIVED_MAX_CH"), macro("KLARA_DERIVED_MAX_COLS")
_libs = {}


def _host(src, D, K):
    key = (src, int(D), int(K))
    if key not in _libs:
        text = (f'#include "detmath.h"\n#define KLARA_USER_FN\n#define KLARA_D {int(D)}\n#define KLARA_K {int(K)}\n#line 1 "klara_user_derived"\n{src}\n'
                '#line 1 "derived_ref_glue"\n'
                'void derived_eval(const double* x, long long n, const double* data, long long ndata, double* out)\n'
                '{ for (long long i = 0; i < n; ++i) klara_user_derived(x + i * KLARA_D, KLARA_D, data, ndata, out + i * KLARA_K, KLARA_K); }\n')
        so = O.build_c("derived_ref", ["-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", "-I", str(O.CSRC)], text=text,
                       hashed=[O.CSRC / "detmath.h", O.CSRC / "detmath_tables.h"])
        lib = C.CDLL(str(so))
        lib.derived_eval.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
        lib.derived_eval.restype = None
        _libs[key] = lib
    return _libs[key]


def evaluate(src, K, values, data=None):
    """y = klara_user_derived(x) for every sample of `values` (..., D): (..., K)"""
    x = np.ascontiguousarray(values, dtype=np.float64)
    D = x.shape[-1]
    d = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
    out = np.empty(x.shape[:-1] + (K,))
    _host(src, D, K).derived_eval(x.ctypes.data, x.size // D, None if d is None else d.ctypes.data, 0 if d is None else d.size, out.ctypes.data)
    return out


def sums(y):
    """(sum, sumsq) [N, K] of y [ncols, N, K] in ascending column: s = s + y, q = q + y * y — the product rounded, then added"""
    s = np.zeros(y.shape[1:]); q = np.zeros(y.shape[1:])
    with np.errstate(all="ignore"):
        for t in range(y.shape[0]):
            s = s + y[t]
            q = q + y[t] * y[t]
    return s, q


def reference(src, K, hist, data=None):
    y = evaluate(src, K, hist, data)
    return sums(y) + (y,)


def geometry(N, D, K):
    """klara_derived.h: (chains per workgroup, doubles per LDS row, threads, workgroups, LDS bytes) from (N, D, K) alone"""
    stride = D | 1
    ch = min(MAX_CH, LDS_BYTES // (8 * stride))
    return ch, stride, 64 * ((ch + 63) // 64), (N + ch - 1) // ch, 8 * ch * stride


def plan(N, D, K, status=False):
    ch, stride, thr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    nwg, lds = C.c_int64(0), C.c_int64(0)
    st = L.load().klara_selftest_derived_plan(int(N), int(D), int(K), C.byref(ch), C.byref(stride), C.byref(thr), C.byref(nwg), C.byref(lds))
    if status:
        return st
    L.check(st, "klara_selftest_derived_plan")
    return ch.value, stride.value, thr.value, nwg.value, lds.value


def selftest(hist, splits, src, K, data=None, values=True, status=False, device=0):
    """klara_selftest_derived on hist (ncols, N, D): (sum, sumsq, values or None)"""
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    ncols, N, D = hist.shape
    spl = np.ascontiguousarray(splits, dtype=np.int64)
    d = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
    s = np.full((N, K), np.nan); q = np.full((N, K), np.nan)
    v = np.full((ncols, N, K), np.nan) if values else None
    st = L.load().klara_selftest_derived(device, N, D, ncols, hist.ctypes.data, spl.size, spl.ctypes.data, src.encode(), K,
                                          None if d is None else d.ctypes.data, 0 if d is None else d.size, s.ctypes.data, q.ctypes.data,
                                          None if v is None else v.ctypes.data)
    if status:
        return st
    L.check(st, "klara_selftest_derived")
    return s, q, v


def bits_differ(a, b):
    """elements whose bit patterns differ; two NaNs count as equal whatever their payloads (the host's and the device's NaN need not share one)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return int(np.count_nonzero(~same))
