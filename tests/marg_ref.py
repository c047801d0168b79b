"""Shared inputs and helpers of the pooled marginal histogram tests (klara_marg.hip: k_marg_update behind every launch of a job with marg_nbins > 0,
klara_gather_histogram, klara_histogram_quantiles).  The reference is klara_jl_amd.stats.pooled_hist / hist_quantiles, the literal NumPy forms of the
index formula and the quantile rule of include/klara_hip.h; counts are integers, so every comparison is exact.  Histories are (ncols, N, D): column t of
the device's value history is hist[t]."""
import functools
import re
from pathlib import Path

import numpy as np

import klara_jl_amd as K
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
_HDR = (ROOT / "klara.jl_amd" / "csrc" / "klara_marg.h").read_text()


def macro(name):
    return int(re.search(r"#define " + name + r" (\d+)", _HDR).group(1))


THREADS, MAX_DB, LDS_BYTES, SLAB_UNIT, MAX_COLS = (macro("KLARA_MARG_" + n) for n in ("THREADS", "MAX_DB", "LDS_BYTES", "SLAB_UNIT", "MAX_COLS"))


def slab(nbins):
    """chains of a slab (klara_marg.h): a function of nbins alone"""
    return SLAB_UNIT * -(-(nbins + 2) // SLAB_UNIT)


def dims_per_block(D, nbins):
    return min(D, MAX_DB, LDS_BYTES // (4 * ((nbins + 2) | 1)))


NCOLS = 33
SPLITS33 = {"1+31+1": [1, 31, 1], "32+1": [32, 1], "0+32+1+0": [0, 32, 1, 0]}     # more than one piece, empty launches, the same counts for every cut
DIMS = [1, 3, 17, 64, 100, 130]          # < 64: lanes of one instruction collide in one table; 100: no multiple of 64; 130: more than one dimension block
BINS = [1, 2, 64, 1024]
N_ODD = 67                               # not a multiple of 4 or 64


def bounds(D, kind="per_dim"):
    """lo, hi per dimension: different in every dimension, none symmetric"""
    d = np.arange(D, dtype=np.float64)
    if kind == "offset":                 # an offset of 1e6 with width 1e-3
        return 1e6 + 1e-3 * d, 1e6 + 1e-3 * d + 1e-3
    return -2.0 - 0.01 * d, 1.5 + 0.03 * d


@functools.lru_cache(maxsize=None)
def make_hist(ncols, N, D, kind="per_dim"):
    """normal values around the range's middle at a third of its width: a few per cent fall in each outer slot"""
    rng = np.random.default_rng(1000003 * ncols + 1009 * N + D)
    lo, hi = bounds(D, kind)
    h = (lo + hi) / 2 + (hi - lo) / 3 * rng.standard_normal((ncols, N, D))
    h.setflags(write=False)
    return h


def edge_values(nbins, lo, hi):
    """per dimension: every documented edge and its two neighbours, lo, hi and theirs, the infinities and NaN — (nvalues, D)"""
    D = lo.size
    k = np.arange(nbins + 1, dtype=np.float64)[:, None]
    e = lo[None, :] + k * ((hi - lo) / nbins)[None, :]
    rows = [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), lo[None, :], hi[None, :], np.nextafter(lo, -np.inf)[None, :], np.nextafter(hi, -np.inf)[None, :],
            np.nextafter(hi, np.inf)[None, :], np.full((1, D), np.inf), np.full((1, D), -np.inf), np.full((1, D), np.nan), np.full((1, D), -0.0),
            np.full((1, D), 1e308), np.full((1, D), -1e308)]
    return np.concatenate(rows, axis=0)


def edge_hist(N, D, nbins, kind="per_dim"):
    """(ncols, N, D) whose values are edge_values dealt over saved steps and chains (the list repeated to fill the last column)"""
    lo, hi = bounds(D, kind)
    v = edge_values(nbins, lo, hi)
    ncols = -(-v.shape[0] // N)
    idx = np.arange(ncols * N) % v.shape[0]
    return np.ascontiguousarray(v[idx].reshape(ncols, N, D)), lo, hi


def splits_of(ncols):
    out = [MAX_COLS] * (ncols // MAX_COLS)
    if ncols % MAX_COLS:
        out.append(ncols % MAX_COLS)
    return out


def reference(hist, nbins, lo, hi):
    return K.stats.pooled_hist(hist, nbins, lo, hi)


def selftest(hist, splits, nbins, lo, hi, status=False):
    """klara_selftest_marginals on a (ncols, N, D) history: counts (D, nbins + 2), or the status"""
    klib = L.load()
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    ncols, N, D = hist.shape
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float64).ravel(), (D,))); hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float64).ravel(), (D,)))
    spl = np.asarray(splits, dtype=np.int64)
    counts = np.full((D, nbins + 2), 0xDEADBEEF, dtype=np.uint64)
    st = klib.klara_selftest_marginals(0, N, D, ncols, hist.ctypes.data, spl.size, spl.ctypes.data, nbins, lo.ctypes.data, hi.ctypes.data, counts.ctypes.data)
    if status:
        return st
    L.check(st, "klara_selftest_marginals")
    return counts


def quantiles_c(counts, nbins, lo, hi, probs, status=False):
    """klara_histogram_quantiles through ctypes directly"""
    klib = L.load()
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    D = counts.shape[0]
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, np.float64).ravel(), (D,))); hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, np.float64).ravel(), (D,)))
    p = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64)
    out = np.full((D, p.size), -12345.0)
    st = klib.klara_histogram_quantiles(counts.ctypes.data, D, nbins, lo.ctypes.data, hi.ctypes.data, p.size, p.ctypes.data, out.ctypes.data)
    if status:
        return st
    L.check(st, "klara_histogram_quantiles")
    return out


def bits_differ(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))
