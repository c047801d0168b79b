"""Extended-precision (np.longdouble: x87 float80 where the platform has it) restatement of the zero-variance control variates of
stats/variance/zv.jl on a given history: centred cross-products and a hand-written Cholesky solve.  The truth the device results
(klara_get_chain_zv) and the double-precision restatement (klara_jl_amd.stats.lzv / qzv) are held to; no dependency beyond NumPy."""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble


def nterms(d: int, order: int) -> int:
    return d if order == 1 else d * (d + 3) // 2


def controls(x: np.ndarray, g: np.ndarray, order: int) -> np.ndarray:
    """(n x K) control variates from (n x D) values and gradients, in the arithmetic of x's dtype (zv.jl:24, 61-70)."""
    z = -g / 2
    if order == 1:
        return z
    n, d = x.shape
    cols = [z, 2 * z * x - 1]
    pairs = [(i, j) for i in range(d - 1) for j in range(i + 1, d)]                    # i outer, j inner
    if pairs:
        cols.append(np.stack([x[:, i] * z[:, j] + x[:, j] * z[:, i] for i, j in pairs], axis=1))
    return np.concatenate(cols, axis=1)


def cholesky_solve(s: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x with s x = b for a symmetric positive definite s, in the dtype of s: Cholesky, forward and back substitution, written out."""
    k = s.shape[0]
    l = np.zeros_like(s)
    for j in range(k):
        d = s[j, j] - np.sum(l[j, :j] * l[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        l[j, j] = np.sqrt(d)
        for r in range(j + 1, k):
            l[r, j] = (s[r, j] - np.sum(l[r, :j] * l[j, :j])) / l[j, j]
    y = np.zeros_like(b)
    for j in range(k):
        y[j] = (b[j] - l[j, :j] @ y[:j]) / l[j, j]
    x = np.zeros_like(b)
    for j in range(k - 1, -1, -1):
        x[j] = (y[j] - l[j + 1:, j] @ x[j + 1:]) / l[j, j]
    return x


def cross_products(value: np.ndarray, grad: np.ndarray, order: int):
    """(S_ff, S_fx, Fc, Xc) in extended precision: centred control variates and values of an (n x D) history."""
    x = np.asarray(value, dtype=np.float64).astype(LD)
    g = np.asarray(grad, dtype=np.float64).astype(LD)
    f = controls(x, g, order)
    fc = f - f.mean(axis=0)
    xc = x - x.mean(axis=0)
    return fc.T @ fc, fc.T @ xc, fc, xc


def zv_truth(value: np.ndarray, grad: np.ndarray, order: int) -> dict:
    """Everything a check needs on one (n x D) history (the concatenation of several chains' for the pooled form):
    a (K x D), the corrected series, its mean and sample variance — rounded to double —, cond_2(S_ff), and the scale
    sum_k max_t |f_k| of the propagated bound."""
    x = np.asarray(value, dtype=np.float64).astype(LD)
    g = np.asarray(grad, dtype=np.float64).astype(LD)
    sff, sfx, fc, xc = cross_products(value, grad, order)
    a = cholesky_solve(sff, -sfx)
    f = controls(x, g, order)
    series = x + f @ a
    return {"a": a.astype(np.float64), "series": series.astype(np.float64), "mean": series.mean(axis=0).astype(np.float64),
            "var": series.var(axis=0, ddof=1).astype(np.float64), "cond": float(np.linalg.cond(sff.astype(np.float64), 2)),
            "fscale": float(np.abs(f).max(axis=0).sum()), "a_ld": a}


def apply_coef(value: np.ndarray, grad: np.ndarray, order: int, a) -> dict:
    """Corrected series of one chain under GIVEN coefficients (the pooled ones), in extended precision, rounded to double."""
    x = np.asarray(value, dtype=np.float64).astype(LD)
    g = np.asarray(grad, dtype=np.float64).astype(LD)
    f = controls(x, g, order)
    series = x + f @ np.asarray(a).astype(LD)
    return {"series": series.astype(np.float64), "mean": series.mean(axis=0).astype(np.float64), "var": series.var(axis=0, ddof=1).astype(np.float64),
            "fscale": float(np.abs(f).max(axis=0).sum())}


def coef_err(a, a_true) -> float:
    """max |A - A_true| / max |A_true|"""
    a_true = np.asarray(a_true, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - a_true).max() / np.abs(a_true).max())


def coef_bound(cond: float) -> float:
    """16 eps cond_2(S_ff): 1.1 eps cond_2 is what the double-precision restatement and a sequential-sum Cholesky were measured at;
    the factor 16 is headroom for another summation order at n <= 2,000."""
    return 16.0 * EPS * cond
