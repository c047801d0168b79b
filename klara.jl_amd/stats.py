"""Post-hoc chain statistics of the reference (src/stats/**) on the saved values of a chain.

These consume the path's output.  `mean`, iid variance and `acceptance` for ALL chains come from
the on-device running sums / accept masks (api.py), and every estimator below also exists on the device for every (chain, dimension)
series at once — post hoc over a stored history (klara_get_chain_mcvar / _ipse) and, for :bm / :imse / :ipse, accumulated while
sampling (klara_get_chain_bm, klara_get_chain_acov_mcvar).  This module is the NumPy restatement of the reference's estimators on one
chain's history: what the device versions are tested against.

  mcvar(v, "iid")            var(v)/length(v)                                  stats/variance/mcvar.jl:5
  mcvar(v, "bm", batchlen)   batch means, Flegal & Jones 2010                  mcvar.jl:35-41
  mcvar(v, "imse"|"ipse")    Geyer's initial monotone / positive sequence      mcvar.jl:75-105, 137-158
  mcse = sqrt(mcvar);  ess = len*iidvar/mcvar (convergence/ess.jl:3);  iact = mcvar/iidvar (convergence/iact.jl:3)
  lzv / qzv(chain, grad)     zero-variance control variates, linear / quadratic       stats/variance/zv.jl:9-84
                             (device: klara_get_chain_zv, which solves by Cholesky instead of inv — DESIGN.md §2)
`v` is a 1-D series; the `*_chain` helpers apply an estimator to every dimension of a (D x n) NState value matrix.
"""
from __future__ import annotations

import numpy as np


def autocov(v: np.ndarray, maxlag: int) -> np.ndarray:
    """StatsBase.autocov(v, 0:maxlag) (demean=true): sum_t (v_t - m)(v_{t+k} - m) / n."""
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    z = v - v.mean()
    nfft = 1 << int(np.ceil(np.log2(2 * n)))
    f = np.fft.rfft(z, nfft)
    ac = np.fft.irfft(f * np.conj(f), nfft)[: maxlag + 1]
    return ac / n


def mcvar(v, vtype: str = "imse", *args) -> float:
    v = np.asarray(v, dtype=np.float64).ravel()
    n = v.size
    if vtype == "iid":
        return float(v.var(ddof=1) / n)
    if vtype == "bm":
        batchlen = int(args[0]) if args else 100
        nbatches = n // batchlen
        assert nbatches > 1, "Choose batch size such that the number of batches is greather than one"
        nbsamples = nbatches * batchlen
        bm = v[:nbsamples].reshape(nbatches, batchlen).mean(axis=1)
        return float(batchlen * bm.var(ddof=1) / nbsamples)
    if vtype in ("imse", "ipse"):
        maxlag = int(args[0]) if args else n - 1
        k = int(np.floor((maxlag - 1) / 2))
        acv = autocov(v, maxlag)
        g = np.empty(k + 1)
        m = k + 1
        for j in range(k + 1):
            g[j] = acv[2 * j] + acv[2 * j + 1]
            if g[j] <= 0:
                m = j
                break
        if vtype == "imse" and m > 1:
            for j in range(1, m):
                if g[j] > g[j - 1]:
                    g[j] = g[j - 1]
        return float((-acv[0] + 2.0 * g[:m].sum()) / n)
    raise ValueError(f"unknown variance type {vtype!r}")


def mcse(v, vtype: str = "imse", *args) -> float:
    return float(np.sqrt(mcvar(v, vtype, *args)))


def ess(v, vtype: str = "imse", *args) -> float:
    v = np.asarray(v, dtype=np.float64).ravel()
    return float(v.size * mcvar(v, "iid") / mcvar(v, vtype, *args))


def iact(v, vtype: str = "imse", *args) -> float:
    return float(mcvar(v, vtype, *args) / mcvar(v, "iid"))


def pooled_cov(values) -> np.ndarray:
    """cov of the concatenated histories: `values` is (nchains, ndims, nsaved) — or a sequence of (ndims, nsaved) chains in NState layout —;
    the literal NumPy form of what a job with covariance=True accumulates on the device (klara_gather_covariance's m2 / (n - 1))."""
    x = np.concatenate([np.asarray(v, dtype=np.float64) for v in values], axis=1)      # (ndims, nchains * nsaved)
    xc = x - x.mean(axis=1, keepdims=True)
    return (xc @ xc.T) / (x.shape[1] - 1)


def derived_sums(values, f):
    """(sum[N, K], sumsq[N, K]) of y = f(x) over the saved steps of every chain — the literal NumPy form of what a job with derived= accumulates on the
    device (klara_get_derived_sums): `values` is (nsaved, N, D), `f` a Python callable from a (D,) sample to K numbers; per chain, in ascending saved
    step, sum = sum + y and sumsq = sumsq + y * y, one rounded product and one addition per step."""
    x = np.asarray(values, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f"values must be (nsaved, nchains, ndims), not {x.shape}")
    nsaved, N, _ = x.shape
    s = q = None
    with np.errstate(all="ignore"):
        for t in range(nsaved):
            for c in range(N):
                y = np.atleast_1d(np.asarray(f(x[t, c]), dtype=np.float64)).ravel()
                if s is None:
                    s = np.zeros((N, y.size)); q = np.zeros((N, y.size))
                s[c] = s[c] + y
                q[c] = q[c] + y * y
    return s, q


def hist_slots(x, nbins: int, lo, hi) -> np.ndarray:
    """The slot of every value of x (..., D) among the nbins + 2 of its dimension — the index formula of klara_gather_histogram, operation for operation:
    inv_w = nbins / (hi - lo); 0 if x < lo; nbins + 1 if not x < hi (x >= hi, +inf, NaN); else 1 + min(nbins - 1, floor((x - lo) * inv_w)) — a subtraction
    followed by a multiplication, nothing that could fuse."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[-1]
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).ravel(), (D,)); hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).ravel(), (D,))
    inv_w = float(nbins) / (hi - lo)
    with np.errstate(all="ignore"):
        f = np.floor((x - lo) * inv_w)
        inner = 1 + np.fmin(float(nbins - 1), f)                 # (the minimum in double before the conversion, as the device takes it)
    under, over = x < lo, ~(x < hi)
    inner = np.where(under | over, 0.0, inner)                   # (the outer slots are decided first, as on the device: nothing of those values is converted)
    slot = np.where(under, 0, np.where(over, nbins + 1, inner.astype(np.int64)))
    return slot.astype(np.int64)


def pooled_hist(values, nbins: int, lo, hi) -> np.ndarray:
    """counts (D, nbins + 2) uint64 of `values` (..., D) — any leading axes: saved steps, chains — per dimension over everything else: the literal NumPy
    form of what a job with marginals= counts on the device (klara_gather_histogram).  Column 0 is the underflow, column nbins + 1 the overflow."""
    x = np.asarray(values, dtype=np.float64)
    D = x.shape[-1]
    slot = hist_slots(x, nbins, lo, hi).reshape(-1, D)
    counts = np.zeros((D, nbins + 2), dtype=np.uint64)
    for d in range(D):
        counts[d] = np.bincount(slot[:, d], minlength=nbins + 2).astype(np.uint64)
    return counts


def hist_quantiles(counts, nbins: int, lo, hi, probs) -> np.ndarray:
    """(D, len(probs)) quantiles from (D, nbins + 2) counts — klara_histogram_quantiles restated operation for operation: n = the row's total,
    w = (hi - lo) / nbins, k = max(1, ceil(p n)), b = the first slot whose cumulative count reaches k; slot 0: -inf, slot nbins + 1: +inf, otherwise
    (lo + (b - 1) w) + w (k - cum_before) / count_b; NaN for n = 0."""
    counts = np.asarray(counts, dtype=np.uint64)
    D = counts.shape[0]
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64).ravel(), (D,)); hi = np.broadcast_to(np.asarray(hi, dtype=np.float64).ravel(), (D,))
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64)).ravel()
    if np.any(~((probs > 0.0) & (probs <= 1.0))):
        raise ValueError("probabilities must lie in (0, 1]")
    out = np.empty((D, probs.size))
    for d in range(D):
        c = [int(v) for v in counts[d]]
        n = sum(c)
        w = np.float64(hi[d] - lo[d]) / np.float64(nbins)
        for j, p in enumerate(probs):
            if n == 0:
                out[d, j] = np.nan
                continue
            k = min(max(1, int(np.ceil(np.float64(p) * np.float64(n)))), n)
            cum, b = 0, 0
            while cum + c[b] < k:
                cum += c[b]; b += 1
            if b == 0:
                out[d, j] = -np.inf
            elif b == nbins + 1:
                out[d, j] = np.inf
            else:
                left = np.float64(lo[d]) + np.float64(b - 1) * w
                out[d, j] = left + w * np.float64(k - cum) / np.float64(c[b])
    return out


def rhat(values, split: bool = False) -> np.ndarray:
    """The Gelman–Rubin potential scale reduction factor per dimension: `values` is (m chains, n samples, D).  With W the mean of the chains' sample
    variances and B / n the sample variance of the chain means, R-hat = sqrt(((n - 1) / n W + B / n) / W) (Gelman & Rubin 1992).  split=True cuts every
    chain into the halves [0, h) and [n - h, n), h = n // 2 (an odd n drops the middle sample), and takes them as 2 m chains of h samples (BDA3 section
    11.4).  NaN for fewer than 2 chains or 2 samples per chain; plain IEEE division otherwise.  The literal NumPy form of klara_gather_rhat."""
    x = np.asarray(values, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if split:
        h = x.shape[1] // 2
        x = np.stack([x[:, :h], x[:, x.shape[1] - h:]], axis=1).reshape(2 * x.shape[0], h, x.shape[2])
    m, n, D = x.shape
    if m < 2 or n < 2:
        return np.full(D, np.nan)
    mu = x.mean(axis=1)                                          # (m, D)
    W = ((x - mu[:, None, :]) ** 2).sum(axis=1).sum(axis=0) / (m * (n - 1))
    Bn = ((mu - mu.mean(axis=0)) ** 2).sum(axis=0) / (m - 1)
    with np.errstate(all="ignore"):
        return np.sqrt(((n - 1) / n * W + Bn) / W)


def ess_from_sums(csum, wsum, bsum, m, n):
    """The pooled effective sample size from the across-unit sums, operation for operation as klara_gather_ess's host step evaluates it: csum (D, L + 1)
    = sum over the m units of their lagged sums c_j(k), wsum = csum[:, 0], bsum = sum (unit mean - mean)^2, n samples per unit.  Returns (ess[D], tau[D],
    rho[D, L + 1], pairs[D]): rho[0] = 1, Geyer's pair sum with pair 0 always summed, the stop at the first later pair <= 0, the monotone clamp; nothing
    capped; n < 4: NaN for ess, tau and rho[1:]."""
    csum = np.atleast_2d(np.asarray(csum, dtype=np.float64)); wsum = np.asarray(wsum, dtype=np.float64).ravel(); bsum = np.asarray(bsum, dtype=np.float64).ravel()
    D, R = csum.shape
    lags = R - 1
    dm, dn = float(m), float(n)
    rho = np.full((D, R), np.nan); rho[:, 0] = 1.0
    ess = np.full(D, np.nan); tau = np.full(D, np.nan); pairs = np.zeros(D, dtype=np.int32)
    if n < 4 or lags < 1:
        return ess, tau, rho, pairs
    with np.errstate(all="ignore"):
        W = wsum / (dm * (dn - 1.0))
        varp = ((dn - 1.0) / dn) * W + (bsum / (dm - 1.0) if m > 1 else 0.0)
        rho[:, 1:] = 1.0 - (W[:, None] - csum[:, 1:] / (dm * dn)) / varp[:, None]
        kk = (lags - 1) // 2
        for j in range(D):
            total = prev = 0.0
            for p in range(kk + 1):
                P = float(rho[j, 2 * p]) + float(rho[j, 2 * p + 1])
                if p >= 1 and P <= 0.0:
                    break
                Pm = prev if (p >= 1 and P > prev) else P
                total = total + Pm; prev = Pm; pairs[j] += 1
            tau[j] = -1.0 + 2.0 * total
        ess = (dm * dn) / tau
    return ess, tau, rho, pairs


def pooled_ess(hist, maxlag, split: bool = False) -> dict:
    """The pooled (multi-chain) effective sample size per dimension of `hist` (n saved steps, m chains, D) — the literal NumPy form of klara_gather_ess
    (BDA3 section 11.5; Vehtari et al. 2021), two-pass: with mu_j the mean of unit j (a chain; split=True: the half-chains [0, h) and [n - h, n),
    h = n // 2, as rhat's split form) and c_j(k) = sum_(t >= k) (x_jt - mu_j)(x_j,t-k - mu_j) for k = 0 .. L = min(maxlag, n - 1),
      csum[k] = sum_j c_j(k), wsum = csum[0], mean = mean of the mu_j, bsum = sum (mu_j - mean)^2, W = wsum / (m (n - 1)),
      var+ = (n - 1) / n W + bsum / (m - 1) (0 between term for m = 1), rho[0] = 1, rho[k] = 1 - (W - csum[k] / (m n)) / var+,
    then ess_from_sums.  Returns a dict as Engine.pooled_ess: ess, tau, rho, mean, wsum, bsum, csum, pairs, window_exhausted, nunits, nper, lags."""
    x = np.asarray(hist, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    if split:
        h = x.shape[0] // 2
        x = np.stack([x[:h], x[x.shape[0] - h:]], axis=2).reshape(h, 2 * x.shape[1], x.shape[2])       # unit 2 c + half
    n, m, D = x.shape
    lags = max(min(int(maxlag), n - 1), 0)
    mu = np.mean(x, axis=0)                                       # (m, D)
    z = x - mu
    csum = np.stack([np.sum(np.sum(z[k:] * z[:n - k], axis=0), axis=0) for k in range(lags + 1)], axis=1)        # (D, L + 1)
    mean = np.mean(mu, axis=0)
    bsum = np.sum((mu - mean) ** 2, axis=0)
    wsum = csum[:, 0].copy()
    ess, tau, rho, pairs = ess_from_sums(csum, wsum, bsum, m, n)
    return {"ess": ess, "tau": tau, "rho": rho, "mean": mean, "wsum": wsum, "bsum": bsum, "csum": csum, "pairs": pairs,
            "window_exhausted": pairs == (max(lags - 1, 0) // 2 + 1), "nunits": m, "nper": n, "lags": lags}


def _per_dim(fn, value: np.ndarray, *args) -> np.ndarray:
    value = np.asarray(value)
    return np.array([fn(value[i, :], *args) for i in range(value.shape[0])])


def mcvar_chain(value, vtype="imse", *args):
    """mcvar(s::VariableNState{Multivariate}, Val{vtype}) for one chain's (D x n) value matrix."""
    return _per_dim(mcvar, value, vtype, *args)


def mcse_chain(value, vtype="imse", *args):
    return _per_dim(mcse, value, vtype, *args)


def ess_chain(value, vtype="imse", *args):
    return _per_dim(ess, value, vtype, *args)


def iact_chain(value, vtype="imse", *args):
    return _per_dim(iact, value, vtype, *args)


# ---- zero-variance control variates (stats/variance/zv.jl, Mira, Solgi & Imparato 2013): the literal restatement — cov, inv, multiply
def zv_nterms(npars: int, order: int) -> int:
    """Number of control variates: npars (lzv) or npars (npars + 3) / 2 (qzv, zv.jl:52)."""
    return npars if order == 1 else npars * (npars + 3) // 2


def zv_controls(chain: np.ndarray, grad: np.ndarray, order: int) -> np.ndarray:
    """The control variates of zv.jl for an (n x D) chain and gradient: z = -grad / 2 (order 1, zv.jl:24) or
    z_i | 2 z_i x_i - 1 | x_i z_j + x_j z_i for i < j, i outer and j inner (order 2, zv.jl:61-70)."""
    chain = np.asarray(chain, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    if order == 1:
        return -0.5 * grad
    nsamples, npars = chain.shape
    k = npars * (npars + 3) // 2
    qz = np.empty((nsamples, k))
    z = -grad / 2
    qz[:, :npars] = z
    qz[:, npars:2 * npars] = 2 * z * chain - 1
    l = 2 * npars
    for i in range(npars - 1):
        for j in range(i + 1, npars):
            qz[:, l] = chain[:, i] * z[:, j] + chain[:, j] * z[:, i]
            l += 1
    return qz


def _zv_matrix(chain: np.ndarray, f: np.ndarray):
    npars, k = chain.shape[1], f.shape[1]
    a = np.empty((k, npars))
    for i in range(npars):                                           # zv.jl:26-31, 72-77
        augmentedcov = np.atleast_2d(np.cov(np.column_stack([f, chain[:, i]]), rowvar=False))
        precision = np.linalg.inv(augmentedcov[:k, :k])
        sigma = augmentedcov[:k, k]
        a[:, i] = -precision @ sigma
    return chain + f @ a, a


def lzv(chain, grad):
    """lzv(chain, grad) of zv.jl:9-34: (chain + z a, a) with z = -grad / 2 and a[:, i] = -inv(cov(z)) cov(z, chain[:, i]).
    (n x D) matrices give an (n x D) series and a (D x D); vectors give the univariate method (a series and a scalar)."""
    chain = np.asarray(chain, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    if chain.ndim == 1:
        z = -0.5 * grad
        augmentedcov = np.cov(np.column_stack([z, chain]), rowvar=False)
        a = -augmentedcov[0, 1] / augmentedcov[0, 0]
        return chain + z * a, float(a)
    return _zv_matrix(chain, zv_controls(chain, grad, 1))


def qzv(chain, grad):
    """qzv(chain, grad) of zv.jl:42-80: the quadratic polynomial, K = D (D + 3) / 2 control variates; vectors give the univariate
    method (a series and a of length 2)."""
    chain = np.asarray(chain, dtype=np.float64)
    grad = np.asarray(grad, dtype=np.float64)
    if chain.ndim == 1:
        z = -0.5 * grad
        qz = np.column_stack([z, 2 * z * chain - 1])
        augmentedcov = np.cov(np.column_stack([qz, chain]), rowvar=False)
        a = -np.linalg.inv(augmentedcov[:2, :2]) @ augmentedcov[:2, 2]
        return chain + qz @ a, a
    return _zv_matrix(chain, zv_controls(chain, grad, 2))


def lzv_chain(value, gradlogtarget):
    """lzv(s::ParameterNState{Continuous, Multivariate}) (zv.jl:38) for one chain's (D x n) value and gradlogtarget matrices:
    (corrected series (n x D), a (D x D))."""
    return lzv(np.asarray(value).T, np.asarray(gradlogtarget).T)


def qzv_chain(value, gradlogtarget):
    """qzv(s::ParameterNState{Continuous, Multivariate}) (zv.jl:84): (corrected series (n x D), a (K x D))."""
    return qzv(np.asarray(value).T, np.asarray(gradlogtarget).T)


# ---------------------------------------------------------------- src/stats/metrics.jl
def softabs(H, a: float = 1000.0) -> np.ndarray:
    """softabs(hessian, a) of src/stats/metrics.jl:1-4, literally: `lambda, Q = eig(hessian); Q * diagm(lambda ./ tanh(a * lambda)) * Q'`.
    LAPACK's symmetric eigen-decomposition (what Julia's `eig` takes for a symmetric matrix) and libm's tanh; a zero eigenvalue gives 0 / 0 as
    in the reference.  The device form (klara.jl_amd/csrc/klara_softabs.h, klara_desc.smmala_softabs) is tested against this."""
    H = np.asarray(H, dtype=np.float64)
    lam, Q = np.linalg.eigh(H)
    return (Q * (lam / np.tanh(float(a) * lam))) @ Q.T
