"""References for the chain statistics kernels (klara_monitors.hip: k_chain_stats, k_acov_update*, k_acov_tail_far, k_acov_finalize).

  exact(v, maxlag, batchlen)      the estimators of stats/variance/mcvar.jl:5, 35-41, 75-105, 137-158 in exact integer arithmetic (every double is a
                                  dyadic rational: the series is scaled to integers, nothing is rounded before the final conversion), with the
                                  margins of the two discontinuous decisions (Geyer's stop, the monotone clamp)
  plain_f64(v, maxlag, batchlen)  the same in f64: two passes, centred, direct sums in sample order, no FFT — how well f64 can do
  stream_f64(v, W, splits)        NumPy mirror of the device's streaming recurrences in their order of operations (lag blocks of 32, head, tail,
                                  near copy, finalize); pivot=False is the form before the series were shifted by their first sample
and the synthetic series the GPU tests run (tests/test_gpu_chain_stats.py), so that the CPU suite can assert their decision margins.
CPU only.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

MARGIN_MIN = 1e-6          # a series whose exact decision margin is below this is ambiguous and may not be used
CAP = 1e-9                 # hard cap on the error of the centred estimators (imse / ipse in IACT units, iid relative): the worst-case bound
                           # n u x (pairs summed <= 128) x (1 + (pivot - mean)^2 / var <= ~30) at n <= 600 is about 2.5e-10


# ---------------------------------------------------------------- exact
def _scaled_ints(v):
    """(X, den): Python integers X_t = v_t * den with den a power of two (exact for every finite double)."""
    pairs = [float(x).as_integer_ratio() for x in np.asarray(v, dtype=np.float64).ravel()]
    den = max(d for _, d in pairs)
    return [p * (den // d) for p, d in pairs], den


_acov_cache: dict = {}


def _exact_crossproducts(v, upto):
    """(c, n, den): c[k] = sum_t z_t z_(t+k) with z_t = n X_t - sum X (integers) = n den (v_t - mean); autocov_k = c[k] / (n^3 den^2)."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    key = v.tobytes()
    ent = _acov_cache.get(key)
    if ent is None:
        X, den = _scaled_ints(v)
        n = len(X)
        tot = sum(X)
        z = np.array([n * x - tot for x in X], dtype=object)
        ent = _acov_cache[key] = {"z": z, "den": den, "c": []}
        if len(_acov_cache) > 4096:
            _acov_cache.pop(next(iter(_acov_cache)))
    z, c = ent["z"], ent["c"]
    n = len(z)
    for k in range(len(c), upto + 1):
        c.append(int(np.dot(z[: n - k], z[k:])) if k < n else 0)
    return c, n, ent["den"]


def exact(v, maxlag=None, batchlen=None):
    """Exact estimators of one series.  Returns a dict of floats (each the correctly rounded exact rational):
      iid, bm (NaN without two batches or batchlen None), imse, ipse, acv0_n (= autocov_0 / n: the IACT unit of the error metric),
      m (Geyer's stopping index), margin_stop = min_j |g_j| / acv0 over the pairs tested, margin_clamp = min |g_j - g'_(j-1)| / acv0 over the clamp
      comparisons (g' the clamped sequence; inf when there is none), constant (acv0 == 0: every margin is inf, the estimators are 0),
      ess_imse, ess_ipse, iact_imse, iact_ipse (n iid / mcvar, mcvar / iid: convergence/ess.jl:3, iact.jl:3; NaN for 0 / 0)."""
    v = np.asarray(v, dtype=np.float64).ravel()
    n = v.size
    assert n >= 2
    maxlag = n - 1 if maxlag is None or maxlag <= 0 else min(int(maxlag), n - 1)
    k = (maxlag - 1) // 2
    c, n, den = _exact_crossproducts(v, 2 * k + 1)
    unit = Fraction(1, n ** 3 * den ** 2)                  # autocov_k = c[k] * unit
    g = [c[2 * j] + c[2 * j + 1] for j in range(k + 1)]     # integers: Gamma_j / unit
    m = k + 1
    for j in range(k + 1):
        if g[j] <= 0:
            m = j
            break
    tested = g[: min(m + 1, k + 1)]
    gm = list(g[:m])
    clamp_gaps = []
    for j in range(1, m):
        clamp_gaps.append(abs(gm[j] - gm[j - 1]))
        if gm[j] > gm[j - 1]:
            gm[j] = gm[j - 1]
    imse = Fraction(-c[0] + 2 * sum(gm)) * unit / n
    ipse = Fraction(-c[0] + 2 * sum(g[:m])) * unit / n
    iid = Fraction(c[0], n * n * den * den) / (n - 1) / n   # var(v) / n,  sum (v - mean)^2 = c[0] / (n den)^2
    out = {"n": n, "maxlag": maxlag, "m": m, "constant": c[0] == 0, "iid": float(iid), "imse": float(imse), "ipse": float(ipse),
           "acv0_n": float(Fraction(c[0]) * unit / n)}
    if c[0] == 0:
        out["margin_stop"] = out["margin_clamp"] = math.inf
    else:
        out["margin_stop"] = float(Fraction(min(abs(x) for x in tested), c[0]))
        out["margin_clamp"] = float(Fraction(min(clamp_gaps), c[0])) if clamp_gaps else math.inf
    out["bm"] = math.nan
    if batchlen:
        nb = n // int(batchlen)
        if nb > 1:
            X, den2 = _scaled_ints(v)
            B = [sum(X[b * batchlen:(b + 1) * batchlen]) for b in range(nb)]
            tb = sum(B)
            ss = sum((nb * b - tb) ** 2 for b in B)          # sum (mean_b - mean of means)^2 = ss / (nb batchlen den)^2
            var = Fraction(ss, (nb * batchlen * den2) ** 2) / (nb - 1)
            out["bm"] = float(batchlen * var / (nb * batchlen))
    for t, val in (("imse", imse), ("ipse", ipse)):
        out["ess_" + t] = float(n * iid / val) if val != 0 else (math.nan if iid == 0 else math.inf)
        out["iact_" + t] = float(val / iid) if iid != 0 else (math.nan if val == 0 else math.inf)
    return out


def exact_many(V, maxlag=None, batchlen=None):
    """exact() of every column of V (n x nseries) as a dict of arrays."""
    V = np.asarray(V, dtype=np.float64)
    rows = [exact(V[:, i], maxlag, batchlen) for i in range(V.shape[1])]
    return {key: np.array([r[key] for r in rows]) for key in rows[0]}


def metric(dev, ex, key):
    """Error of the device's `key` against exact_many's result: imse / ipse in IACT units, |dev - exact| / (exact acv0 / n) — a relative error
    means nothing on an antithetic chain, whose estimate is near 0; iid / bm as plain relative errors."""
    dev = np.asarray(dev, dtype=np.float64).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(dev - ex[key]) / (ex["acv0_n"] if key in ("imse", "ipse") else np.abs(ex[key]))


# ---------------------------------------------------------------- plain f64
def _seqsum(a):
    return float(np.cumsum(a)[-1]) if len(a) else 0.0        # (cumsum adds in index order; np.sum adds pairwise)


def plain_f64(v, maxlag=None, batchlen=None):
    """iid, bm, imse, ipse in f64, two-pass and centred, direct sums in sample order."""
    v = np.asarray(v, dtype=np.float64).ravel()
    n = v.size
    maxlag = n - 1 if maxlag is None or maxlag <= 0 else min(int(maxlag), n - 1)
    k = (maxlag - 1) // 2
    z = v - _seqsum(v) / n
    acv = lambda lag: _seqsum(z[: n - lag] * z[lag:]) / n
    acv0 = acv(0)
    out = {"iid": acv0 * n / (n - 1) / n, "bm": math.nan}
    gs_m = gs_p = gprev = 0.0
    for j in range(k + 1):
        gj = (acv0 if j == 0 else acv(2 * j)) + acv(2 * j + 1)
        if gj <= 0.0:
            break
        gs_p += gj
        if j > 0 and gj > gprev:
            gj = gprev
        gs_m += gj
        gprev = gj
    out["imse"] = (-acv0 + 2.0 * gs_m) / n
    out["ipse"] = (-acv0 + 2.0 * gs_p) / n
    if batchlen:
        nb = n // int(batchlen)
        if nb > 1:
            b = np.array([_seqsum(v[i * batchlen:(i + 1) * batchlen]) / batchlen for i in range(nb)])
            d = b - _seqsum(b) / nb
            out["bm"] = batchlen * (_seqsum(d * d) / (nb - 1)) / (nb * batchlen)
    return out


def plain_many(V, maxlag=None, batchlen=None):
    V = np.asarray(V, dtype=np.float64)
    rows = [plain_f64(V[:, i], maxlag, batchlen) for i in range(V.shape[1])]
    return {key: np.array([r[key] for r in rows]) for key in rows[0]}


# ---------------------------------------------------------------- mirror of the streaming recurrences
def stream_f64(v, W, splits, pivot=True):
    """(imse, ipse) of every column of v (n x nseries, or one series) from the device's streaming recurrences, launch by launch over `splits`
    (saved samples per launch, summing to n), in the device's order of operations (klara_monitors.hip launch_acov_update / k_acov_finalize):
    lag blocks b >= 1 first (they read the tail as the earlier launches left it), the copy of tail[0..31], the lag-0 pass, the far tail, and
    at the end the finalize step.  pivot=True: cross-products, total and tail of x - pivot with pivot = the series' first sample and the
    head kept raw; pivot=False: of x itself — the form that loses (mean / sd)^2 digits."""
    v = np.asarray(v, dtype=np.float64)
    one = v.ndim == 1
    if one:
        v = v[:, None]
    n, ns = v.shape
    assert sum(splits) == n and 2 <= W <= 128
    S = np.zeros((W, ns)); head = np.zeros((W, ns)); tail = np.zeros((W, ns)); total = np.zeros(ns)
    n_before = col0 = 0
    WL = min(W, 32)
    for m in splits:
        if m == 0:
            continue
        piv = (v[col0].copy() if n_before == 0 else head[0].copy()) if pivot else np.zeros(ns)
        if W > 32:
            for b in range((W - 1) // 32, 0, -1):                       # k_acov_update_block
                k0 = 32 * b
                nr = min(32, W - k0)
                s = np.zeros((32, ns)); win = np.zeros((32, ns))
                s[:nr] = S[k0:k0 + nr]; win[:nr] = tail[k0:k0 + nr]
                for j in range(m):
                    x = v[col0 + j] - piv
                    y = v[col0 + j - k0] - piv if j >= k0 else tail[k0 - j - 1]
                    s[0] = s[0] + x * y
                    s[1:] = s[1:] + x * win[:-1]
                    win[1:] = win[:-1].copy()
                    win[0] = y
                S[k0:k0 + nr] = s[:nr]
            near = tail[:32].copy()
        s = np.zeros((32, ns)); win = np.zeros((32, ns))                # k_acov_update<8|16|32>
        s[:WL] = S[:WL]; win[:WL] = tail[:WL]
        tot = total.copy()
        for j in range(m):
            raw = v[col0 + j]
            x = raw - piv
            s[0] = s[0] + x * x
            s[1:] = s[1:] + x * win[:-1]
            if n_before + j < W:
                head[n_before + j] = raw
            win[1:] = win[:-1].copy()
            win[0] = x
            tot = tot + x
        S[:WL] = s[:WL]; tail[:WL] = win[:WL]; total = tot
        if W > 32:                                                      # k_acov_tail_far
            piv2 = head[0] if pivot else np.zeros(ns)
            for k in range(W - 1, 31, -1):
                if k < m:
                    val = v[col0 + m - 1 - k] - piv2
                elif k - m >= 32:
                    val = tail[k - m]
                else:
                    val = near[k - m]
                tail[k] = val
        n_before += m
        col0 += m
    # k_acov_finalize
    piv = head[0] if pivot else np.zeros(ns)
    mean = total / n
    maxlag = min(W - 1, n - 1)
    kk = (maxlag - 1) // 2
    imse = np.zeros(ns); ipse = np.zeros(ns)
    for i in range(ns):
        hs = ts = acv0 = gsum_m = gsum_p = gprev = 0.0
        tt, mn = float(total[i]), float(mean[i])
        for j in range(kk + 1):
            pair = 0.0
            for h2 in range(2):
                k = 2 * j + h2
                a = (S[k, i] - mn * ((tt - ts) + (tt - hs)) + float(n - k) * mn * mn) / n
                if k == 0:
                    acv0 = a
                pair += a
                hs += head[k, i] - piv[i]; ts += tail[k, i]
            if pair <= 0.0:
                break
            gsum_p += pair
            gm = pair
            if j > 0 and gm > gprev:
                gm = gprev
            gsum_m += gm; gprev = gm
        imse[i] = (-acv0 + 2.0 * gsum_m) / n
        ipse[i] = (-acv0 + 2.0 * gsum_p) / n
    return (imse[0], ipse[0]) if one else (imse, ipse)


# ---------------------------------------------------------------- the series of the GPU tests
GRID = 2.0 ** -10           # the synthetic series live on this dyadic grid: offsets up to 1.25e8 keep them exact in f64 (37 of 53 bits)
SD = 1.25                   # innovation scale of the synthetic series; the shift cases add offsets of `k * SD`
OFFSETS = (0.0, 90.0, 1e3, 1e4, 1e6, 1e8)
WINDOWS = (1, 2, 7, 8, 15, 16, 31, 32, 33, 63, 64, 95, 127)          # maxlag = W - 1: each template width, even / odd, one entry in a lag block, exact blocks
N_A = 200


def ar1_series(n, nseries, seed):
    """(n x nseries) on GRID: thirds AR(1) with coefficient 0.6, -0.6 and white noise, innovations N(0, SD^2)."""
    rng = np.random.default_rng(seed)
    e = SD * rng.standard_normal((n + 50, nseries))
    phi = np.array([(0.6, -0.6, 0.0)[(3 * i) // nseries] for i in range(nseries)])
    x = np.zeros((n + 50, nseries))
    for t in range(1, n + 50):
        x[t] = phi * x[t - 1] + e[t]
    return np.round(x[50:] / GRID) * GRID


def _fill(n, parts):
    out, i = [], 0
    while n > 0:
        out.append(min(parts[i % len(parts)], n)); n -= out[-1]; i += 1
    return out


def splits_a(n=N_A):
    """Launch splits of case (a): one launch; all ones; 31 / 33 straddling the block delay; 32s; a first launch shorter than the window
    (the head fills across launches: 3, then 1, then 40s); [5, 1, 64, 130]."""
    return {"one": [n], "ones": [1] * n, "31_33": _fill(n, [31, 33]), "32s": _fill(n, [32]), "short_first": [3, 1] + _fill(n - 4, [40]),
            "5_1_64_130": [5, 1, 64, n - 70]}


SEED_A, SEED_C = 20260927, 20260928


def series_a():
    return ar1_series(N_A, 24, SEED_A)


def series_b(n):
    return ar1_series(n, 24, SEED_A + 200 + n)


def series_c():
    return ar1_series(40, 300, SEED_C)


def constant_series(n=60):
    """(n x 4): c = 0.1, c = 1000.1, c = 2^20, and a series that changes once (1000.1 -> 1000.1 + 2^-10 after 17 samples)."""
    v = np.empty((n, 4))
    v[:, 0] = 0.1; v[:, 1] = 1000.1; v[:, 2] = 2.0 ** 20
    v[:, 3] = 1000.1; v[17:, 3] = 1000.1 + 2.0 ** -10
    return v


def constant_bound(c, n, maxlag):
    """|imse|, |ipse|, iid of a constant series c: a computed mean off by at most n u |c| gives deviations at most that large —
    (4 n u |c|)^2 (maxlag + 1) / n with u = 2^-53."""
    return (4.0 * n * 2.0 ** -53 * abs(c)) ** 2 * (maxlag + 1) / n


# ---------------------------------------------------------------- the jobs of the GPU tests (case f)
JOB_SIGMA = np.array([1.0, 0.5, 2.0, 1.25, 0.75])
JOB_MU = np.array([0.0, 90.0, 1e4, -1e6, 3.0]) * JOB_SIGMA
JOB_NCHAINS, JOB_NSTEPS, JOB_BURNIN, JOB_THIN = 7, 400, 25, 2


def job_x0():
    return JOB_MU + JOB_SIGMA * np.random.default_rng(11).standard_normal((JOB_NCHAINS, 5))


def job_cases():
    """name -> engine case (tests/cases.py form): the samplers on GaussDiagTarget.mvnormal(JOB_MU, JOB_SIGMA), hmc_rats, and an MH job whose
    proposals are all rejected (a constant off-centre chain through the real path)."""
    import klara_jl_amd as K
    from klara_jl_amd import _lib as L
    import cases
    tgt = K.GaussDiagTarget.mvnormal(JOB_MU, JOB_SIGMA)
    base = dict(target=tgt, nchains=JOB_NCHAINS, nsteps=JOB_NSTEPS, burnin=JOB_BURNIN, thinning=JOB_THIN, x0=job_x0())
    out = {
        "mh": dict(base, sampler=L.SAMPLER_MH, mh_sigma=JOB_SIGMA.copy()),
        "mala": dict(base, sampler=L.SAMPLER_MALA, driftstep=0.3),
        "hmc": dict(base, sampler=L.SAMPLER_HMC, leapstep=0.25, nleaps=3),
        # leapstep * nleaps = 2.7: 0.86 of a half period (pi sigma) at sigma = 1, past it at sigma = 0.75 — antithetic series in those dimensions
        "hmc_antithetic": dict(base, sampler=L.SAMPLER_HMC, leapstep=0.3, nleaps=9),
        "slice": dict(base, sampler=L.SAMPLER_SLICE, slice_widths=2.0 * JOB_SIGMA, slice_stepout=True),
        "mh_constant": dict(base, sampler=L.SAMPLER_MH, mh_sigma=np.full(5, 1e12)),
    }
    r = dict(cases.make_case("hmc_rats")); r.update(nsteps=JOB_NSTEPS, burnin=JOB_BURNIN, thinning=JOB_THIN, nchains=7, x0=r["x0"][:7])
    out["hmc_rats"] = r
    return out


# (case, acov_maxlag, steps_per_launch, with MON_HISTORY): both lag windows, both launch lengths, with and without a value history (without:
# the estimator's own 32-column ring wraps), every sampler; hmc_rats at maxlag 9
JOB_RUNS = [("mh", 12, 7, False), ("mh", 40, 50, True), ("mala", 40, 7, False), ("mala", 12, 50, True), ("hmc", 12, 50, False), ("hmc", 40, 7, True),
            ("hmc_antithetic", 40, 50, False), ("slice", 12, 7, False), ("slice", 40, 50, True), ("hmc_rats", 9, 7, False), ("mh_constant", 12, 7, False)]
JOB_BATCHLEN = 7


def oracle_history(case):
    """(nsaved x nchains*D) history of the job on the CPU oracle — the device's series bit for bit."""
    import cases
    import oracle_ffi as O
    job = O.OracleJob(**cases.oracle_kwargs(case), want_hist=True)
    job.set_state(case["x0"])
    assert job.run(case["nsteps"]) == 0
    return job.hist.reshape(job.hist.shape[0], -1).copy()


def bm_stream_bound(V, batchlen, ex):
    """Bound on |streaming bm - exact bm| per column of V (klara_get_chain_bm: batch means from the transition kernels' running sums).
    u = 2^-53, M = max |x|, ns = nb batchlen samples, L = batchlen.
      running sum at a batch boundary: at most ns + 1 terms held * x (one rounding each, u held |x|) added one after the other (klara_kernels.h
        fold_state: sum + hf * x; the read-back view adds the held state once more), every addition rounding a partial sum of at most (ns + 1) M:
        |error| <= E = u M (ns + 1)(ns + 2)                                              (recursive summation, first order in u)
      batch mean b = (s - prev) / L: two sums in error, the difference and the quotient rounded: |error| <= 2 E / L + 2 u M
      Welford's running mean of the b's is rounded once per batch (u M each, nb of them), which shifts a deviation by at most nb u M:
        delta = 2 E / L + (2 + nb) u M per deviation
      M2 = sum (b - mean b)^2 with every b off by at most delta: |dM2| <= 2 sqrt(M2 nb) delta + nb delta^2  (Cauchy-Schwarz; centring does
        not enlarge the perturbation's norm), and 8 nb u M2 for the roundings of the M2 recurrence itself
      bm = M2 / ((nb - 1) nb)."""
    V = np.asarray(V, dtype=np.float64)
    n = V.shape[0]
    nb = n // batchlen
    ns = nb * batchlen
    u = 2.0 ** -53
    M = np.abs(V).max(axis=0)
    E = u * M * (ns + 1) * (ns + 2)
    delta = 2.0 * E / batchlen + (2 + nb) * u * M
    M2 = ex["bm"] * (nb - 1) * nb
    return (2.0 * np.sqrt(M2 * nb) * delta + nb * delta ** 2 + 8 * nb * u * M2) / ((nb - 1) * nb)


# Asserted tolerances of the centred estimators per case class (same metric as CAP): 4 x the larger of plain_f64's and the device's worst error
# against exact on the class's series, rounded up to a power of two — the measured values are in profiles/chain_stats_accuracy.txt.
TOL = {
    "selftest": 2.0 ** -45,       # classes a-c: plain_f64 4.11e-15, device 4.11e-15
    "shift": 2.0 ** -45,          # classes d-e: plain_f64 4.11e-15 (on the unshifted series: on the shifted ones fl(mean) costs it up to 7.7e-9), device 6.15e-15
    "jobs": 2.0 ** -44,           # class f, post-hoc / iid / bm: plain_f64 1.06e-14 (series minus their first sample; 1.6e-9 as they are), device 1.12e-14
    "jobs_stream": 2.0 ** -39,    # class f, streaming: device 3.77e-13 — 36 x plain_f64, because the streamed sums are centred on the pivot, not on the mean:
                                  # the finalize step's cancellation costs (pivot - mean)^2 / var digits (inside CAP's worst-case bound)
}
