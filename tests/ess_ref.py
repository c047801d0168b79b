"""References for the pooled (multi-chain) effective sample size (klara_ess.hip: k_ess_stage1 / k_ess_stage2 over a streamed autocovariance state,
R-hat's unit reduction for mean / bsum / wsum; klara_comm.hip: ess_finish and the between-rank merge with the lagged sums in MergeLayout's X slot, behind
klara_gather_ess and klara_selftest_ess).  A "unit" is a chain, or for the split form a half-chain (unit 2 c + half); m units of n samples each.

  exact(hist, maxlag, split)                 csum, wsum, mean, bsum, rho, pairs, tau, ess of chosen columns in exact rational arithmetic, with the margins of
                                             the two discontinuous decisions (Geyer's stop, the monotone clamp)
  stream_state(v, W, splits)                 the streamed state (S, head, tail, total) after the device's update recurrences, launch by launch — the update
                                             part of chain_stats_ref.stream_f64, which keeps its state to itself
  mirror(hist, maxlag, split, splits)        NumPy restatement of the device's order of operations (klara_ess.h), one handle
  mirror_ranks(bounds, hist, ...)            mirror's sums of every shard, the between-rank merge with the all-reduces as ascending sums from zero, finish()
  bound(ex, ranks)                           derived worst-case bounds on csum, wsum, bsum, rho, tau and ess against exact (see its docstring)
and the shapes and inputs the CPU and GPU tests share.  CPU only.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import chain_stats_ref as R
import pooled_ref as P
import rhat_ref as H

U = P.U
GRID, SD, MARGIN_MIN = R.GRID, R.SD, R.MARGIN_MIN
# The cap on every relative bound an input may have.  pooled_ref.CAP (1e-7), not chain_stats_ref.CAP (1e-9): the lagged sums themselves are bounded near
# 1e-13 (they are sums of z = x - first sample, which the offset never enters), but bsum enters var+ and hence every rho, and its bound is R-hat's: at an
# offset of 1e6 sd the units' means carry u * 1.25e6 = 1.4e-10 against a between-unit sd of a few tenths — 1e-8 after the merges, exactly the situation
# pooled_ref.CAP was set for.  A pair is off by at most 2 e_rho + 4 u <= 3 CAP, well below the decision margins: no decision can flip.
CAP = P.CAP
assert 4 * CAP < MARGIN_MIN
OFFSETS = (0.0, 1e4, 1e6)
ESS_BLOCKS, THREADS = 512, 256         # KLARA_ESS_BLOCKS; the workgroup size


# ---------------------------------------------------------------- inputs
def make_hist(N, D, ncols, offset=0.0, seed=0):
    """A value history (ncols, N, D) — column t at hist[t], as the device keeps it — on chain_stats_ref's dyadic grid: AR(1)-like series (thirds with
    coefficient 0.6, -0.6 and white noise: chain_stats_ref.ar1_series) around offset * SD plus a chain-specific shift of about SD / 2 (so that the
    between-unit variance is not only sampling noise); chains c % 9 == 4 never move (every c_j(k) is exactly 0) unless that would leave no moving chain."""
    base = float(offset) * SD
    assert base / GRID == round(base / GRID) and ncols >= 2
    rng = np.random.default_rng([20261101, seed, N, D, ncols])
    x = R.ar1_series(ncols, N * D, int(rng.integers(1 << 30))).reshape(ncols, N, D)
    shift = np.rint(0.5 * SD * rng.standard_normal((N, D)) / GRID) * GRID
    x = base + (x + shift)
    c = np.arange(N)
    still = (c % 9 == 4) & (N > 5)
    x[:, still] = x[0, still]
    return np.ascontiguousarray(x)


def units_of(hist, split):
    """(n, m, D) view with the units along axis 1: the chains, or the half-chains [0, h) and [ncols - h, ncols) as unit 2 c + half"""
    if not split:
        return hist
    ncols, N, D = hist.shape
    h = ncols // 2
    return np.stack([hist[:h], hist[ncols - h:]], axis=2).reshape(h, 2 * N, D)


# ---------------------------------------------------------------- exact
def exact(hist, maxlag, split=False, cols=None):
    """Exact quantities per column of `cols`, each the correctly rounded rational: csum (len(cols), L + 1), wsum, mean, bsum, rho, tau, ess, pairs, and
    margin_stop = min |P_j| over the pairs the stop tested (j >= 1; inf when there is none), margin_clamp = min |P_j - P'_(j-1)| over the clamp's comparisons
    — both in units of rho, that is relative to var+.  Also what bound() needs: m, n, L, sumQ = sum over the units of sum_t (x - first sample)^2,
    max_abs_mean, spread and sigma_b of the units' means, varp, W.  var+ = 0: rho[1:], tau and ess NaN, pairs as the device's NaN arithmetic leaves it
    (every comparison false: all kk + 1 pairs)."""
    x = units_of(hist, split)
    n, m, D = x.shape
    cols = list(range(D)) if cols is None else list(cols)
    L = min(int(maxlag), n - 1)
    kk = (L - 1) // 2 if L >= 1 else -1
    k = x[:, :, cols] / GRID
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2.0 ** 40
    X = k.astype(np.int64)
    s = X.sum(axis=0)                                                        # (m, cols)
    z = n * X - s                                                            # n den (x - mu_u): integers
    assert n * float(np.abs(z).max()) ** 2 < 2.0 ** 62
    den = int(round(1 / GRID))
    unit = Fraction(1, n * n * den * den)                                    # c_u(k) = (sum_t z_t z_(t-k)) * unit
    nc = len(cols)
    out = {key: np.full(nc, np.nan) for key in ("wsum", "mean", "bsum", "tau", "ess", "margin_stop", "margin_clamp", "sumQ", "max_abs_mean", "spread",
                                                "sigma_b", "varp", "W")}
    out["csum"] = np.zeros((nc, L + 1)); out["rho"] = np.full((nc, L + 1), np.nan); out["pairs"] = np.zeros(nc, dtype=np.int64)
    out["wsum_zero"] = np.zeros(nc, dtype=bool); out["bsum_zero"] = np.zeros(nc, dtype=bool)
    zf = (x[:, :, cols] - x[0][None, :, cols])
    out["sumQ"] = (zf * zf).sum(axis=(0, 1))
    out["max_abs"] = np.abs(x[:, :, cols]).max(axis=(0, 1))
    for i in range(nc):
        C = [int(np.sum((z[lag:, :, i] * z[:n - lag, :, i]).sum(axis=0).astype(object))) for lag in range(L + 1)]
        csum = [c * unit for c in C]
        si = [int(a) for a in s[:, i]]
        tot = sum(si); ss = sum(a * a for a in si)
        mean = Fraction(tot, den * n * m)
        bsum = Fraction(ss * m - tot * tot, m * den * den * n * n)
        wsum = csum[0]
        out["csum"][i] = [float(c) for c in csum]
        out["wsum"][i] = float(wsum); out["mean"][i] = float(mean); out["bsum"][i] = float(bsum)
        out["wsum_zero"][i] = wsum == 0; out["bsum_zero"][i] = bsum == 0
        mu = np.array([a / (den * n) for a in si])
        out["max_abs_mean"][i] = np.abs(mu).max(); out["spread"][i] = mu.max() - mu.min(); out["sigma_b"][i] = math.sqrt(float(bsum) / m)
        out["rho"][i, 0] = 1.0
        out["margin_stop"][i] = out["margin_clamp"][i] = math.inf
        if n < 4 or L < 1:
            continue
        W = wsum / (m * (n - 1))
        varp = Fraction(n - 1, n) * W + (bsum / (m - 1) if m > 1 else 0)
        out["varp"][i] = float(varp); out["W"][i] = float(W)
        if varp == 0:
            out["pairs"][i] = kk + 1
            continue
        rho = [Fraction(1)] + [1 - (W - csum[lag] / (m * n)) / varp for lag in range(1, L + 1)]
        out["rho"][i] = [float(r) for r in rho]
        total = Fraction(0); prev = None; pairs = 0
        stop_m, clamp_m = [], []
        for j in range(kk + 1):
            Pj = rho[2 * j] + rho[2 * j + 1]
            if j >= 1:
                stop_m.append(abs(Pj))
                if Pj <= 0:
                    break
                clamp_m.append(abs(Pj - prev))
                if Pj > prev:
                    Pj = prev
            total += Pj; prev = Pj; pairs += 1
        tau = -1 + 2 * total
        out["pairs"][i] = pairs
        out["tau"][i] = float(tau)
        out["ess"][i] = float(m * n / tau) if tau != 0 else math.nan
        if stop_m:
            out["margin_stop"][i] = float(min(stop_m))
        if clamp_m:
            out["margin_clamp"][i] = float(min(clamp_m))
    out["m"], out["n"], out["L"], out["cols"], out["split"], out["D"] = m, n, L, cols, bool(split), D
    return out


# ---------------------------------------------------------------- mirror
def stream_state(v, W, splits):
    """(S, head, tail, total) of every column of v (n x ns) after launch_acov_update over the launches `splits` (klara_monitors.hip) — the update loop of
    chain_stats_ref.stream_f64 (pivot form), operation for operation; tests/test_ess_host.py holds the two together through k_acov_finalize's estimators."""
    v = np.asarray(v, dtype=np.float64)
    n, ns = v.shape
    assert sum(splits) == n and 1 <= W <= 128
    S = np.zeros((W, ns)); head = np.zeros((W, ns)); tail = np.zeros((W, ns)); total = np.zeros(ns)
    n_before = col0 = 0
    WL = min(W, 32)
    for m in splits:
        if m == 0:
            continue
        piv = v[col0].copy() if n_before == 0 else head[0].copy()
        if W > 32:
            for b in range((W - 1) // 32, 0, -1):                           # k_acov_update_block
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
        s = np.zeros((32, ns)); win = np.zeros((32, ns))                    # k_acov_update<8|16|32>
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
        if W > 32:                                                          # k_acov_tail_far
            piv2 = head[0]
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
    return S, head, tail, total


def unit_lagged_sums(state, n, L):
    """(c[L + 1, ns], mu[ns]) of every series of a streamed state as k_ess_stage1 forms them (klara_ess.h): k ascending, hs / ts carried"""
    S, head, tail, total = state
    tot = total; mean = tot / float(n); piv = head[0]
    hs = np.zeros_like(tot); ts = np.zeros_like(tot)
    c = np.zeros((L + 1, tot.size))
    for k in range(L + 1):
        c[k] = (S[k] - mean * ((tot - ts) + (tot - hs))) + (float(n - k) * mean) * mean
        hs = hs + (head[k] - piv)
        ts = ts + tail[k]
    return c, piv + mean


def lanes(E, D):
    nb = max(min(-(-E // THREADS), ESS_BLOCKS), -(-D // THREADS))
    return D * ((THREADS * nb) // D)


def sum_units(c, D):
    """csum (D, L + 1) from c (L + 1, E), unit-series e = u D + j: stage 1's lanes, then stage 2 (klara_ess.h)"""
    R1, E = c.shape
    V = lanes(E, D)
    acc = np.zeros((R1, V))
    for r in range(-(-E // V)):
        a = min(V, E - r * V)
        acc[:, :a] = acc[:, :a] + c[:, r * V:r * V + a]
    out = np.zeros((R1, D))
    if D > THREADS:
        for q in range(V // D):
            out = out + acc[:, q * D:(q + 1) * D]
        return np.ascontiguousarray(out.T)
    V2 = D * (THREADS // D)
    lane = np.zeros((R1, V2))
    for r in range(-(-V // V2)):
        a = min(V2, V - r * V2)
        lane[:, :a] = lane[:, :a] + acc[:, r * V2:r * V2 + a]
    for q in range(V2 // D):
        out = out + lane[:, q * D:(q + 1) * D]
    return np.ascontiguousarray(out.T)


def sum_depth(E, D):
    """additions on the longest path of sum_units"""
    V = lanes(E, D)
    if D > THREADS:
        return -(-E // V) + V // D
    V2 = D * (THREADS // D)
    return -(-E // V) + -(-V // V2) + V2 // D


def finish(csum, wsum, bsum, m, n):
    """ess_finish of klara_comm.hip per dimension, scalar by scalar: (ess, tau, rho, pairs)"""
    D, R1 = csum.shape
    L = R1 - 1
    dm, dn = float(m), float(n)
    ess = np.full(D, np.nan); tau = np.full(D, np.nan); rho = np.full((D, R1), np.nan); pairs = np.zeros(D, dtype=np.int32)
    rho[:, 0] = 1.0
    if n < 4 or L < 1:
        return ess, tau, rho, pairs
    kk = (L - 1) // 2
    with np.errstate(all="ignore"):
        for j in range(D):
            ws, bs = np.float64(wsum[j]), np.float64(bsum[j])
            Wv = ws / np.float64(dm * (dn - 1.0))
            varp = np.float64((dn - 1.0) / dn) * Wv + (bs / np.float64(dm - 1.0) if m > 1 else np.float64(0.0))
            for k in range(1, R1):
                rho[j, k] = 1.0 - (Wv - csum[j, k] / np.float64(dm * dn)) / varp
            total = np.float64(0.0); prev = np.float64(0.0); np_ = 0
            for p in range(kk + 1):
                Pp = rho[j, 2 * p] + rho[j, 2 * p + 1]
                if p >= 1 and Pp <= 0.0:
                    break
                Pm = prev if (p >= 1 and Pp > prev) else Pp
                total = total + Pm; prev = Pm; np_ += 1
            tau[j] = -1.0 + 2.0 * total
            ess[j] = np.float64(dm * dn) / tau[j]
            pairs[j] = np_
    return ess, tau, rho, pairs


def local_sums(hist, maxlag, split=False, splits=None):
    """what one handle stages: dict of mean, bsum, wsum, csum (D, L + 1), m, n, L.  splits: the launches of the streamed path (None: one launch; the
    streamed sums do not depend on it — test_ess_host asserts that on the mirror, test_gpu_ess on the device)"""
    ncols, N, D = hist.shape
    W = int(maxlag) + 1
    if split:
        h = ncols // 2
        n = h
        parts = [hist[:h], hist[ncols - h:]]
    else:
        n = ncols
        parts = [hist]
    L = min(int(maxlag), n - 1)
    cs, mus = [], []
    for part in parts:
        sp = list(splits) if (splits is not None and not split) else [part.shape[0]]
        c, mu = unit_lagged_sums(stream_state(part.reshape(part.shape[0], N * D), W, sp), n, L)
        cs.append(c.reshape(L + 1, N, D)); mus.append(mu.reshape(N, D))
    per = len(parts)
    c = np.stack(cs, axis=2).reshape(L + 1, per * N * D)                    # unit 2 c + half
    mu = np.stack(mus, axis=1).reshape(per * N, D)
    csum = sum_units(c, D)
    mean, bsum, wsum = H.reduce_units(mu, c[0].reshape(per * N, D))
    return {"mean": mean, "bsum": bsum, "wsum": wsum, "csum": csum, "m": per * N, "n": n, "L": L}


def _result(mean, bsum, wsum, csum, m, n, L):
    ess, tau, rho, pairs = finish(csum, wsum, bsum, m, n)
    return {"ess": ess, "tau": tau, "rho": rho, "mean": mean, "wsum": wsum, "bsum": bsum, "csum": csum, "pairs": pairs, "nunits": int(m), "nper": int(n),
            "lags": int(L)}


def mirror(hist, maxlag, split=False, splits=None):
    """klara_gather_ess without a communicator: dict as Engine.pooled_ess returns it, and csum"""
    s = local_sums(hist, maxlag, split, splits)
    return _result(s["mean"], s["bsum"], s["wsum"], s["csum"], s["m"], s["n"], s["L"])


def merge_ranks(parts):
    """The between-rank merge from every rank's local_sums: (m_r, mean_r, bsum_r) as pooled_ref.between_ranks merges (n_r, mean_r, M2_r); wsum and csum
    ascending sums from 0.0; the same n and L on every rank"""
    n, L = parts[0]["n"], parts[0]["L"]
    assert all(p["n"] == n and p["L"] == L for p in parts)
    mean, bsum, m = P.between_ranks([p["mean"] for p in parts], [p["bsum"] for p in parts], [p["m"] for p in parts])
    wsum = np.zeros_like(mean); csum = np.zeros_like(parts[0]["csum"])
    for p in parts:
        wsum = wsum + p["wsum"]; csum = csum + p["csum"]
    return _result(mean, bsum, wsum, csum, m, n, L)


def mirror_ranks(bounds, hist, maxlag, split=False, splits=None):
    return merge_ranks([local_sums(np.ascontiguousarray(hist[:, c0:c1]), maxlag, split, splits) for c0, c1 in zip(bounds[:-1], bounds[1:])])


# ---------------------------------------------------------------- bound
def bound(ex, ranks=1, plain=False):
    """dict of worst-case bounds per column of exact()'s result, for the device's order of operations (`ranks` > 1: cut into that many shards and merged):
    rel_c (|csum[k] - exact| / exact wsum, every lag), rel_w, rel_b (relative, NaN where the exact value is 0), abs_rho (every lag), abs_tau, rel_ess.
    First order in u = 2^-53, doubled for the rest.

    Notation: m units of n samples, E = m D unit-series, pivot = a unit's first sample, z = x - pivot, Q_u = sum_t z_t^2 = c_u(0) (1 + ((pivot - mu_u) /
    sd_u)^2) with sd_u^2 = c_u(0) / n, sumQ = sum_u Q_u, depth = sum_depth(E, D), R = ranks.
      the streamed sums are exact: on the dyadic grid (multiples of 2^-10 below 2^41 of them) z, z z', S_k, total, hs and ts are integers far below 2^53 in
        units of 2^-10 or 2^-20 (tests/test_ess_host.py checks this on the mirror against exact integer sums).
      per unit-series and lag: with mu = total / n exactly and the computed mean = mu (1 + d), |d| <= u, and A = (total - ts) + (total - hs) exact,
        c = fl(fl(S - fl(mean A)) + fl(fl((n - k) mean) mean)) against S - mu A + (n - k) mu^2:  u |mu A| for d, u |mu A| for the product, u (|S| + |mu A|)
        for the difference, 4 u (n - k) mu^2 for the square term (2 u from d, 2 u from its products), u (|S| + |mu A| + (n - k) mu^2) for the last sum.
        By Cauchy–Schwarz |S_k| <= Q, |mu| <= sqrt(Q / n), |A| <= 2 sqrt(n Q), (n - k) mu^2 <= Q:  e_c <= u (2 + 4 * 2 + 5) Q = 15 u Q <= 16 u Q.
      csum[k]: |c_u(k)| <= c_u(0), so a sum along `depth` additions adds depth u wsum, the sum over the ranks R u wsum:
            rel_c = 16 u sumQ / wsum + (depth + R) u                 (R = 0 for one handle)
      wsum is the sum of the same c_u(0) through R-hat's reduction, pooled_ref.merge_depth(m) additions deep:  rel_w = 16 u sumQ / wsum + (merge_depth + R) u.
      bsum: the units' means are fl(pivot + fl(total / n)), off by 2 u M — the split form's e_mu of rhat_ref.bound, whose rel_b is taken as it stands
        (the same reduction and the same between-rank merge).
      rho[k] = 1 - (W - csum[k] / (m n)) / var+:  W = wsum / (m (n - 1)) carries rel_W = rel_w + 2 u; csum[k] / (m n) an absolute (rel_c + 2 u) wsum / (m n)
        <= (rel_c + 2 u) W; the numerator num, |num| <= 2 W, so e_num <= (rel_W + rel_c + 2 u + 2 u) W; var+ is a sum of two non-negative terms:
        rel_v <= max(rel_W, rel_b) + 4 u.  The quotient is off by e_num / var+ + |num| / var+ (rel_v + u) and, W / var+ <= n / (n - 1) <= 4 / 3,
            abs_rho = (4 / 3) (rel_W + rel_c + 4 u + 2 (rel_v + u)) + 4 u    (the last for the subtraction from 1; |rho| <= 4)
      tau = -1 + 2 sum P'_j over `pairs` pairs, each P' some P_i = rho + rho':  e_P = 2 abs_rho + 4 u (|P| <= 2 ... 8 u at most for |P| <= 8), and with the
        decisions the same — admissible() demands margins >= MARGIN_MIN > 4 CAP >= e_P —
            abs_tau = 2 pairs (e_P + u |tau + 1|) + 2 u |tau|,   rel_ess = abs_tau / |tau| + 2 u.
    All doubled for the second order.

    plain=True: the bounds of klara_jl_amd.stats.pooled_ess instead — two passes, centred on np.mean, nothing shifted by a pivot, so the offset enters:
      mu_hat = mu + d with |d| <= e_mu = (log2 n + 2) u max |x| (pairwise summation), z_hat = fl(x - mu_hat) = (z - d)(1 + e).  Then sum z_hat z_hat' -
      sum z z' = -d (sum_(t >= k) z + sum_(t < n - k) z) + (n - k) d^2 + roundings; the two edge sums are at most sqrt(n c_u(0)) each (the whole sum of z
      is 0), so over the units, by Cauchy–Schwarz, with sd^2 = wsum / (m n):
            rel_c = rel_w = 2 e_mu / sd + (e_mu / sd)^2 + (log2(m n) + 6) u,
      and for bsum = sum (mu_hat_u - mean_hat)^2, every difference off by 2 e_mu:  rel_b = 4 e_mu / sigma_b + (2 e_mu / sigma_b)^2 + (log2 m + 6) u.
      rho, tau and ess follow from these as above."""
    m, n, D = ex["m"], ex["n"], ex["D"]
    depth = sum_depth(m * D, D)
    Rk = ranks if ranks > 1 else 0
    rex = {"m": m, "n": n, "split": True, "max_abs_mean": ex["max_abs_mean"], "spread": ex["spread"], "sigma_b": ex["sigma_b"], "T": np.zeros_like(ex["wsum"]),
           "wsum": ex["wsum"], "wsum_zero": ex["wsum_zero"], "bsum_zero": ex["bsum_zero"]}
    with np.errstate(all="ignore"):
        _, rel_b, _ = H.bound(rex, ranks)                                   # (already doubled)
        base = 16.0 * U * ex["sumQ"] / ex["wsum"]
        rel_c = 2.0 * (base + (depth + Rk) * U)
        rel_w = 2.0 * (base + (P.merge_depth(m) + Rk) * U)
        if plain:
            e_mu = (math.log2(n) + 2.0) * U * ex["max_abs"]
            sd = np.sqrt(ex["wsum"] / (m * n))
            rel_c = rel_w = 2.0 * (2.0 * e_mu / sd + (e_mu / sd) ** 2 + (math.log2(m * n) + 6.0) * U)
            rel_b = 2.0 * (4.0 * e_mu / ex["sigma_b"] + (2.0 * e_mu / ex["sigma_b"]) ** 2 + (math.log2(m) + 6.0) * U)
            rel_b = np.where(ex["bsum_zero"], np.nan, rel_b)
        rel_c = np.where(ex["wsum_zero"], np.nan, rel_c); rel_w = np.where(ex["wsum_zero"], np.nan, rel_w)
        rel_W = np.nan_to_num(rel_w) + 2 * U
        rel_v = np.maximum(rel_W, np.nan_to_num(rel_b)) + 4 * U
        abs_rho = 2.0 * ((4.0 / 3.0) * (rel_W + np.nan_to_num(rel_c) + 4 * U + 2.0 * (rel_v + U)) + 4 * U)
        e_P = 2.0 * abs_rho + 8 * U
        abs_tau = 2.0 * ex["pairs"] * (e_P + U * np.abs(ex["tau"] + 1.0)) + 2 * U * np.abs(ex["tau"])
        rel_ess = abs_tau / np.abs(ex["tau"]) + 2 * U
    return {"rel_c": rel_c, "rel_w": rel_w, "rel_b": rel_b, "abs_rho": abs_rho, "abs_tau": abs_tau, "rel_ess": rel_ess}


def admissible(ex, ranks=1):
    """a condition on the exact quantities alone: every bound under the cap, both decision margins at least MARGIN_MIN"""
    b = bound(ex, ranks)
    ok = all(bool(np.all(np.isnan(b[k]) | (b[k] <= CAP))) for k in ("rel_c", "rel_w", "rel_b", "abs_rho"))
    return ok and bool(np.all(ex["margin_stop"] >= MARGIN_MIN) and np.all(ex["margin_clamp"] >= MARGIN_MIN))


def check(got, mir, ex, ranks=1, what="", plain=False):
    """got (dict as mirror returns) against the mirror bit for bit (mir = None: skipped), pairs against exact's, every continuous output within bound() of
    exact (plain: within the bounds of the plain two-pass form; a still unit's deviations are then rounding residue, not 0).  Returns the largest
    error / bound."""
    cols = ex["cols"]
    if mir is not None:
        for k in ("csum", "wsum", "mean", "bsum", "rho", "tau", "ess"):
            assert np.array_equal(got[k], mir[k], equal_nan=True), (what, k, got[k], mir[k])
        assert np.array_equal(got["pairs"], mir["pairs"]), (what, got["pairs"], mir["pairs"])
        assert (got["nunits"], got["nper"], got["lags"]) == (mir["nunits"], mir["nper"], mir["lags"]), what
    assert (got["nunits"], got["nper"], got["lags"]) == (ex["m"], ex["n"], ex["L"]), what
    assert admissible(ex, ranks), (what, bound(ex, ranks), ex["margin_stop"], ex["margin_clamp"])
    b = bound(ex, ranks, plain)
    worst = 0.0
    for i, j in enumerate(cols):
        assert got["pairs"][j] == ex["pairs"][i], (what, "pairs", j, got["pairs"][j], ex["pairs"][i])
        if ex["wsum_zero"][i]:
            assert got["wsum"][j] == 0.0 and not np.any(got["csum"][j]), (what, j)
        else:
            e = np.abs(got["csum"][j] - ex["csum"][i]).max() / ex["wsum"][i]
            assert e <= b["rel_c"][i], (what, "csum", j, e, b["rel_c"][i]); worst = max(worst, e / b["rel_c"][i])
            e = abs(got["wsum"][j] - ex["wsum"][i]) / ex["wsum"][i]
            assert e <= b["rel_w"][i], (what, "wsum", j, e, b["rel_w"][i]); worst = max(worst, e / b["rel_w"][i])
        if ex["bsum_zero"][i]:
            assert got["bsum"][j] == 0.0, (what, j)
        else:
            e = abs(got["bsum"][j] - ex["bsum"][i]) / ex["bsum"][i]
            assert e <= b["rel_b"][i], (what, "bsum", j, e, b["rel_b"][i]); worst = max(worst, e / b["rel_b"][i])
        E = 2.0 * (2.0 * (math.log2(ex["n"]) + 2.0 if plain else 1.0) * U * ex["max_abs_mean"][i] + (4 * (P.merge_depth(ex["m"]) + 1) + 1) * U * ex["spread"][i] + (ranks + 3) * U * ex["max_abs_mean"][i])
        assert abs(got["mean"][j] - ex["mean"][i]) <= E, (what, "mean", j, got["mean"][j], ex["mean"][i], E)
        if math.isnan(ex["tau"][i]):                                        # n < 4, or var+ = 0: NaN throughout
            assert np.all(np.isnan(got["rho"][j, 1:])) and math.isnan(got["tau"][j]) and math.isnan(got["ess"][j]), (what, j)
            continue
        e = np.abs(got["rho"][j] - ex["rho"][i]).max()
        assert e <= b["abs_rho"][i], (what, "rho", j, e, b["abs_rho"][i]); worst = max(worst, e / b["abs_rho"][i])
        e = abs(got["tau"][j] - ex["tau"][i])
        assert e <= b["abs_tau"][i], (what, "tau", j, e, b["abs_tau"][i]); worst = max(worst, e / b["abs_tau"][i])
        e = abs(got["ess"][j] - ex["ess"][i]) / abs(ex["ess"][i])
        assert e <= b["rel_ess"][i], (what, "ess", j, e, b["rel_ess"][i]); worst = max(worst, e / b["rel_ess"][i])
    return worst


# ---------------------------------------------------------------- the shapes the CPU and the GPU tests share
NS = H.NS                                                                   # (1, 2, 3, 255, 257, 1023, 1025, 3077)
MAXLAGS = (1, 7, 8, 15, 31, 32, 33, 64, 127)
NCOLS_KINDS = ("4", "5", "W-1", "W", "W+1", "200")


def ncols_of(kind, maxlag):
    W = maxlag + 1
    return max({"4": 4, "5": 5, "W-1": W - 1, "W": W, "W+1": W + 1, "200": 200}[kind], 2)


def dims_for(N):
    """every D of (1, 3, 4, 100, 1024) at the small chain counts, thinned out as N grows (as rhat_ref.dims_for)"""
    return {1: (1, 4, 1024), 2: (3, 100), 3: (1, 3, 4, 100, 1024), 255: (1, 4, 100), 257: (3, 100), 1023: (4,), 1025: (3,), 3077: (1, 4)}[N]


def cols_for(D):
    return sorted({0, D // 2, D - 1})


def launch_splits(ncols, kind):
    """the streamed path's launches: one; all of 32; a ragged cut with launches shorter than 32 and of 0"""
    if kind == "one":
        return [ncols]
    if kind == "32s":
        return R._fill(ncols, [32])
    out, left, i = [], ncols, 0
    parts = [3, 0, 1, 40, 0, 31, 33, 7]
    while left > 0:
        out.append(min(parts[i % len(parts)], left)); left -= out[-1]; i += 1
    return out + [0]


SPLIT_KINDS = ("one", "32s", "ragged")


def cases():
    """(N, D, maxlag, ncols, offset, splits kind, nranks): every (maxlag, ncols kind) at N = 3, D = 3; every (N, D) of dims_for with the windows, lengths,
    offsets, launch cuts and rank cuts cycling so that each value meets small and large shapes; the widest window on the most chains (3077 x 1, maxlag 127, 200 columns) once; 307,700 unit-series once"""
    out = []
    i = 0
    for ml in MAXLAGS:
        for kind in NCOLS_KINDS:
            out.append((3, 3, ml, ncols_of(kind, ml), OFFSETS[i % 3], SPLIT_KINDS[(i // 3) % 3], (1, 2, 3)[(i // 2) % 3]))
            i += 1
    for N in NS:
        for D in dims_for(N):
            big = N * D > 4096
            ml = (7, 15, 31, 33)[i % 4] if big else MAXLAGS[i % len(MAXLAGS)]
            kind = ("5", "W+1", "200", "W")[i % 4] if big else NCOLS_KINDS[(i // 2) % len(NCOLS_KINDS)]
            rb = sorted(H.rank_bounds(N))
            out.append((N, D, ml, ncols_of(kind, ml), OFFSETS[i % 3], SPLIT_KINDS[(i // 3) % 3], rb[i % len(rb)]))
            i += 1
    out.append((3077, 1, 127, 200, 1e6, "ragged", 4))
    out.append((3077, 100, 7, 9, 0.0, "one", 2))                             # more unit-series than stage 1 has lanes: several per lane
    out.append((257, 4, 64, 17, 1e4, "ragged", 4))
    return list(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(hist, {split: exact}, seed) of a case: the first seed whose input is admissible for one handle and for the case's rank count, in both forms where
    the split form exists (ncols >= 8) — the choice looks at the exact quantities only"""
    N, D, ml, ncols, offset, _, nranks = case
    for seed in range(16):
        hist = make_hist(N, D, ncols, offset, seed)
        exs = {sp: exact(hist, ml, sp, cols_for(D)) for sp in ((False, True) if ncols >= 8 else (False,))}
        if all(admissible(ex, r) for ex in exs.values() for r in {1, nranks}):
            hist.setflags(write=False)
            return hist, exs, seed
    raise AssertionError(("no admissible seed", case))


# ---------------------------------------------------------------- klara_selftest_ess through ctypes (the GPU tests; the CPU suite calls it for its refusals)
SLOTS = {("streamed", False): 0, ("streamed", True): 1, ("history", False): 2, ("history", True): 3, ("split", False): 4, ("split", True): 5}


def selftest(lib, hist, maxlag, splits, bounds, device=0):
    """(status, {(path, ranks): dict as mirror returns}) of klara_selftest_ess on the history (ncols, N, D); a path that did not run (split under 8
    columns) is absent"""
    ncols, N, D = hist.shape
    R1 = maxlag + 1
    hist = np.ascontiguousarray(hist, dtype=np.float64)
    sp = np.asarray(splits, dtype=np.int64); bd = np.asarray(bounds, dtype=np.int64)
    out = np.full((6, 5, D), np.nan); rho = np.full((6, D * R1), np.nan); csum = np.full((6, D * R1), np.nan)
    pairs = np.zeros((6, D), dtype=np.int32); cnt = np.zeros((6, 3), dtype=np.uint64)
    st = lib.klara_selftest_ess(device, N, D, ncols, hist.ctypes.data, maxlag, len(sp), sp.ctypes.data, len(bd) - 1, bd.ctypes.data, out.ctypes.data,
                                rho.ctypes.data, csum.ctypes.data, pairs.ctypes.data, cnt.ctypes.data)
    res = {}
    for key, s in SLOTS.items():
        m, n, L = (int(v) for v in cnt[s])
        if st != 0 or m == 0:
            continue
        res[key] = {"ess": out[s, 0], "tau": out[s, 1], "mean": out[s, 2], "wsum": out[s, 3], "bsum": out[s, 4], "pairs": pairs[s],
                    "rho": rho[s, :D * (L + 1)].reshape(D, L + 1), "csum": csum[s, :D * (L + 1)].reshape(D, L + 1), "nunits": m, "nper": n, "lags": L}
    return st, res
