"""References for the Gelman–Rubin diagnostic (klara_rhat.hip: k_rhat_stage1 / k_rhat_stage2 over the chains' running sums, k_rhat_halves over the stored
history for the split form; klara_comm.hip: the between-rank merge of klara_merge.h with chains where the samples stand, behind klara_gather_rhat and
klara_selftest_rhat).  A "unit" is a chain, or for the split form a half-chain (unit 2 c + half); m units of n samples each.

  units_of_sums(inp) / units_of_hist(hist)   every unit's exact integer sums (s, q) over a common denominator, for exact()
  exact(...)                                 mean, Wsum, Bsum, R-hat^2 of chosen columns from the input doubles in exact rational arithmetic
  mirror(inp=..., hist=...)                  NumPy restatement of the kernels' order of operations, both paths
  mirror_ranks(..., bounds)                  mirror() of every shard, then the between-rank merge with the all-reduces as ascending sums from zero
  bound(ex, ranks)                           derived worst-case relative bounds on Wsum, Bsum and R-hat against exact (see its docstring)
and the inputs the CPU and GPU tests share: pooled_ref.make_inputs for the sums, make_hist for the history, on the same dyadic grid.  CPU only.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import pooled_ref as P

U, CAP, GRID, SD = P.U, P.CAP, P.GRID, P.SD
THREADS, POOL_BLOCKS = P.THREADS, P.POOL_BLOCKS
OFFSETS = (0.0, 242.0, 1e6)


# ---------------------------------------------------------------- inputs
def make_hist(N, D, ncols, offset=0.0, seed=0, still="some"):
    """A value history (ncols, N, D) — column t at hist[t], as the device keeps it — of series offset * SD + SD z on GRID.  In each half [0, h) and
    [ncols - h, ncols), h = ncols // 2 >= 2, the first and the last sample of a moving chain are at least 2 SD apart, so that the half's exact M2 is at
    least 2 SD^2 > pooled_ref.MARGIN.  still = "some": chains c % 9 == 4 never move (state on a grid of 1/2: every half's M2 is exactly 0) and chains
    c % 9 == 7 stand still through their first half only; "all": every chain stands still at its own state; "same": all at one state; "none"."""
    rng = np.random.default_rng([20261021, seed, N, D, ncols])
    base = float(offset) * SD
    assert base / GRID == round(base / GRID) and ncols >= 2
    x = base + np.rint(SD * rng.standard_normal((ncols, N, D)) / GRID) * GRID
    h = ncols // 2
    if h >= 2:
        for a, b in ((0, h - 1), (ncols - h, ncols - 1)):
            d = x[b] - x[a]
            x[b] = np.where(np.abs(d) < 2 * SD, x[a] + np.where(d < 0, -2 * SD, 2 * SD), x[b])
    X = base + np.rint(SD * rng.standard_normal((N, D)) * 2) / 2
    c = np.arange(N)
    if still == "some":
        x[:, c % 9 == 4] = X[c % 9 == 4]
        x[:h, c % 9 == 7] = X[c % 9 == 7]
    elif still == "all":
        x[:] = X
    elif still == "same":
        x[:] = X[0]
    else:
        assert still == "none"
    return np.ascontiguousarray(x)


def still_inputs(N, D, nsaved, offset=0.0, seed=0, same=False):
    """pooled_ref.make_inputs with every chain still (held = nsaved, its sums exact): Wsum is exactly 0; same: all at one state, Bsum exactly 0 too."""
    inp = P.make_inputs(N, D, nsaved, offset, seed)
    rng = np.random.default_rng([20261022, seed, N, D])
    X = float(offset) * SD + np.rint(SD * rng.standard_normal((N, D)) * 2) / 2
    if same:
        X[:] = X[0]
    inp["X"] = X; inp["held"] = np.full(N, nsaved, dtype=np.int64)
    inp["sum"] = np.zeros((N, D)); inp["sumsq"] = np.zeros((N, D))
    return inp


# ---------------------------------------------------------------- exact
def units_of_sums(inp, cols):
    """(s, q, sden, qden, n): the chains' sums of the columns `cols` as the device views them (pooled_ref.chain_view), as integers over common denominators"""
    s, q = P.chain_view(inp)
    out_s, out_q = [], []
    sden = qden = 1
    pairs = {}
    for j in cols:
        pairs[j] = ([float(a).as_integer_ratio() for a in s[:, j]], [float(a).as_integer_ratio() for a in q[:, j]])
        sden = max(sden, max(d for _, d in pairs[j][0])); qden = max(qden, max(d for _, d in pairs[j][1]))
    for j in cols:
        out_s.append([p * (sden // d) for p, d in pairs[j][0]]); out_q.append([p * (qden // d) for p, d in pairs[j][1]])
    return out_s, out_q, sden, qden, int(inp["nsaved"])


def units_of_hist(hist, cols):
    """the same for the 2 N half-chains of a history on GRID: s in units of GRID, q of GRID^2, exact integers"""
    ncols, N, D = hist.shape
    h = ncols // 2
    k = hist[:, :, list(cols)] / GRID
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() < 2.0 ** 31
    k = k.astype(np.int64)
    halves = np.stack([k[:h], k[ncols - h:]], axis=2)                         # (h, N, 2, cols)
    s = halves.sum(axis=0).reshape(2 * N, len(cols)); q = (halves * halves).sum(axis=0).reshape(2 * N, len(cols))
    return [[int(a) for a in s[:, i]] for i in range(len(cols))], [[int(a) for a in q[:, i]] for i in range(len(cols))], int(1 / GRID), int(1 / GRID) ** 2, h


def exact(inp=None, hist=None, cols=None):
    """Exact quantities per column of `cols` over m units of n samples: mean = (1 / m) sum mu_u, wsum = sum (q_u - s_u^2 / n), bsum = sum (mu_u - mean)^2 =
    (sum s_u^2 - S^2 / m) / n^2, rhat2 = (n - 1) / n + m (n - 1) bsum / ((m - 1) wsum) (NaN for m < 2 or n < 2, inf for wsum = 0 < bsum, NaN for both 0),
    each the correctly rounded rational; wsum_zero / bsum_zero say which are exactly 0; max_abs_mean and spread of the units' means, sigma_b =
    sqrt(bsum / m), T = sum s_u^2 / n (what the cancelling subtraction removes), and m, n."""
    if inp is not None:
        D = inp["sum"].shape[1]
        cols = list(range(D)) if cols is None else list(cols)
        S, Q, sden, qden, n = units_of_sums(inp, cols)
    else:
        D = hist.shape[2]
        cols = list(range(D)) if cols is None else list(cols)
        S, Q, sden, qden, n = units_of_hist(hist, cols)
    out = {k: np.zeros(len(cols)) for k in ("mean", "wsum", "bsum", "rhat2", "max_abs_mean", "spread", "sigma_b", "T")}
    out["wsum_zero"] = np.zeros(len(cols), dtype=bool); out["bsum_zero"] = np.zeros(len(cols), dtype=bool)
    m = len(S[0])
    for i in range(len(cols)):
        si, qi = S[i], Q[i]
        tot = sum(si); ss = sum(a * a for a in si)
        mean = Fraction(tot, sden * n * m)
        wsum = Fraction(sum(qi), qden) - Fraction(ss, sden * sden * n)
        bsum = Fraction(ss * m - tot * tot, m * sden * sden * n * n)
        assert wsum >= 0 and bsum >= 0 and min(a * sden * sden * n - b * b * qden for a, b in zip(qi, si)) >= 0     # true series: no unit's M2 is negative
        out["mean"][i] = float(mean); out["wsum"][i] = float(wsum); out["bsum"][i] = float(bsum)
        out["wsum_zero"][i] = wsum == 0; out["bsum_zero"][i] = bsum == 0
        if m < 2 or n < 2:
            out["rhat2"][i] = math.nan
        elif wsum == 0:
            out["rhat2"][i] = math.inf if bsum > 0 else math.nan
        else:
            out["rhat2"][i] = float(Fraction(n - 1, n) + Fraction(m * (n - 1), m - 1) * bsum / wsum)
        mu = np.array([a / (sden * n) for a in si])
        out["max_abs_mean"][i] = np.abs(mu).max(); out["spread"][i] = mu.max() - mu.min()
        out["sigma_b"][i] = math.sqrt(float(bsum) / m)
        out["T"][i] = float(Fraction(ss, sden * sden * n))
    out["m"], out["n"], out["cols"], out["split"] = m, n, cols, hist is not None
    if hist is not None:                                                     # the split kernel sums z = x - (the half's first sample): its own s, q
        ncols = hist.shape[0]
        z = np.concatenate([hist[:n] - hist[0], hist[ncols - n:] - hist[ncols - n]])[:, :, cols]
        out["T"] = (np.abs(z).max(axis=(0, 1)) ** 2) * n * m                 # sum over the units of (sum z)^2 / n <= m n max z^2
    return out


# ---------------------------------------------------------------- mirror
def rhat_value(wsum, bsum, m, n):
    """rhat_value of klara_rhat.hip, elementwise"""
    if m < 2 or n < 2:
        return np.full(np.shape(wsum), np.nan)
    m, n = float(m), float(n)
    with np.errstate(all="ignore"):
        W = wsum / (m * (n - 1.0)); Bn = bsum / (m - 1.0)
        return np.sqrt((((n - 1.0) / n) * W + Bn) / W)


def units_mirror_sums(inp):
    """(mu[N, D], m2[N, D]) as chain_moments of klara_rhat.h forms them — the very values k_moments_stage1 merges"""
    s, q = P.chain_view(inp)
    return P.chain_moments(s, q, float(inp["nsaved"]))


def units_mirror_hist(hist):
    """(mu[2 N, D], m2[2 N, D]) as k_rhat_halves forms them: both halves summed as z = x - (the half's first sample) in sample order, s = sum z, q = sum z z,
    then moments_of_sums (pooled_ref.chain_moments) and mean = first + mean of z"""
    ncols, N, D = hist.shape
    h = ncols // 2
    va, vb = hist[:h], hist[ncols - h:]
    sa = np.zeros((N, D)); qa = np.zeros((N, D)); sb = np.zeros((N, D)); qb = np.zeros((N, D))
    for t in range(h):
        za = va[t] - va[0]; zb = vb[t] - vb[0]
        sa = sa + za; qa = qa + za * za
        sb = sb + zb; qb = qb + zb * zb
    ma, m2a = P.chain_moments(sa, qa, float(h))
    mb, m2b = P.chain_moments(sb, qb, float(h))
    mu = np.stack([va[0] + ma, vb[0] + mb], axis=1).reshape(2 * N, D)
    m2 = np.stack([m2a, m2b], axis=1).reshape(2 * N, D)
    return mu, m2


def reduce_units(mu, m2):
    """(mean[D], bsum[D], wsum[D]) as k_rhat_stage1 / k_rhat_stage2 form them from the units' (mu, m2): the means shifted by unit 0's, chan_merge at unit
    weight over u = b, b + nb, ... per block, the plain ascending sum of m2; per thread the partials b = t, t + 256, ... with their unit counts; the tree"""
    M, D = mu.shape
    nb = min(M, POOL_BLOCKS)
    pivot = mu[0].copy()
    d = mu - pivot
    k = np.zeros((nb, 1)); mean = np.zeros((nb, D)); bs = np.zeros((nb, D)); ws = np.zeros((nb, D))
    for c in range((M + nb - 1) // nb):
        a = min(nb, M - c * nb)
        k[:a], mean[:a], bs[:a] = P.chan_merge(k[:a], mean[:a], bs[:a], 1.0, d[c * nb:c * nb + a], 0.0)
        ws[:a] = ws[:a] + m2[c * nb:c * nb + a]
    b = np.arange(nb)
    units = ((M - b + nb - 1) // nb).astype(np.float64)[:, None]
    tn = np.zeros((THREADS, 1)); tm = np.zeros((THREADS, D)); tb = np.zeros((THREADS, D)); tw = np.zeros((THREADS, D))
    for c in range((nb + THREADS - 1) // THREADS):
        a = min(THREADS, nb - c * THREADS)
        sl = slice(c * THREADS, c * THREADS + a)
        tn[:a], tm[:a], tb[:a] = P.chan_merge(tn[:a], tm[:a], tb[:a], units[sl], mean[sl], bs[sl])
        tw[:a] = tw[:a] + ws[sl]
    w = THREADS // 2
    while w > 0:
        tn[:w], tm[:w], tb[:w] = P.chan_merge(tn[:w], tm[:w], tb[:w], tn[w:2 * w], tm[w:2 * w], tb[w:2 * w])
        tw[:w] = tw[:w] + tw[w:2 * w]
        w >>= 1
    return pivot + tm[0], tb[0].copy(), tw[0].copy()


def _result(mean, bsum, wsum, m, n):
    return {"rhat": rhat_value(wsum, bsum, m, n), "mean": mean, "wsum": wsum, "bsum": bsum, "nchains": int(m), "nper": int(n)}


def mirror(inp=None, hist=None):
    """klara_gather_rhat without a communicator, unsplit from the sums `inp` or split from the history `hist`: dict as Engine.rhat returns it"""
    if inp is not None:
        mu, m2 = units_mirror_sums(inp); n = int(inp["nsaved"])
    else:
        mu, m2 = units_mirror_hist(hist); n = hist.shape[0] // 2
    mean, bsum, wsum = reduce_units(mu, m2)
    return _result(mean, bsum, wsum, mu.shape[0], n)


def merge_ranks(parts):
    """The between-rank merge from every rank's mirror() result: (m_r, mean_r, bsum_r) as pooled_ref.between_ranks merges (n_r, mean_r, M2_r), wsum an
    ascending sum from 0.0; the same n on every rank"""
    n = parts[0]["nper"]
    assert all(p["nper"] == n for p in parts)
    mean, bsum, m = P.between_ranks([p["mean"] for p in parts], [p["bsum"] for p in parts], [p["nchains"] for p in parts])
    wsum = np.zeros_like(mean)
    for p in parts:
        wsum = wsum + p["wsum"]
    return _result(mean, bsum, wsum, m, n)


def mirror_ranks(bounds, inp=None, hist=None):
    parts = []
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        parts.append(mirror(inp=P.slice_inputs(inp, c0, c1)) if inp is not None else mirror(hist=np.ascontiguousarray(hist[:, c0:c1])))
    return merge_ranks(parts)


# ---------------------------------------------------------------- bound
def bound(ex, ranks=1):
    """(rel_w, rel_b, rel_r): worst-case relative bounds on |wsum - exact|, |bsum - exact| and |rhat - exact| per column of exact()'s result, for the
    device's order of operations (`ranks` > 1: cut into that many shards and merged between them).  First order in u = 2^-53, doubled for the rest.

    Notation: m units of n samples, L = pooled_ref.merge_depth(m), M = max |mu_u|, spread = max mu_u - min mu_u, sigma_b = sqrt(bsum / m), R = ranks.
    The units' sums (s_u, q_u) are exact: inputs for the unsplit form; for the split form x - x_first, its sum and the sum of its squares are exact on the
    dyadic grid of make_hist (multiples of 2^-4 and 2^-8 below 2^53 of them; tests/test_rhat_host.py checks this on the mirror).
      per unit: M2_u = (q - qh) - ql as in pooled_ref.bound: 3 u M2_u + 4 u^2 s_u^2 / n.  mu_u = fl(s / n) is off by e_mu = u M; for the split form it is
        fl(first + fl(s / n)): e_mu = 2 u M.
      wsum: a sum of m non-negative terms along a path of L additions: L u relative.  With the above
            rel_w = (L + 3) u + 4 u^2 T / wsum,  T = sum_u s_u^2 / n     (+ R u for the sum over the ranks)
      bsum does not change when every mean is shifted by one number, so the pivot's own error does not enter; the shifted values mu_u - pivot carry e_mu
        and the rounding of the subtraction, u spread: e_in = e_mu + u spread.  They are of size spread at most, so the merges of pooled_ref.bound add
        E' = 4 (L + 1) u spread to a running mean (there: (L + 1) u (M + 3 spread) with M -> spread), on top of an average of the e_in.  A delta is the
        difference of two such: e_d = 2 e_in + 2 E' + u spread.  As there, exactly sum delta^2 k w = bsum (Chan) and Cauchy-Schwarz over the merges
        gives 2 sqrt(F) e_d / sigma_b + F (e_d / sigma_b)^2, F m bounding the sum of the weights k w = k k_b / (k + k_b) <= min(k, k_b) of all merges: at
        most m in stage 1 — and none unless a block holds two units, m > 1024 —, at most m in stage 2's sequential part — none unless nb > 256 —, and
        m / 2 per level of the tree that merges two non-empty operands, ceil(log2(min(nb, 256))) levels:
            F = [m > 1024] + [nb > 256] + ceil(log2(min(nb, 256))) / 2   (6 at most, 1 / 2 for two units);  the sums' roundings add (2 L + 8) u.
        Cut into shards, the same holds shard by shard with the absolute errors adding up under one more Cauchy-Schwarz (sum bsum_r <= bsum).
      between ranks: mean_r = fl(pivot + shifted mean) is off by E = e_in + E' + u M; sum_r fl(m_r mean_r) / m by E (an average of those) plus u M for
        every product, (R - 1) u M for the additions and u M for the division; so d_r = mean_r - mean by e_r = 2 E + (R + 1) u M + u spread.  Exactly sum m_r d_r^2 <= bsum and the weights add up to m:  2 e_r / sigma_b + (e_r / sigma_b)^2,
        plus (R + 4) u for the roundings of the terms and their sum.
      rhat^2 = (n - 1) / n + m (n - 1) bsum / ((m - 1) wsum) with both terms positive: its relative error is at most rel_b + rel_w, that of the
        square root half of it; 4 u more for the evaluation's own divisions, product, sum and root.
    The offset enters through u M in e_mu alone (the pivot keeps it out of every merge): at 1e6 sd and sigma_b = 0.06 (two chains of 200 samples)
    rel_b is about 5e-8.  Columns whose exact wsum or bsum is 0 have no relative bound (the tests compare them exactly): NaN there."""
    m, n = ex["m"], ex["n"]
    L = P.merge_depth(m)
    M, spread, sb = ex["max_abs_mean"], ex["spread"], ex["sigma_b"]
    with np.errstate(all="ignore"):
        rel_w = (L + 3) * U + 4.0 * U * U * ex["T"] / ex["wsum"] + (ranks * U if ranks > 1 else 0.0)
        e_in = (2.0 if ex["split"] else 1.0) * U * M + U * spread
        nb = min(m, POOL_BLOCKS)
        F = (1.0 if m > POOL_BLOCKS else 0.0) + (1.0 if nb > THREADS else 0.0) + 0.5 * math.ceil(math.log2(min(nb, THREADS))) if m > 1 else 0.0
        Ep = 4.0 * (L + 1) * U * spread
        e_d = 2.0 * e_in + 2.0 * Ep + U * spread
        rel_b = (2 * L + 8) * U + 2.0 * math.sqrt(F) * e_d / sb + F * (e_d / sb) ** 2
        if ranks > 1:
            E = e_in + Ep + U * M
            e_r = 2.0 * E + (ranks + 1) * U * M + U * spread
            rel_b = rel_b + (ranks + 4) * U + 2.0 * e_r / sb + (e_r / sb) ** 2
        rel_w = np.where(ex["wsum_zero"], np.nan, 2.0 * rel_w); rel_b = np.where(ex["bsum_zero"], np.nan, 2.0 * rel_b)
        rel_r = 0.5 * (np.nan_to_num(rel_w) + np.nan_to_num(rel_b)) + 4.0 * U       # (a sum that is exactly 0 is returned as 0: no error from it)
    return rel_w, rel_b, rel_r


def admissible(ex, ranks=1):
    """every column with a relative bound has it under the cap"""
    rel_w, rel_b, _ = bound(ex, ranks)
    return bool(np.all(np.isnan(rel_w) | (rel_w <= CAP)) and np.all(np.isnan(rel_b) | (rel_b <= CAP)))


def check(got, mir, ex, ranks=1, what=""):
    """got (dict of arrays as Engine.rhat / mirror return) against the mirror bit for bit (mir = None: skipped) and against exact within bound();
    columns whose exact wsum or bsum is zero are compared exactly (0, and inf or NaN for R-hat as defined).  Returns the largest error / bound."""
    cols = ex["cols"]
    if mir is not None:
        for k in ("rhat", "mean", "wsum", "bsum"):
            assert np.array_equal(got[k], mir[k], equal_nan=True), (what, k, got[k], mir[k])
        assert got["nchains"] == mir["nchains"] and got["nper"] == mir["nper"], what
    assert got["nchains"] == ex["m"] and got["nper"] == ex["n"], what
    assert admissible(ex, ranks), (what, bound(ex, ranks))
    rel_w, rel_b, rel_r = bound(ex, ranks)
    worst = 0.0
    for i, j in enumerate(cols):
        w, b, r = got["wsum"][j], got["bsum"][j], got["rhat"][j]
        if ex["wsum_zero"][i]:
            assert w == 0.0, (what, j, w)
        else:
            e = abs(w - ex["wsum"][i]) / ex["wsum"][i]
            assert e <= rel_w[i], (what, "wsum", j, e, rel_w[i]); worst = max(worst, e / rel_w[i])
        if ex["bsum_zero"][i]:
            assert b == 0.0, (what, j, b)
        else:
            e = abs(b - ex["bsum"][i]) / ex["bsum"][i]
            assert e <= rel_b[i], (what, "bsum", j, e, rel_b[i]); worst = max(worst, e / rel_b[i])
        r2 = ex["rhat2"][i]
        if math.isnan(r2):
            assert math.isnan(r), (what, j, r)
        elif math.isinf(r2):
            assert r == math.inf, (what, j, r)
        else:
            e = abs(r - math.sqrt(r2)) / math.sqrt(r2)
            assert e <= rel_r[i], (what, "rhat", j, e, rel_r[i]); worst = max(worst, e / rel_r[i])
        E = 2.0 * (2.0 * U * ex["max_abs_mean"][i] + (4 * (P.merge_depth(ex["m"]) + 1) + 1) * U * ex["spread"][i] + (ranks + 3) * U * ex["max_abs_mean"][i])
        assert abs(got["mean"][j] - ex["mean"][i]) <= E, (what, "mean", j, got["mean"][j], ex["mean"][i], E)
    return worst


# ---------------------------------------------------------------- the shapes the CPU and the GPU tests share
NS = (1, 2, 3, 255, 257, 1023, 1025, 3077)
NSAVED = (1, 2, 3, 200)
NCOLS = (3, 4, 5, 7, 200)


def dims_for(N, n):
    """D = 1 and 3 everywhere; 257 (across the 256-thread stride over the dimensions) at a small chain count and, for the short series, at a multi-block one"""
    return (1, 3, 257) if N == 3 or (N == 1025 and n <= 7) else (1, 3)


def cols_for(D):
    return sorted({0, D // 2, D - 1})


def rank_bounds(N):
    """nranks -> shard boundaries, uneven, with a one-chain shard where N allows"""
    out = {1: [0, N]}
    if N >= 2:
        out[2] = [0, 1, N]
    if N >= 3:
        out[3] = [0, N // 3, N - 1, N] if N // 3 >= 1 else [0, 1, 2, N]
    if N >= 255:
        out[4] = [0, 1, N // 2 - 7, N - 100, N]
    return out


def first_admissible(make, ranks, tries=16):
    """make(seed) -> (inputs, exact): the first seed whose inputs have every bound under the cap for every rank count in `ranks` (the choice looks at the
    exact quantities only)"""
    for seed in range(tries):
        data, ex = make(seed)
        if all(admissible(ex, r) for r in ranks):
            return data, ex, seed
    raise AssertionError("no admissible seed")
