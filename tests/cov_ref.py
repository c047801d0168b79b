"""References for the pooled posterior covariance (klara_cov.hip: k_cov_update behind every launch of a job with KLARA_MON_COVARIANCE, k_cov_finalize
behind klara_gather_covariance, then between ranks klara_comm.hip's k_scale / k_merge_between in the one sequence of klara_merge.h merge_ranks).

  exact(hist, pairs)              mean (all dimensions) and M_ij = sum x_i x_j - (sum x_i)(sum x_j) / n on the (i, j) pairs in exact integer arithmetic (every
                                  double is a dyadic rational; nothing is rounded before the final conversion)
  mirror(hist, splits)            NumPy restatement of the kernels' order of operations: z = x - pivot, the slabs of slab(N, D) chains, every element of S_s one
                                  fma chain over (saved step, then chain) with the saved step padded to 4 chains by zeros, launch by launch, T_s a plain sum in
                                  the same order, the slabs added in ascending order, M = (S - qh) - ql with T_i T_j / n = qh + ql, the diagonal's clamp.
                                  v_mfma_f64_16x16x4_f64 is one fma chain over k ascending from C (klara_selftest_mfma_f64 pins it), so the instruction adds
                                  nothing to the order.  fma() is exact (checked against rational arithmetic in tests/test_cov_host.py).
  mirror_ranks(hist, bounds)      mirror() of every shard, then the between-rank merge with the all-reduces as sums over the ranks in ascending order from 0
  bound(hist) / bound_ranks(...)  derived worst-case bounds on |device - exact| (see their docstrings)
and the inputs the CPU and GPU tests share.  CPU only.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import pooled_ref as P

U = 2.0 ** -53
SLAB_MIN = 64                       # KLARA_COV_SLAB_MIN
MAX_COLS = 32                       # KLARA_COV_MAX_COLS
WORKSPACE_BYTES = 480 << 20         # KLARA_COV_WORKSPACE_BYTES
SD = P.SD


# ---------------------------------------------------------------- geometry
def slab(N, D):
    """klara_cov_slab: chains per slab, a function of (N, D) alone"""
    mt = (D + 15) // 16
    per = (mt * (mt + 1) // 2 * 256 + 16 * mt) * 8
    ch = SLAB_MIN
    while -(-N // ch) * per > WORKSPACE_BYTES:
        ch *= 2
    return ch


CH = slab(1, 3)                     # the slab of every shape the tests use (64)


# ---------------------------------------------------------------- inputs
def make_hist(N, D, ncols, offset=0.0, seed=0):
    """(ncols, N, D) full-mantissa values offset * SD + SD (0.6 g + 0.8 e_d + 0.3 e_(d-1)): a factor g shared by all coordinates of a sample
    (correlation 0.36 between distant coordinates) and a neighbour term, so that no covariance is near zero by construction."""
    rng = np.random.default_rng([20261019, 77, seed, N, D, ncols])
    g = rng.standard_normal((ncols, N, 1))
    e = rng.standard_normal((ncols, N, D + 1))
    return np.ascontiguousarray(float(offset) * SD + SD * (0.6 * g + 0.8 * e[:, :, 1:] + 0.3 * e[:, :, :-1]))


def const_hist(N, D, ncols, seed=0):
    """every chain at one full-mantissa point for all saved steps"""
    v = 242.0 * SD + SD * np.random.default_rng([20261019, 78, seed, D]).standard_normal(D)
    return np.ascontiguousarray(np.broadcast_to(v, (ncols, N, D))), v


def pairs(D):
    """a fixed handful of (i, j): corners, both sides of every tile edge the dimension has, and two pairs below the diagonal"""
    cand = [(0, 0), (0, D - 1), (D - 1, D - 1), (D - 1, 0), (D // 2, D // 3), (15, 15), (15, 16), (16, 16), (16, 17), (0, 16), (15, 31), (31, 32), (17, 15),
            (127, 128), (128, 128), (100, 255), (240, 255), (255, 255)]
    out = []
    for i, j in cand:
        if i < D and j < D and (i, j) not in out:
            out.append((i, j))
    return out


# ---------------------------------------------------------------- exact
def _ints(v):
    prs = [float(a).as_integer_ratio() for a in v]
    den = max(d for _, d in prs)
    return [p * (den // d) for p, d in prs], den


def exact(hist, prs=None):
    """{"mean": (D,), "M": {(i, j): float}, "n": int}: correctly rounded exact rationals over all ncols * N samples"""
    ncols, N, D = hist.shape
    n = ncols * N
    x = hist.reshape(n, D)
    prs = pairs(D) if prs is None else prs
    cols = {}
    for d in range(D):
        cols[d] = _ints(x[:, d])
    mean = np.array([float(Fraction(sum(cols[d][0]), cols[d][1] * n)) for d in range(D)])
    M = {}
    for i, j in prs:
        (xi, di), (xj, dj) = cols[i], cols[j]
        sij = sum(a * b for a, b in zip(xi, xj))
        M[(i, j)] = float(Fraction(sij * n - sum(xi) * sum(xj), di * dj * n))
    return {"mean": mean, "M": M, "n": n}


# ---------------------------------------------------------------- exact fma on arrays
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """a * b + c rounded once, elementwise.  a b = p + e and p + c = s + t exactly (Dekker, Knuth), t + e = u + v exactly; u is then rounded to odd
    (Boldo & Melquiond: when v != 0 and u's last mantissa bit is even, u moves one ulp towards v) so that the last addition s + u rounds the exact
    value correctly: u carries 53 bits below s's last place — or p + c was exact (t = 0, v = 0) and s + e is a single rounding anyway.  Finite
    operands without overflow or underflow in the product."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p, e = P.two_prod(a, b)
    s, t = two_sum(p, c)
    u, v = two_sum(t, e)
    even = (u.view(np.int64) & 1) == 0
    fix = (v != 0.0) & even
    if np.any(fix):
        u = np.where(fix, np.nextafter(u, np.where(v > 0.0, np.inf, -np.inf)), u)
    return s + u


# ---------------------------------------------------------------- mirror
def _launches(splits):
    """the kernel launches of a job's launches: pieces of at most MAX_COLS saved steps (klara_cov_launch_update), empty ones skipped"""
    out = []
    for m in splits:
        m = int(m)
        while m > 0:
            out.append(min(m, MAX_COLS)); m -= out[-1]
    return out


def accumulate(hist, splits=None):
    """(pivot, S (nslabs, D, D) upper triangle filled, T (nslabs, D)) as k_cov_update leaves them after the launches `splits` (default: one launch per
    MAX_COLS saved steps).  The accumulators go to memory and come back between launches — no arithmetic — and the padding samples (chains of a saved
    step beyond the slab's, up to a multiple of 4) are z = 0: fma(0, 0, acc) = acc and T + 0 = T, applied as such."""
    ncols, N, D = hist.shape
    splits = [ncols] if splits is None else list(splits)
    assert sum(splits) == ncols
    ch = slab(N, D)
    ns = -(-N // ch)
    pivot = hist[0, 0].copy()
    z = np.zeros((ncols, ns * ch, D))
    z[:, :N] = hist - pivot
    z = z.reshape(ncols, ns, ch, D)
    iu, ju = np.triu_indices(D)
    S = np.zeros((ns, iu.size)); T = np.zeros((ns, D))
    nc_max = min(ch, N)
    ncp = (nc_max + 3) & ~3
    col = 0
    for m in _launches(splits):
        s_in, t_in = S.copy(), T.copy()                                     # the launch reads its accumulators ...
        for t in range(col, col + m):
            for cc in range(ncp):
                zz = z[t, :, cc] if cc < ch else np.zeros((ns, D))          # (a padding sample: zeros)
                s_in = fma(zz[:, iu], zz[:, ju], s_in)
                t_in = t_in + zz
        S, T = s_in, t_in                                                    # ... and stores them
        col += m
    full = np.zeros((ns, D, D))
    full[:, iu, ju] = S
    return pivot, full, T


def finalize(pivot, S, T, n):
    """(mean, M) as k_cov_finalize forms them from the slabs' accumulators"""
    D = pivot.size
    s = np.zeros((D, D)); t = np.zeros(D)
    for k in range(S.shape[0]):
        s = s + S[k]; t = t + T[k]
    nn = float(n)
    with np.errstate(all="ignore"):
        ti, tj = np.broadcast_arrays(t[:, None], t[None, :])
        p, pe = P.two_prod(ti, tj)
        qh = p / nn
        r = P.fma_remainder(qh, nn, p)
        ql = (r + pe) / nn
        v = (s - qh) - ql
        d = np.diag(v).copy()
        v[np.diag_indices(D)] = np.where(d < 0.0, 0.0, d)
        M = np.triu(v) + np.triu(v, 1).T
        return pivot + t / nn, M


def mirror(hist, splits=None):
    ncols, N, D = hist.shape
    pivot, S, T = accumulate(hist, splits)
    return finalize(pivot, S, T, ncols * N)


def between_ranks(means, Ms, counts):
    """klara_gather_covariance's between-rank merge: n_r mean_r summed over the ranks (ascending, from 0.0), mean = that / sum n_r,
    M = sum over the ranks of M_r + n_r d d' with d = mean_r - mean."""
    D = means[0].size
    wsum = np.zeros(D); ntot = 0
    for mr, nr in zip(means, counts):
        wsum = wsum + float(nr) * mr
        ntot += int(nr)
    mean = wsum / float(ntot) if ntot > 0 else np.zeros(D)
    M = np.zeros((D, D))
    for mr, qr, nr in zip(means, Ms, counts):
        d = mr - mean
        M = M + (qr + float(nr) * (d[:, None] * d[None, :]))
    return mean, M, ntot


def mirror_ranks(hist, bounds, splits=None):
    """(mean, M, (saved samples, chains)) of the chains cut into the shards [bounds[r], bounds[r + 1]); also the shards' own (mean_r, M_r, n_r)"""
    ncols, N, D = hist.shape
    assert bounds[0] == 0 and bounds[-1] == N and all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
    means, Ms, counts = [], [], []
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        mr, qr = mirror(np.ascontiguousarray(hist[:, c0:c1]), splits)
        means.append(mr); Ms.append(qr); counts.append(ncols * (c1 - c0))
    mean, M, ntot = between_ranks(means, Ms, counts)
    return mean, M, (ntot, N), (means, Ms, counts)


# ---------------------------------------------------------------- bound
def bound(hist):
    """(E (D, D), Emean (D,)): absolute worst-case bounds on |M - exact M| and |mean - exact mean| for the device's order of operations on this
    history, first order in u = 2^-53, doubled for the rest.

    Notation: z = x - pivot (the exact M and mean - pivot do not depend on the pivot); A_ij = sum |z_i z_j|, B_i = sum |z_i| over all n samples;
    L = saved steps x chains of a slab, the length of the fma chains; NS = slabs.
      shift: the device holds fl(x - pivot) = z (1 + d), |d| <= u (exact when x and the pivot are within a factor 2): a product is off by 2 u
        |z_i z_j|, a sum of z by u |z|: 2 u A_ij on S, u B_i on T_i.
      S_s: one fma chain of L terms, one rounding per term: L u A_ij(slab) (Higham, Thm 3.1 with fused products); the slabs are then added in NS - 1
        plain additions: NS u A_ij.  Together (L + NS + 2) u A_ij.
      T_i: L + NS additions: (L + NS + 1) u B_i with the shift.  T_i T_j / n is therefore off by (L + NS + 1) u (B_i |T_j| + B_j |T_i|) / n
        <= 2 (L + NS + 1) u B_i B_j / n; the double-double quotient adds O(u^2).
      (S - qh) - ql: two roundings of quantities no larger than A_ij + B_i B_j / n: 2 u of that.
    E_ij = 2 [(L + NS + 4) u A_ij + (2 (L + NS) + 4) u B_i B_j / n].
      mean_i = pivot_i + T_i / n: (L + NS + 1) u B_i / n from T, u |T_i / n| from the division, u |mean_i| from the last addition:
    Emean_i = 2 [(L + NS + 2) u B_i / n + u |mean_i|].
    The offset of the posterior enters the mean's bound through u |mean| only, and E not at all: z does not carry it."""
    ncols, N, D = hist.shape
    n = ncols * N
    ch = slab(N, D)
    L = ncols * min(ch, N)
    NS = -(-N // ch)
    z = np.abs(hist - hist[0, 0]).reshape(n, D)
    A = z.T @ z
    B = z.sum(axis=0)
    E = 2.0 * U * ((L + NS + 4) * A + (2 * (L + NS) + 4) * np.outer(B, B) / n)
    mean = hist.reshape(n, D).mean(axis=0)
    Emean = 2.0 * U * ((L + NS + 2) * B / n + np.abs(mean))
    return E, Emean


def bound_ranks(hist, bounds):
    """(E, Emean) for the chains cut into R shards and merged between the ranks.  Every shard carries its own bound()s E_r, Emean_r.
      mean: n_r mean_r is rounded once (u |n_r mean_r|), the R terms are added (R u of their absolute sum), the quotient is rounded: relative to
        the largest |mean_r| that is (R + 2) u, and a weighted mean of the shards' errors is no larger than the largest:
            Eg_i = max_r Emean_r,i + (R + 2) u max_r |mean_r,i|.
      d = mean_r - mean carries e_i = Emean_r,i + Eg_i + u |d_i|, so n_r d_i d_j is off by n_r (|d_i| e_j + |d_j| e_i + e_i e_j) and by 3 u of
        itself for its roundings; M_r + n_r d d' and the R additions add (R + 1) u of the terms' absolute sum.
    E_ij = 2 [sum_r E_r,ij + sum_r n_r (|d_i| e_j + |d_j| e_i + e_i e_j) + (R + 4) u sum_r (|M_r,ij| + n_r |d_i d_j|)].
    Here the offset does enter, through u |mean| in e — as in klara_gather_moments' merge."""
    ncols, N, D = hist.shape
    R = len(bounds) - 1
    shards = [np.ascontiguousarray(hist[:, c0:c1]) for c0, c1 in zip(bounds[:-1], bounds[1:])]
    bs = [bound(h) for h in shards]
    means = [h.reshape(-1, D).mean(axis=0) for h in shards]
    counts = [float(ncols * (c1 - c0)) for c0, c1 in zip(bounds[:-1], bounds[1:])]
    mean = sum(c * m for c, m in zip(counts, means)) / sum(counts)
    Eg = np.max([b[1] for b in bs], axis=0) + (R + 2) * U * np.max(np.abs(means), axis=0)
    E = np.zeros((D, D))
    for h, (Er, Emr), mr, nr in zip(shards, bs, means, counts):
        d = np.abs(mr - mean)
        e = Emr + Eg + U * d
        xc = h.reshape(-1, D) - mr
        Mr = np.abs(xc.T @ xc)
        E = E + Er + nr * (np.outer(d, e) + np.outer(e, d) + np.outer(e, e)) + (R + 4) * U * (Mr + nr * np.outer(d, d))
    return 2.0 * E, 2.0 * Eg


def errors(mean, M, ex, E, Emean):
    """largest |M - exact| / bound over the exact pairs and largest |mean - exact| / bound: both must be <= 1"""
    rm = max(abs(M[i, j] - v) / E[i, j] if E[i, j] > 0 else (0.0 if M[i, j] == v else np.inf) for (i, j), v in ex["M"].items())
    with np.errstate(all="ignore"):
        q = np.abs(mean - ex["mean"]) / Emean
    return rm, float(np.nanmax(np.where(Emean > 0, q, np.where(mean == ex["mean"], 0.0, np.inf))))


def bits_differ(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


# the shapes of the selftest cases (tests/test_gpu_cov.py runs them on the device, tests/test_cov_host.py holds the mirror to exact on the same inputs)
CHAINS = [1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 5]          # at D = 3, 200 saved steps
DIMS = [1, 2, 15, 16, 17, 32, 33, 100, 128, 129, 255, 256]      # at N = 37, 9 saved steps
SPLITS70 = {"32+32+6": [32, 32, 6], "1x70": [1] * 70, "7x10": [7] * 10}
N_SPLIT, D_SPLIT = 2 * CH + 5, 17


def splits_of(ncols):
    """the default feeding of a history: launches of 32 saved steps and the rest"""
    return [32] * (ncols // 32) + ([ncols % 32] if ncols % 32 else [])
