"""References for the across-chain reductions (klara_monitors.hip: k_pool_stage1 / k_pool_stage2 behind klara_get_pooled_summaries, k_moments_stage1 /
k_moments_stage2 with chan_merge behind klara_gather_moments; klara_comm.hip: k_scale / k_merge_between, the rank-local steps of the one between-rank merge, klara_merge.h merge_ranks, that the gather calls and the
simulated-rank self tests both run).

  chain_view(inp)                 every chain's sums as the device views them: part + held * x in two f64 operations (what klara_get_chain_sums returns)
  exact(inp, cols)                pooled S, Q, mean = S / n, M2 = Q - S^2 / n, the accept total and the smallest per-chain q_c - s_c^2 / nsaved from those doubles
                                  in exact integer arithmetic (every double is a dyadic rational; nothing is rounded before the final conversion)
  mirror(inp)                     NumPy restatement of the kernels' order of operations: stage 1 over c = b, b + nb, ..., the double-double q - s^2 / n, the clamp
                                  at 0, chan_merge as written in the kernel, stage 2's per-thread ascending merge with its `chains` count, the 256-wide tree; the
                                  plain-sum analogues for the summaries
  mirror_ranks(inp, bounds)       mirror() of every shard, then the between-rank merge with the all-reduces as sums over the ranks in ascending order from 0
  bound(N, ex, ranks)             derived worst-case bound on the error of the device's order of operations against exact (see its docstring)
and the inputs the CPU and GPU tests share (make_inputs, clamp_inputs).  CPU only.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

POOL_BLOCKS = 1024         # KLARA_POOL_BLOCKS
THREADS = 256              # workgroup size of every kernel here
U = 2.0 ** -53
CAP = 1e-7                 # hard cap on bound()'s relative M2 bound: inputs whose bound exceeds it may not be used (1e6 sd at 3,077 chains: 3.7e-8)
GRID = 2.0 ** -4           # the synthetic series live on this dyadic grid
SD = 1.25                  # their innovation scale; an offset of k sd adds k * SD
OFFSETS = (0.0, 242.0, 1e4, 1e6)
MARGIN = 1.0               # every chain of make_inputs has its exact M2 above this — or exactly 0 (a chain that never moved: held = nsaved, exact sums)
MARGIN_200 = 100.0         # ... and above this from nsaved = 200 on


# ---------------------------------------------------------------- inputs
def make_inputs(N, D, nsaved, offset=0.0, seed=0):
    """Per-chain running sums of N x D series of nsaved samples offset * SD + SD z on GRID, as a job leaves them: sum / sumsq hold the samples already
    folded in (sumsq added in sample order in f64), the last `held` samples sit at the current state X (sojourn form).  Chains c % 3 == 1 get
    held = 1, 7, nsaved in turn (cut to nsaved); a chain with held = nsaved never moved: its state lies on a grid of 1/2, so that nsaved x and nsaved x^2
    are exact and its M2 is exactly 0.  The first and the last sample of every other chain are at least 2 SD apart, so that its M2 is at least
    2 SD^2 > MARGIN whatever nsaved >= 2 is.  Accept counters: below 2^20, every fifth chain just below 2^40."""
    rng = np.random.default_rng([20261019, seed, N, D, nsaved])
    base = float(offset) * SD
    assert base / GRID == round(base / GRID) and nsaved >= 0
    ns = int(nsaved)
    x = base + np.rint(SD * rng.standard_normal((ns, N, D)) / GRID) * GRID
    if ns >= 2:
        d = x[ns - 1] - x[0]
        x[ns - 1] = np.where(np.abs(d) < 2 * SD, x[0] + np.where(d < 0, -2 * SD, 2 * SD), x[ns - 1])
    held = np.zeros(N, dtype=np.int64)
    c = np.arange(N)
    sel = c % 3 == 1
    held[sel] = np.minimum(np.array([1, 7, max(ns, 1)])[(c[sel] // 3) % 3], ns)
    X = x[ns - 1].copy() if ns else base + np.rint(SD * rng.standard_normal((N, D)) / GRID) * GRID
    still = (held == ns) & (ns > 0)
    X[still] = base + np.rint(SD * rng.standard_normal((int(still.sum()), D)) * 2) / 2
    if ns:
        t = np.arange(ns)[:, None]
        tail = t >= ns - held[None, :]                                       # (ns, N): the samples that sit at the current state
        x = np.where(tail[:, :, None], X[None], x)
        part = np.where(tail[:, :, None], 0.0, x)
        s = part.sum(axis=0)                                                 # exact: grid values, |sum| < 2^53 GRID
        q = np.cumsum(part * part, axis=0)[-1]
        assert np.array_equal(np.cumsum(part, axis=0)[-1], s)
    else:
        s = np.zeros((N, D)); q = np.zeros((N, D))
    nacc = rng.integers(0, 2 ** 20, N).astype(np.uint64)
    nacc[::5] = np.uint64(2 ** 40) - nacc[::5] - np.uint64(1)
    return {"sum": np.ascontiguousarray(s), "sumsq": np.ascontiguousarray(q), "X": np.ascontiguousarray(X), "held": held, "naccept": nacc, "nsaved": ns}


def clamp_inputs(N, D, offset=0.0, seed=0):
    """nsaved = 1, deliberately at the clamp: one full-mantissa sample x per chain, sum = x, sumsq = fl(x x), so that q - s^2 is minus the rounding error
    of the square and has either sign.  The expected value there is the mirror's."""
    rng = np.random.default_rng([20261020, seed, N, D])
    x = float(offset) * SD + SD * rng.standard_normal((N, D))
    nacc = rng.integers(0, 2 ** 20, N).astype(np.uint64)
    return {"sum": x.copy(), "sumsq": x * x, "X": x.copy(), "held": np.zeros(N, dtype=np.int64), "naccept": nacc, "nsaved": 1}


def slice_inputs(inp, c0, c1):
    out = {k: (v[c0:c1] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    return out


def chain_view(inp):
    """(s, q): sum + held x and sumsq + held (x x), each in two f64 operations, where held > 0 (k_sum_view, k_pool_stage1, k_moments_stage1)."""
    h = inp["held"].astype(np.float64)[:, None]
    x = inp["X"]
    s = np.where(h > 0, inp["sum"] + h * x, inp["sum"])
    q = np.where(h > 0, inp["sumsq"] + h * (x * x), inp["sumsq"])
    return s, q


# ---------------------------------------------------------------- exact
def _scaled_ints(v):
    pairs = [float(a).as_integer_ratio() for a in v]
    den = max(d for _, d in pairs)
    return [p * (den // d) for p, d in pairs], den


def exact(inp, cols=None):
    """Exact pooled quantities of the columns `cols` (all by default) from the chains' sums as the device views them (chain_view).  Dict of arrays over
    the columns, each the correctly rounded exact rational: S, Q, mean = S / n, M2 = Q - S^2 / n with n = nsaved N (zeros for n = 0), min_chain_m2 (smallest
    q_c - s_c^2 / nsaved), min_chain_m2_pos (smallest one that is not exactly 0), clamped (minus the sum of the negative ones: what a clamp at 0 adds), sd = sqrt(M2 / n), max_abs_mean and spread of the chains' means; and
    n and accept (int)."""
    s, q = chain_view(inp)
    N, D = s.shape
    ns = int(inp["nsaved"])
    cols = list(range(D)) if cols is None else list(cols)
    n = ns * N
    out = {k: np.zeros(len(cols)) for k in ("S", "Q", "mean", "M2", "min_chain_m2", "min_chain_m2_pos", "clamped", "sd", "max_abs_mean", "spread")}
    for i, j in enumerate(cols):
        si, sden = _scaled_ints(s[:, j]); qi, qden = _scaled_ints(q[:, j])
        S = Fraction(sum(si), sden); Q = Fraction(sum(qi), qden)
        out["S"][i] = float(S); out["Q"][i] = float(Q)
        if n > 0:
            out["mean"][i] = float(S / n)
            m2 = Q - S * S / n
            out["M2"][i] = float(m2)
            out["sd"][i] = math.sqrt(max(float(m2 / n), 0.0))
            # q_c - s_c^2 / ns = (q_c sden^2 ns - s_c^2 qden) / (qden sden^2 ns): integers over one denominator
            per = [a * sden * sden * ns - b * b * qden for a, b in zip(qi, si)]
            den = qden * sden * sden * ns
            out["min_chain_m2"][i] = float(Fraction(min(per), den))
            out["clamped"][i] = float(Fraction(-sum(p for p in per if p < 0), den))
            pos = [p for p in per if p != 0]
            out["min_chain_m2_pos"][i] = float(Fraction(min(pos), den)) if pos else math.inf
            means = s[:, j] / ns
            out["max_abs_mean"][i] = np.abs(means).max(); out["spread"][i] = means.max() - means.min()
    out["n"] = n
    out["accept"] = sum(int(a) for a in inp["naccept"])
    out["cols"] = cols
    return out


# ---------------------------------------------------------------- mirror
def two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; as klara_jl_amd.distributed._two_prod)."""
    p = a * b

    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a); bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_square_error(s, p):
    """fma(s, s, -p) for p = fl(s s): the rounding error of the square, exactly representable."""
    p2, e = two_prod(s, s)
    return e


def fma_remainder(qh, n, p):
    """fma(-qh, n, p) for qh = fl(p / n): the division's remainder p - qh n, exactly representable; qh n = t + te exactly, p - t is exact (t is within an
    ulp of p) and so is the rest."""
    t, te = two_prod(qh, np.full_like(qh, n))
    return (p - t) - te


def chain_moments(s, q, ns):
    """(mean_c, M2_c) of every chain and dimension as k_moments_stage1 forms them: q - s^2 / ns in double-double, clamped at 0."""
    with np.errstate(all="ignore"):
        p = s * s
        pe = fma_square_error(s, p)
        qh = p / ns
        r = fma_remainder(qh, ns, p)
        ql = (r + pe) / ns
        m2 = (q - qh) - ql
        m2 = np.where(m2 < 0.0, 0.0, m2)
        return s / ns, m2


def chan_merge(n, mean, m2, nb, meanb, m2b):
    """chan_merge of klara_monitors.hip on arrays (n, nb broadcast against mean / m2): where n + nb > 0, and unchanged elsewhere."""
    nt = n + nb
    ok = nt > 0.0
    with np.errstate(all="ignore"):
        delta = meanb - mean
        w = nb / nt
        mean2 = mean + delta * w
        m22 = (m2 + m2b) + (delta * delta) * (n * w)
    return np.where(ok, nt, n), np.where(ok, mean2, mean), np.where(ok, m22, m2)


def _nb(N):
    return min(int(N), POOL_BLOCKS)


def mirror_summaries(inp):
    """(sum[D], sumsq[D], accept total) as k_pool_stage1 / k_pool_stage2 add them: block b adds the chains b, b + nb, ... from 0.0; thread t adds the
    partials t, t + 256, ... from 0.0; a tree over the 256 threads.  The accept counters are u64: their sum mod 2^64 does not depend on the order."""
    s, q = chain_view(inp)
    N, D = s.shape
    nb = _nb(N)
    v = np.concatenate([s, q], axis=1)
    part = np.zeros((nb, 2 * D))
    for k in range((N + nb - 1) // nb):
        rows = v[k * nb:(k + 1) * nb]
        part[:rows.shape[0]] = part[:rows.shape[0]] + rows
    th = np.zeros((THREADS, 2 * D))
    for k in range((nb + THREADS - 1) // THREADS):
        rows = part[k * THREADS:(k + 1) * THREADS]
        th[:rows.shape[0]] = th[:rows.shape[0]] + rows
    m = THREADS // 2
    while m > 0:
        th[:m] = th[:m] + th[m:2 * m]
        m >>= 1
    acc = int(np.sum(inp["naccept"].astype(object))) % 2 ** 64
    return th[0, :D].copy(), th[0, D:].copy(), acc


def mirror(inp):
    """(mean[D], M2[D]) as k_moments_stage1 / k_moments_stage2 form them."""
    s, q = chain_view(inp)
    N, D = s.shape
    ns = float(inp["nsaved"])
    nb = _nb(N)
    mc, m2c = chain_moments(s, q, ns)
    # stage 1: block b merges its chains c = b, b + nb, ... in ascending order into (0, 0, 0)
    n = np.zeros((nb, 1)); mean = np.zeros((nb, D)); m2 = np.zeros((nb, D))
    for k in range((N + nb - 1) // nb):
        a = min(nb, N - k * nb)
        n[:a], mean[:a], m2[:a] = chan_merge(n[:a], mean[:a], m2[:a], ns, mc[k * nb:k * nb + a], m2c[k * nb:k * nb + a])
    # stage 2: thread t merges the partials b = t, t + 256, ... with the count nsaved * chains(b); then the tree
    b = np.arange(nb)
    chains = (N - b + nb - 1) // nb                                          # chains c = b, b + nb, ... < N
    cnt = (ns * chains.astype(np.float64))[:, None]
    tn = np.zeros((THREADS, 1)); tm = np.zeros((THREADS, D)); tq = np.zeros((THREADS, D))
    for k in range((nb + THREADS - 1) // THREADS):
        a = min(THREADS, nb - k * THREADS)
        sl = slice(k * THREADS, k * THREADS + a)
        tn[:a], tm[:a], tq[:a] = chan_merge(tn[:a], tm[:a], tq[:a], cnt[sl], mean[sl], m2[sl])
    m = THREADS // 2
    while m > 0:
        tn[:m], tm[:m], tq[:m] = chan_merge(tn[:m], tm[:m], tq[:m], tn[m:2 * m], tm[m:2 * m], tq[m:2 * m])
        m >>= 1
    return tm[0].copy(), tq[0].copy()


def between_ranks(means, m2s, counts):
    """The between-rank merge of klara_gather_moments from every rank's (mean_r, M2_r, n_r): n_r mean_r summed over the ranks (ascending, from 0.0),
    mean = that / sum n_r (0 when there is no sample), M2 = sum over the ranks of M2_r + n_r (mean_r - mean)^2.  Returns (mean, M2, n)."""
    D = means[0].shape[0]
    wsum = np.zeros(D)
    ntot = 0
    for mr, nr in zip(means, counts):
        wsum = wsum + float(nr) * mr                                         # k_scale
        ntot += int(nr)
    nt = float(ntot)
    with np.errstate(all="ignore"):
        mean = wsum / nt if nt > 0.0 else np.zeros(D)
        m2 = np.zeros(D)
        for mr, qr, nr in zip(means, m2s, counts):
            d = mr - mean
            m2 = m2 + (qr + float(nr) * (d * d))   # k_merge_between (the diagonal form)
    return mean, m2, ntot


def mirror_ranks(inp, bounds):
    """(mean[D], M2[D], counters (accept total, saved samples, chains)) of the chains cut into the shards [bounds[r], bounds[r + 1])."""
    assert bounds[0] == 0 and bounds[-1] == inp["sum"].shape[0] and all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
    means, m2s, counts = [], [], []
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        mr, qr = mirror(slice_inputs(inp, c0, c1))
        means.append(mr); m2s.append(qr); counts.append(int(inp["nsaved"]) * (c1 - c0))
    mean, m2, ntot = between_ranks(means, m2s, counts)
    return mean, m2, (sum(int(a) for a in inp["naccept"]) % 2 ** 64, ntot, int(bounds[-1]))


def shard_bounds(N, R):
    """the boundaries of klara_jl_amd.shard_chains(N, r, R)"""
    base, rem = divmod(N, R)
    out = [0]
    for r in range(R):
        out.append(out[-1] + base + (1 if r < rem else 0))
    return out


def splits(N):
    """R -> shard boundaries of the rank tests: the shard_chains split for R = 1, 2, 3, 5 and unequal ones (1 | N - 1; N - 1 | 1; 1 | 1 | N - 2)."""
    return {"1": [0, N], "2": shard_bounds(N, 2), "3": shard_bounds(N, 3), "5": shard_bounds(N, 5), "1|N-1": [0, 1, N], "N-1|1": [0, N - 1, N],
            "1|1|N-2": [0, 1, 2, N], "1025|rest": [0, min(1025, N - 1), N]}


# ---------------------------------------------------------------- bound
def merge_depth(N):
    """sequential merges on the longest path: ceil(N / 1024) in stage 1, ceil(nb / 256) per thread in stage 2, 8 levels of the tree"""
    nb = _nb(N)
    return -(-int(N) // POOL_BLOCKS) + -(-nb // THREADS) + 8


def bound(N, ex, ranks=1):
    """(relative bound on |M2 - exact M2| / exact M2, absolute bound on |mean - exact mean|) per column of exact()'s result `ex`, for the device's order of
    operations on N chains (`ranks` > 1: cut into that many shards and merged between the ranks).  First order in u = 2^-53, doubled for the rest.

    Notation: L = merge_depth(N) (+ 2 for the between-rank step), M = max |mean_c| over the chains, spread = max mean_c - min mean_c, sd = sqrt(M2 / n),
    n = nsaved N.  The chains' sums s_c, q_c are the inputs: exact doubles.
      per chain: mean_c = fl(s / nsaved) is off by u M.  M2_c = (q - qh) - ql with s^2 / nsaved = qh + ql (1 + 2u) + O(u^2 s^2 / nsaved): q - qh is exact
        or rounded once, the second subtraction once: 3 u M2_c + 4 u^2 s^2 / nsaved, and summed over the chains 3 u M2 + 4 u^2 n M^2.
      means: one merge forms mean + delta w from (mean, mean_b) carrying errors (e, e_b): (1 - w) e + w e_b — an average, no growth — plus the roundings
        of delta, w and the product, 3 u |delta| w <= 3 u spread, and of the sum, u M.  Over a path of L merges:
            E = (L + 1) u (M + 3 spread)                                              [the absolute bound on the mean]
      between terms: delta is computed from two such means, off by e_d = 2 E + u spread, so delta^2 n w is off by (2 |delta| e_d + e_d^2) n w, plus 4 u of
        itself for its four roundings.  Exactly, sum over all merges of delta^2 n w = M2 - sum_c M2_c <= M2 (Chan), and the weights n w = n n_b / (n + n_b)
        <= min(n, n_b) add up to at most n in stage 1 (one chain at a time), n in stage 2's sequential part and n / 2 per tree level: W <= 6 n.  By
        Cauchy-Schwarz  sum 2 |delta| e_d n w <= 2 e_d sqrt(W) sqrt(M2), so relative to M2 = n sd^2:
            2 sqrt(6) e_d / sd + 6 (e_d / sd)^2
      sums: every M2 passes at most L merges of two additions each: 2 L u, relative (all terms are non-negative).
      clamp: sums with q_c < s_c^2 / nsaved (no series has them; clamp_inputs makes them) have a negative exact M2_c that the device sets to 0: ex["clamped"]
        in all, an error of the input that the bound carries as it is.
    Together:  rel = (2 L + 8) u + 4 u^2 (M / sd)^2 + 2 sqrt(6) e_d / sd + 6 (e_d / sd)^2 + clamped / M2, returned doubled.  nsaved enters through n only: it cancels.
    At |mean| / sd = k and L = 16 (3,077 chains) this is about 330 k u: 1e-11 at 242 sd, 3.7e-10 at 1e4, 3.7e-8 at 1e6 — the mean's u |mean| rounding carried into
    delta^2, the one place where the offset enters.  Merging about a per-chain pivot would remove it.

    Largest |mirror - exact| / bound on the inputs of tests/test_pooled_host.py (CPU, N in {1 ... 3077}, D = 3, nsaved = 200; measured, not fitted) —
    M2: 0.021 at 0 sd, 3.0e-4 at 242, 2.7e-4 at 1e4, 8.1e-4 at 1e6 (the roundings of the means do not line up as the worst case has them: the errors
    themselves are 3.6e-16, 1.8e-15, 6.5e-14 and 1.9e-11); mean: 0.018, 0.077, 0.060, 0.076.  MEASURED below holds the same figures."""
    if ex["n"] == 0:                                                         # no saved sample: zeros, exactly
        return np.zeros_like(ex["M2"]), np.zeros_like(ex["M2"])
    L = merge_depth(N) + (2 if ranks > 1 else 0)
    M, spread, sd = ex["max_abs_mean"], ex["spread"], ex["sd"]
    E = (L + 1) * U * (M + 3.0 * spread)
    ed = 2.0 * E + U * spread
    with np.errstate(all="ignore"):
        rel = (2 * L + 8) * U + 4.0 * U * U * (M / sd) ** 2 + 2.0 * math.sqrt(6.0) * ed / sd + 6.0 * (ed / sd) ** 2 + ex["clamped"] / ex["M2"]
    return 2.0 * rel, 2.0 * E


# largest observed (|mirror M2 - exact M2| / exact M2) / bound and |mirror mean - exact mean| / bound per offset (sd), over the shapes of
# tests/test_pooled_host.py; worst relative M2 error itself in the third place.  Filled in from the CPU run, not from the device.
MEASURED = {0.0: (0.0206, 0.0180, 3.58e-16), 242.0: (0.000302, 0.0767, 1.82e-15), 1e4: (0.000274, 0.0596, 6.55e-14), 1e6: (0.000808, 0.0763, 1.9e-11)}
