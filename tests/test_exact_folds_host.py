"""The exact folds of the unit-diagonal kernels (klara.jl_amd/csrc/klara_diagt.h), without a GPU.

On lt = -|x|^2 the gradient is -2.0 * x, an exact scaling.  The MALA kernels therefore form the proposal mean as x + (-h) * x in place of
x + (0.5 * h) * (-2.0 * x), and the HMC kernels kick with fma(-2.0 * kf, x, m) in place of fma(kf, -2.0 * x, m).  Both pairs compute one
real number and round it once, so they agree bit for bit — checked here over values of every magnitude (uint64 views, so that signed
zeros and NaN payloads count), in IEEE double arithmetic (NumPy: one rounding per operation, nothing fused) and, for the fma, in exact
rational arithmetic rounded once."""
import math
from fractions import Fraction

import numpy as np

STEPS = [0.9, 0.3, 1e-3, math.pi / 10.0]          # the headline's, the commit-path tests', a small one, one with a full mantissa


def _values(n, seed):
    """n doubles of every kind a state element or a gradient argument can be: normal magnitudes, subnormals, values of order
    1e+-300, both zeros and both infinities."""
    rng = np.random.default_rng(seed)
    k = n // 5
    sign = lambda m: np.where(rng.random(m) < 0.5, -1.0, 1.0)
    parts = [
        rng.standard_normal(k) * 3.0,                                                     # what a chain holds
        sign(k) * np.exp(rng.uniform(-40.0, 40.0, k)),                                    # many binades
        sign(k) * rng.integers(1, 2 ** 52, k).astype(np.float64) * 5e-324,                # subnormals (full and short mantissas)
        sign(k) * (1.0 + rng.random(k)) * 10.0 ** rng.uniform(299.0, 300.9, k),           # ~1e300: -2 x stays finite
        sign(k) * (1.0 + rng.random(k)) * 10.0 ** rng.uniform(-300.9, -299.0, k),         # ~1e-300: products go subnormal
        np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0]),
    ]
    return np.concatenate(parts)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_mala_mean_fold_is_bit_exact():
    """halfh * (-2 x) has the bits of (-h) * x, and x + halfh * (-2 x) the bits of x + (-h) * x (MALA.jl:83 and :91 on the unit diagonal):
    1e5 values x 4 steps, every element compared."""
    x = _values(100_000, seed=11)
    assert x.size >= 100_000 and np.isinf(x).any() and (np.abs(x[x != 0.0]) < 2.3e-308).any()
    with np.errstate(all="ignore"):                   # (inf - inf = nan in the sums of the infinite elements: both forms give it)
        for h in STEPS:
            h = np.float64(h)
            halfh = np.float64(0.5) * h
            assert float(halfh) * 2.0 == float(h)                                  # the precondition: 0.5 * h is exact
            g = np.float64(-2.0) * x                                               # the gradient the oracle forms
            a, b = halfh * g, (-h) * x
            assert np.array_equal(_bits(a), _bits(b)), f"h = {h}: products differ at {np.flatnonzero(_bits(a) != _bits(b))[:5]}"
            sa, sb = x + a, x + b
            assert np.array_equal(_bits(sa), _bits(sb)), f"h = {h}: means differ"


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic; float() of a Fraction rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_hmc_kick_fold_is_bit_exact():
    """fma(kf, -2 x, m) has the bits of fma(-2 kf, x, m) for kf = eps (a full kick) and kf = 0.5 * eps (a half kick, where -2 kf = -eps:
    the opening update), in exact arithmetic rounded once.  Finite values only (a Fraction has no infinity); -2.0 * x and -2.0 * kf are
    the floating-point products the kernels form."""
    x = _values(4_000, seed=12)
    x = x[np.isfinite(x)]
    rng = np.random.default_rng(13)
    m = np.concatenate([rng.standard_normal(x.size - 6), [0.0, -0.0, 5e-324, -1e300, 1e-300, 1.0]])
    n = 0
    for eps in STEPS + [0.1]:
        halfe = 0.5 * eps
        assert halfe * 2.0 == eps and -2.0 * halfe == -eps
        for kf in (eps, halfe):
            nkf2 = -2.0 * kf
            for xe, me in zip(x.tolist(), m.tolist()):
                ref = _fma(kf, -2.0 * xe, me)
                got = _fma(nkf2, xe, me)
                assert np.float64(ref).view(np.uint64) == np.float64(got).view(np.uint64), (eps, kf, xe, me)
                n += 1
    assert n >= 30_000
