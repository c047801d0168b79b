"""The rejection screen of the 4-lane MALA table kernel (klara.jl_amd/csrc/klara_mala_screen.h), without a GPU.

The kernel draws a transition's normals, adds up sum x z and sum z^2 and asks the screen whether the accept test certainly fails; only a wavefront
with a chain that may accept runs the literal arithmetic of MALA.jl:83-92.  tests/mala_screen_ref.c is compiled against the header (gcc,
-ffp-contract=off) and called through ctypes; the reference is a NumPy restatement of the literal ratio in the kernel's operation order (two
partial sums per lane, the butterfly over four lanes, the sum of the partials).

(a) soundness: "certain" implies that the literal test rejects — stationary draws, other steps, scaled states, zeros and subnormals, a log-target at
    odds with the state, both ends of log u, near-ties; NaN / infinite inputs are never certain.
(b) sharpness: at the stationary h = 0.9 inputs at most 1 in 10^4 literal rejections stays undecided (derived: the undecided window is
    2 x 2^-30 T ~ 1e-6 wide against a ratio density under 0.05 per unit, ~1e-7).
(c) the proven error bound: |est - ratio| / T < 2^-44 over every finite input of (a).
(d) the same soundness check as a program of its own under AddressSanitizer and UBSan (nothing loaded into python is sanitized)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_ffi as O

ROOT = Path(__file__).resolve().parent.parent
SRC = Path(__file__).resolve().parent / "mala_screen_ref.c"
INC = ["-I", str(ROOT / "klara.jl_amd" / "csrc"), "-I", str(ROOT / "include")]
HDRS = [O.CSRC / "klara_mala_screen.h", O.CSRC / "detmath.h", O.CSRC / "detmath_tables.h"]
GUARD = -31.2                                   # KD_LOG_UMIN_GUARD: layouts without a padding pair (D = 103, 104) have no accept draw in hand
LG_HI, LG_LO = float(np.log1p(-2.0 ** -45)), float(np.log(2.0 ** -45))
H_MIN, H_MAX = 2.0 ** -6, 2.0                   # the step range the bound is proven for
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    so = O.build_c("mala_screen_ref", ["-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared", *INC], sources=[SRC], hashed=HDRS)
    lb = C.CDLL(str(so))
    lb.ms_consts.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p]
    lb.ms_consts.restype = C.c_int
    lb.ms_screen.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_double,
                             C.c_void_p, C.c_void_p, C.c_void_p]
    lb.ms_screen.restype = C.c_int
    lb.ms_literal.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lb.ms_literal.restype = None
    return lb


def consts(h):
    """the kernel's launch constants: sqrt_step0 and 0.5 * inv_step0 (klara_create.hip)"""
    h = np.float64(h)
    return float(h), float(np.sqrt(h)), float(np.float64(0.5) * (np.float64(1.0) / h))


def literal_ratio(x, z, lt, gconst, h):
    """MALA.jl:83-92 on lt = gconst - sum x^2 as k_diagt<MALA, 13, 4, .., UNITW> evaluates it: element 2 (4 p + q) + j in lane q, pair p; per lane
    one partial sum over the even pairs and one over the odd ones, each in ascending order; (l0 + l1) + (l2 + l3) over the lanes; even + odd."""
    h, s, c = consts(h)
    n, d = x.shape
    xs, zs = np.zeros((n, 104)), np.zeros((n, 104))
    xs[:, :d], zs[:, :d] = x, z
    xs, zs = xs.reshape(n, 13, 4, 2), zs.reshape(n, 13, 4, 2)
    neg_h = -h
    red = np.zeros((3, 2, n, 4))
    with np.errstate(all="ignore"):
        for p in range(13):
            for j in range(2):
                xv, zv = xs[:, p, :, j], zs[:, p, :, j]
                m = xv + neg_h * xv
                xe = m + s * zv
                r = p & 1
                red[0, r] = red[0, r] + xe * xe
                q1 = m - xe
                red[1, r] = red[1, r] + (q1 * q1) * c
                mup = xe + neg_h * xe
                q2 = mup - xv
                red[2, r] = red[2, r] + (q2 * q2) * c
        part = (red[..., 0] + red[..., 1]) + (red[..., 2] + red[..., 3])
        tot = part[:, 0] + part[:, 1]
        ltp = gconst - tot[0]
        ratio = ltp - lt
        ratio = ratio + tot[1]
        ratio = ratio - tot[2]
    return ratio


def kernel_lt(x, gconst=0.0):
    """gconst - sum x^2 in the same order (what a chain's log-target holds after an accepted transition)"""
    n, d = x.shape
    xs = np.zeros((n, 104))
    xs[:, :d] = x
    xs = xs.reshape(n, 13, 4, 2)
    red = np.zeros((2, n, 4))
    for p in range(13):
        for j in range(2):
            red[p & 1] = red[p & 1] + xs[:, p, :, j] * xs[:, p, :, j]
    part = (red[..., 0] + red[..., 1]) + (red[..., 2] + red[..., 3])
    return gconst - (part[0] + part[1])


def screen(lib, x, z, lt, gconst, lg, h):
    h, s, c = consts(h)
    x, z, lt, lg = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, z, lt, lg))
    n, d = x.shape
    certain, est, T = np.zeros(n, dtype=np.int32), np.empty(n), np.empty(n)
    on = lib.ms_screen(n, d, x.ctypes.data, z.ctypes.data, lt.ctypes.data, gconst, lg.ctypes.data, h, s, c, certain.ctypes.data, est.ctypes.data, T.ctypes.data)
    return bool(on), certain.astype(bool), est, T


class Tally:
    """what (a), (b) and (c) hold the screen to, over every batch it is shown"""
    def __init__(self):
        self.n = self.rejected = self.certain = self.undecided = 0
        self.worst = 0.0

    def check(self, lib, x, z, lt, gconst, lg, h, what, expect_on=True):
        on, certain, est, T = screen(lib, x, z, lt, gconst, lg, h)
        assert on == expect_on, f"{what}: the launch flag is {on}"
        ratio = literal_ratio(x, z, lt, gconst, h)
        with np.errstate(invalid="ignore"):
            accepts = (ratio > 0.0) | (ratio > lg)           # (no draw in hand: lg is the guard, above which the kernel draws and may accept)
        wrong = certain & accepts
        assert not wrong.any(), f"{what}: {int(wrong.sum())} certain rejections that the literal test accepts, the first at {int(np.argmax(wrong))}"
        if not on:
            assert not certain.any(), f"{what}: the screen is off and answered"
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(ratio) & (T <= 2.0 ** 1000) & np.isfinite(est)          # (the bound is claimed up to T = 2^1000)
        if fin.any() and on:
            with np.errstate(all="ignore"):
                rel = np.abs(est[fin] - ratio[fin]) / T[fin]
            self.worst = max(self.worst, float(rel.max()))
            assert rel.max() < 2.0 ** -44, f"{what}: |est - ratio| / T reaches 2^{np.log2(rel.max()):.1f}"
        self.n += len(lt); self.rejected += int((~accepts).sum()); self.certain += int(certain.sum()); self.undecided += int((~accepts & ~certain).sum())
        return certain, ratio, est, T


def stationary(rng, n, d):
    return rng.standard_normal((n, d)) * np.sqrt(0.5), rng.standard_normal((n, d))


def log_u(rng, n, d):
    return np.full(n, GUARD) if d >= 103 else np.log(rng.random(n))


def test_launch_flag_and_proof_coefficients(lib):
    out = np.empty(5)
    hs = np.concatenate([np.geomspace(H_MIN, H_MAX, 20001), [H_MIN, H_MAX, 1.0, 0.9, 0.3, 0.02, 1.5]])
    hs = np.clip(hs, H_MIN, H_MAX)
    for h in hs:                                            # the proof's numeric condition (E0 <= 96 T0, E2 <= 96 T2) holds on the whole range
        assert lib.ms_consts(*consts(h), out.ctypes.data) == 1, f"the screen is off at h = {h!r}"
        assert np.isfinite(out).all() and out[3] >= 0.25 and out[4] >= 0.25 and out[0] < 0 and out[2] < 0
    sub = 5e-324
    with np.errstate(all="ignore"):
        for h in (0.0, -0.9, sub, 2.0 ** -1030, np.nan, np.inf, np.nextafter(H_MIN, 0.0), np.nextafter(H_MAX, 4.0), 0.01, 2.5, 1e-9, 40.0):
            assert lib.ms_consts(*consts(h), out.ctypes.data) == 0, f"the screen is on at h = {h!r}"
    h, s, c = consts(0.9)                                   # constants that are not this step's sqrt and 0.5 / h
    assert lib.ms_consts(h, s * (1 + 2.0 ** -40), c, out.ctypes.data) == 0 and lib.ms_consts(h, s, c * (1 - 2.0 ** -40), out.ctypes.data) == 0
    assert lib.ms_consts(h, np.nan, c, out.ctypes.data) == 0 and lib.ms_consts(h, s, np.inf, out.ctypes.data) == 0


def test_c_restatement_equals_the_numpy_one(lib):
    """the stand-alone program's own literal ratio (ms_literal_ratio) is the NumPy reference bit for bit"""
    rng = np.random.default_rng(20261020)
    for d in (97, 100, 103, 104):
        for h in (0.9, 0.3, 0.02, 1.5):
            x, z = stationary(rng, 500, d)
            lt = kernel_lt(x, -1.5)
            got = np.empty(500)
            hh, s, c = consts(h)
            lib.ms_literal(500, d, x.ctypes.data, z.ctypes.data, lt.ctypes.data, -1.5, hh, s, c, got.ctypes.data)
            assert np.array_equal(got.view(np.uint64), literal_ratio(x, z, lt, -1.5, h).view(np.uint64))


def test_soundness_sharpness_and_error_bound(lib):
    rng = np.random.default_rng(20261020)
    # stationary draws at the headline step: (a), and what (b) is counted on
    head = Tally()
    for d in (97, 100, 104):
        for _ in range(5):
            x, z = stationary(rng, 200_000, d)
            head.check(lib, x, z, kernel_lt(x), 0.0, log_u(rng, len(x), d), 0.9, f"stationary d{d} h0.9")
    print(f"h 0.9: {head.n} draws, {head.rejected} literal rejections, {head.certain} certain, {head.undecided} undecided, "
          f"|est - ratio| / T at most 2^{np.log2(max(head.worst, 1e-300)):.1f}")
    # (d = 104 has no accept draw in hand: a rejection the screen can know of is a ratio at or below the guard, about 3 % of its draws)
    assert head.n >= 3_000_000 and head.rejected > 1_960_000
    assert head.undecided * 10_000 <= head.rejected, f"(b) {head.undecided} of {head.rejected} literal rejections undecided"
    rest = Tally()
    for h in (0.3, 0.02, 1.5, H_MIN, H_MAX, 1.0):
        for d in (97, 100, 104):
            x, z = stationary(rng, 70_000, d)
            rest.check(lib, x, z, kernel_lt(x, -2.75), -2.75, log_u(rng, len(x), d), h, f"stationary d{d} h{h}")
    assert rest.n >= 3 * 200_000 and 0 < rest.certain
    # a step outside the proven range: the screen is off
    for h in (0.01, 2.5):
        x, z = stationary(rng, 2_000, 100)
        rest.check(lib, x, z, kernel_lt(x), 0.0, log_u(rng, 2_000, 100), h, f"h{h}", expect_on=False)
    # scaled states: |x| up to where T passes 2^1000 and beyond it (sum x^2 overflows), down to subnormal and zero; lt formed from the scaled x
    n = 4_000
    for d in (100, 104):
        for k in (30, 100, 300, 480, 494, 497, 500, 505, 512, 600, -30, -100, -300, -500, -537, -600, -1000, -1060, -1074, -1080):
            x, z = stationary(rng, n, d)
            with np.errstate(all="ignore"):
                x = np.ldexp(x, k)
                lt = kernel_lt(x)
                certain, ratio, est, T = rest.check(lib, x, z, lt, 0.0, log_u(rng, n, d), 0.9, f"x scaled by 2^{k}, d{d}")
            if k >= 497:
                assert not certain.any(), f"x scaled by 2^{k}: T is above 2^1000 or not finite, and the screen answered"
    # zeros and subnormals among the elements; every element zero
    for d in (97, 100, 104):
        x, z = stationary(rng, 20_000, d)
        x[rng.random(x.shape) < 0.3] = 0.0
        x[rng.random(x.shape) < 0.2] = 2.0 ** -1070
        z[rng.random(z.shape) < 0.05] = 0.0
        x[:50] = 0.0
        z[50:60] = 0.0
        rest.check(lib, x, z, kernel_lt(x), 0.0, log_u(rng, len(x), d), 0.9, f"zeros and subnormals d{d}")
    # a log-target at odds with the state (the caller may set it)
    for d in (100, 104):
        for h in (0.9, 0.3):
            x, z = stationary(rng, 50_000, d)
            lt = np.concatenate([rng.standard_normal(25_000) * 30.0, kernel_lt(x[25_000:]) + rng.standard_normal(25_000) * 3.0])
            rest.check(lib, x, z, lt, 0.0, log_u(rng, len(x), d), h, f"inconsistent lt d{d} h{h}")
    # both ends of log u
    for lg_end in (LG_HI, LG_LO):
        for h in (0.9, 0.3, 0.02):
            x, z = stationary(rng, 50_000, 100)
            rest.check(lib, x, z, kernel_lt(x), 0.0, np.full(len(x), lg_end), h, f"log u = {lg_end} h{h}")
    # NaN / infinity in x, z and lt, lt = -inf: never certain
    for d in (100, 104):
        x, z = stationary(rng, 6_000, d)
        z *= 3.0                                            # (a long jump: without the poison every one of these is certain)
        lt = kernel_lt(x)
        rows = np.arange(6_000)
        col = rng.integers(0, d, 6_000)
        x[rows[:1000], col[:1000]] = np.nan
        x[rows[1000:2000], col[1000:2000]] = np.where(rng.random(1000) < 0.5, np.inf, -np.inf)
        z[rows[2000:3000], col[2000:3000]] = np.nan
        z[rows[3000:4000], col[3000:4000]] = np.where(rng.random(1000) < 0.5, np.inf, -np.inf)
        lt[4000:4500] = np.nan; lt[4500:5000] = -np.inf; lt[5000:5500] = np.inf
        certain, *_ = rest.check(lib, x, z, lt, 0.0, log_u(rng, 6_000, d), 0.9, f"non-finite d{d}")
        assert not certain[:5500].any(), "a NaN or an infinity was screened as certain"
        assert certain[5500:].mean() > 0.9
    print(f"other inputs: {rest.n} draws, {rest.rejected} literal rejections, {rest.certain} certain, |est - ratio| / T at most 2^{np.log2(max(rest.worst, 1e-300)):.1f}")


@pytest.mark.parametrize("h", [0.9, 0.3, 0.02])
def test_near_ties_are_not_certain(lib, h):
    """z scaled by bisection until the literal ratio stands within 2^-35 T of log u: far inside the margin, so the answer is "not certain" """
    rng = np.random.default_rng(7)
    n, d = 3_000, 100
    x, z = stationary(rng, n, d)
    lt, lg = kernel_lt(x), np.log(rng.random(n))
    lo, hi = np.zeros(n), np.full(n, 64.0)                  # ratio(0 z) > 0 > log u (the drift alone moves towards the mode), ratio(64 z) << log u
    assert (literal_ratio(x, lo[:, None] * z, lt, 0.0, h) > lg).all() and (literal_ratio(x, hi[:, None] * z, lt, 0.0, h) < lg).all()
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        above = literal_ratio(x, mid[:, None] * z, lt, 0.0, h) > lg
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    for scale in (lo, hi):                                  # the two sides of the tie
        zz = scale[:, None] * z
        on, certain, est, T = screen(lib, x, zz, lt, 0.0, lg, h)
        ratio = literal_ratio(x, zz, lt, 0.0, h)
        assert on and (np.abs(ratio - lg) < 2.0 ** -35 * T).all(), "the bisection did not reach a near-tie"
        assert not certain.any(), f"{int(certain.sum())} near-ties were screened as certain"


def test_standalone_sanitizer_run(tmp_path):
    """(d) the soundness check on 10^5 draws as a program with its own main, under AddressSanitizer and UBSan, in a child process"""
    exe = tmp_path / "mala_screen_asan"
    r = subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMS_MAIN",
                        *INC, "-o", str(exe), str(SRC), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, "tests/mala_screen_ref.c -DMS_MAIN did not compile with the sanitizers:\n" + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "violations 0" in r.stdout and "draws 100000" in r.stdout
