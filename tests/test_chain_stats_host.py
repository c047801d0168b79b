"""CPU tests of the chain statistics references (tests/chain_stats_ref.py): the exact reference against hand-computed rational values, the
user-facing restatement (klara_jl_amd/stats.py) and the plain f64 form against it, the mirror of the device's streaming recurrences — which
proves without a GPU that the recurrences on x lose (mean / sd)^2 digits and that the ones on x - pivot do not — and the decision margins
of every series the GPU tests (tests/test_gpu_chain_stats.py) use."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import klara_jl_amd as K
import chain_stats_ref as R


def test_exact_equals_hand_computed_rational_values():
    # 1, 2, 3, 4: mean 5/2, autocov = 5/4, 5/16, -3/8, -9/16; Gamma_0 = 25/16 > 0, Gamma_1 = -15/16 <= 0 -> m = 1
    e = R.exact([1, 2, 3, 4], 3, 2)
    assert e["m"] == 1 and e["imse"] == e["ipse"] == float((-F(5, 4) + 2 * F(25, 16)) / 4) == 0.46875
    assert e["iid"] == float(F(5, 3) / 4) and e["bm"] == 1.0 and e["acv0_n"] == 0.3125       # batch means 3/2, 7/2: var 2, 2 * 2 / 4
    assert e["margin_stop"] == 0.75 and e["margin_clamp"] == math.inf                        # min(25/16, 15/16) / (5/4)
    assert e["ess_imse"] == float(4 * F(5, 12) / F(15, 32)) and e["iact_imse"] == float(F(15, 32) / F(5, 12))
    # 0, 2, 0, 2, 0, 1: mean 5/6, autocov = 29/36, -145/216, 53/108, -25/72, 4/27, -5/216; Gamma = 29/216, 31/216, 27/216: no stop (m = 3), the
    # clamp lowers Gamma_1 to 29/216: imse = (-174 + 2 (29 + 29 + 27)) / 216 / 6 = -1/324, ipse = (-174 + 2 * 87) / 216 / 6 = 0
    e = R.exact([0, 2, 0, 2, 0, 1], 5)
    assert e["m"] == 3 and e["imse"] == float(F(-1, 324)) and e["ipse"] == 0.0 and e["iid"] == float(F(29, 180))
    assert e["margin_stop"] == float(F(27, 174)) and e["margin_clamp"] == float(F(2, 174)) and math.isnan(e["bm"])
    assert e["ess_ipse"] == math.inf and e["iact_ipse"] == 0.0
    # 1, -1, 1, -1, 1, -1 (antithetic): autocov_k = (-1)^k (6 - k) / 6, every Gamma = 1/6 (ties: nothing is clamped), imse = (-1 + 2 * 3/6) / 6 = 0
    e = R.exact([1, -1, 1, -1, 1, -1], 5, 2)
    assert e["m"] == 3 and e["imse"] == 0.0 and e["ipse"] == 0.0 and e["iid"] == 0.2 and e["bm"] == 0.0
    assert e["margin_stop"] == float(F(1, 6)) and e["margin_clamp"] == 0.0
    # maxlag = 1 (n = 2): one pair, autocov = 1/4, -1/8 -> Gamma_0 = 1/8 > 0: m = 1, imse = (-1/4 + 2/8) / 2 = 0
    e = R.exact([0, 1], 127)
    assert e["maxlag"] == 1 and e["m"] == 1 and e["imse"] == 0.0 and e["margin_stop"] == 0.5 and e["iid"] == 0.25
    # a constant series: everything 0, ESS and IACT are 0 / 0
    e = R.exact([1000.1] * 9, 5, 2)
    assert e["constant"] and e["iid"] == e["imse"] == e["ipse"] == e["bm"] == 0.0 and math.isnan(e["ess_imse"]) and math.isnan(e["iact_ipse"])


def test_stats_py_and_plain_f64_match_exact_on_centred_series():
    """klara_jl_amd/stats.py (FFT autocovariance) and plain_f64 within 1e-10 of exact — imse / ipse in IACT units, iid / bm relative."""
    V = R.series_a()
    for maxlag in (1, 2, 15, 40, 127, None):
        ex = R.exact_many(V, maxlag, 7)
        pl = R.plain_many(V, maxlag, 7)
        args = () if maxlag is None else (maxlag,)
        st = {"iid": [K.stats.mcvar(V[:, i], "iid") for i in range(24)], "bm": [K.stats.mcvar(V[:, i], "bm", 7) for i in range(24)],
              "imse": [K.stats.mcvar(V[:, i], "imse", *args) for i in range(24)], "ipse": [K.stats.mcvar(V[:, i], "ipse", *args) for i in range(24)]}
        for key in ("iid", "bm", "imse", "ipse"):
            assert R.metric(pl[key], ex, key).max() < 1e-10, ("plain_f64", maxlag, key)
            assert R.metric(st[key], ex, key).max() < 1e-10, ("stats.py", maxlag, key)
    e = R.exact(V[:, 0], 15)
    assert np.isclose(K.stats.ess(V[:, 0], "imse", 15), e["ess_imse"], rtol=1e-10) and np.isclose(K.stats.iact(V[:, 0], "ipse", 15), e["iact_ipse"], rtol=1e-10)


def _table_series():
    return R.ar1_series(600, 3, 7)[:, 0]            # AR(1), coefficient 0.6, sd 1.25, n = 600


def test_recurrences_on_raw_samples_lose_the_mean_over_sd_squared():
    """The streaming recurrences as they were (cross-products of x: pivot=False), window 16: exact to rounding at the origin, past the cap from an
    offset of 1e4 on, a wrong stopping index at 1e7; and a constant series at 1000.1 comes out with spurious positive pairs instead of 0."""
    v = _table_series()
    ex = R.exact_many(v[:, None], 16)
    err = {}
    for off in (0.0, 90.0, 1e3, 1e4, 1e5, 1e6, 1e7):
        assert np.array_equal((v + off) - off, v)                       # the shifted series is the same series: exact holds for it as it is
        imse, ipse = R.stream_f64(v + off, 17, [600], pivot=False)
        err[off] = max(R.metric(imse, ex, "imse")[0], R.metric(ipse, ex, "ipse")[0])
    assert err[0.0] < 1e-13
    for off in (1e4, 1e5, 1e6, 1e7):
        assert err[off] > R.CAP, (off, err[off])
    assert err[1e3] < err[1e4] < err[1e5] < err[1e6] < err[1e7] and err[1e7] > 1e-2
    imse, _ = R.stream_f64(np.full(600, 1000.1), 17, [600], pivot=False)
    assert imse != 0.0
    # the shift cases of the GPU tests: the old form fails them from 1e4 sd on
    V = R.series_a()
    for maxlag in (15, 40):
        ex = R.exact_many(V, maxlag)
        for off in R.OFFSETS:
            imse, ipse = R.stream_f64(V + off * R.SD, maxlag + 1, [R.N_A], pivot=False)
            worst = max(R.metric(imse, ex, "imse").max(), R.metric(ipse, ex, "ipse").max())
            assert worst > R.CAP if off >= 1e4 else (worst < R.CAP or off == 1e3), (maxlag, off, worst)       # (1e3 sd: about the cap — 1.6e-9 at maxlag 15)


def test_recurrences_on_shifted_samples_are_shift_invariant():
    """The fixed form (cross-products, total and tail of x - first sample) stays inside the tolerance at every offset, and returns exactly 0 on a
    constant series."""
    v = _table_series()
    ex = R.exact_many(v[:, None], 16)
    for off in (0.0, 90.0, 1e3, 1e4, 1e5, 1e6, 1e7):
        imse, ipse = R.stream_f64(v + off, 17, [600])
        assert max(R.metric(imse, ex, "imse")[0], R.metric(ipse, ex, "ipse")[0]) < R.TOL["shift"], off
    V = R.series_a()
    for maxlag in (15, 40):
        ex = R.exact_many(V, maxlag)
        for off in R.OFFSETS:
            assert np.array_equal((V + off * R.SD) - off * R.SD, V)
            imse, ipse = R.stream_f64(V + off * R.SD, maxlag + 1, R.splits_a()["5_1_64_130"])
            assert max(R.metric(imse, ex, "imse").max(), R.metric(ipse, ex, "ipse").max()) < R.TOL["shift"], (maxlag, off)
    C = R.constant_series()
    for W in (8, 16, 41):
        imse, ipse = R.stream_f64(C, W, [7, 1, 52])
        assert np.all(imse[:3] == 0.0) and np.all(ipse[:3] == 0.0)
        ex = R.exact_many(C[:, 3:], W - 1)
        assert R.metric(imse[3:], ex, "imse")[0] < R.TOL["shift"] and R.metric(ipse[3:], ex, "ipse")[0] < R.TOL["shift"]


@pytest.mark.parametrize("W", [2, 9, 17, 33, 34, 65, 128])
def test_stream_mirror_does_not_depend_on_the_launch_splits(W):
    """Every split of case (a) gives the same estimators up to rounding (in fact the same bits: each S_k is the same sequential sum), within
    the tolerance of exact; fewer samples than the window too."""
    V = R.series_a()[:, ::5]
    ex = R.exact_many(V, W - 1)
    ref = None
    for name, sp in R.splits_a().items():
        imse, ipse = R.stream_f64(V, W, sp)
        assert max(R.metric(imse, ex, "imse").max(), R.metric(ipse, ex, "ipse").max()) < R.TOL["selftest"], name
        if ref is not None:
            assert np.allclose(imse, ref[0], rtol=0, atol=R.TOL["selftest"] * ex["acv0_n"].min()) and np.allclose(ipse, ref[1], rtol=0, atol=R.TOL["selftest"] * ex["acv0_n"].min())
        ref = (imse, ipse)
    for n in (2, 3, 4, 17, 40):
        Vn = R.series_b(n)[:, :5]
        exn = R.exact_many(Vn, W - 1)
        imse, ipse = R.stream_f64(Vn, W, [1] * n)
        assert max(R.metric(imse, exn, "imse").max(), R.metric(ipse, exn, "ipse").max()) < R.TOL["selftest"], n


def _assert_margins(V, maxlag, what):
    ex = R.exact_many(V, maxlag)
    live = ~ex["constant"]
    if not live.any():
        return
    assert ex["margin_stop"][live].min() > R.MARGIN_MIN and ex["margin_clamp"][live].min() > R.MARGIN_MIN, (what, maxlag)


def test_no_series_of_the_gpu_tests_is_ambiguous():
    """The stop and the clamp are discontinuous: a series whose exact decision margin is below 1e-6 may not be used (the cap on ambiguous series is
    zero).  Every synthetic series of tests/test_gpu_chain_stats.py, at every lag window it is run with."""
    A = R.series_a()
    for w in R.WINDOWS + (15, 40):
        _assert_margins(A, w, "a")
    for n in (2, 3, 4, 17, 40):
        for w in (127, 32):
            _assert_margins(R.series_b(n), w, ("b", n))
        assert not R.exact_many(R.series_b(n), 127)["constant"].any()
    _assert_margins(R.series_c(), 7, "c")
    _assert_margins(R.constant_series(), 15, "e")
    assert R.exact_many(R.constant_series(), 15)["constant"].tolist() == [True, True, True, False]


@pytest.mark.parametrize("name", ["mh", "mala", "hmc", "hmc_antithetic", "slice", "hmc_rats", "mh_constant"])
def test_job_series_margins_and_streaming_batch_means_bound(name):
    """The job series of the GPU tests on the CPU oracle (the device's series bit for bit): no decision is ambiguous at the windows the jobs run
    with, and the streaming batch means from the oracle's running sums (the device's bits) are inside the derived bound (chain_stats_ref.bm_stream_bound),
    which itself stays below 1e-3 of the exact value at the chosen offsets — otherwise the case would test nothing."""
    import cases
    import oracle_ffi as O
    case = R.job_cases()[name]
    V = R.oracle_history(case)
    assert V.shape[0] == 188
    for maxlag in sorted({r[1] for r in R.JOB_RUNS if r[0] == name}) + ([None] if name == "mh" else []):     # (None: n - 1 lags, the job API's default)
        _assert_margins(V, maxlag, name)
    ex = R.exact_many(V, 12, R.JOB_BATCHLEN)
    assert ex["constant"].all() == (name == "mh_constant") and ex["constant"].any() == (name == "mh_constant")
    job = O.OracleJob(**cases.oracle_kwargs(case))
    job.set_state(case["x0"])
    bm, nb = job.run_with_batch_means(case["nsteps"], R.JOB_BATCHLEN)
    assert nb == 188 // R.JOB_BATCHLEN
    bound = R.bm_stream_bound(V, R.JOB_BATCHLEN, ex)
    err = np.abs(bm.ravel() - ex["bm"])
    assert np.all(err <= bound), (err / bound).max()
    if name != "mh_constant":
        assert np.all(bound < 1e-3 * ex["bm"]), (bound / ex["bm"]).max()
