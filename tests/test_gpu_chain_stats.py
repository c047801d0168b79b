"""The chain statistics kernels (klara_monitors.hip: k_chain_stats, k_bm_close, k_acov_update<8|16|32>, k_acov_update_block, k_acov_tail_far,
k_acov_finalize) against exact rational arithmetic (tests/chain_stats_ref.py) — the numbers a user reads at the end of a run: Monte Carlo
variance, ESS, IACT.  (a)-(e) run the kernels on synthetic series through klara_selftest_chain_stats (the launch functions of the job path);
(f) runs jobs for the plumbing the self-test cannot reach: ring bookkeeping, launch planning, thinning, streaming batch means.

Error metric: imse / ipse in IACT units, |device - exact| / (exact autocov_0 / n); iid / bm relative.  Hard cap 1e-9 (chain_stats_ref.CAP);
the asserted tolerances (chain_stats_ref.TOL) are measured: profiles/chain_stats_accuracy.txt.  No series is ambiguous in the stop or the clamp
(margins above 1e-6: tests/test_chain_stats_host.py asserts that on the CPU, the job series through the CPU oracle).  Every test prints its
worst figures before it asserts them."""
import functools

import numpy as np
import pytest

import cases
import chain_stats_ref as R
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

KEYS = ("iid", "bm", "imse", "ipse", "stream_imse", "stream_ipse")


def selftest(V, nchains, ndims, maxlag, batchlen, splits):
    """klara_selftest_chain_stats on the (n x nchains*ndims) series V: dict of the six outputs, each (nchains*ndims,)."""
    klib = L.load()
    V = np.ascontiguousarray(V, dtype=np.float64)
    n, nd = V.shape
    assert nd == nchains * ndims and sum(splits) == n
    sp = np.asarray(splits, dtype=np.int64)
    out = {k: np.full(nd, np.nan) for k in KEYS}
    L.check(klib.klara_selftest_chain_stats(0, nchains, ndims, n, V.ctypes.data, maxlag, batchlen, sp.size, sp.ctypes.data,
                                            *[out[k].ctypes.data for k in KEYS]), "klara_selftest_chain_stats")
    return out


@functools.lru_cache(maxsize=None)
def _exact_a(maxlag):
    return R.exact_many(R.series_a(), maxlag, 7)


def _worst(dev, ex, what, keys=KEYS):
    """worst error per output against exact (imse / ipse, streamed or not, in IACT units; iid / bm relative), printed"""
    w = {}
    for k in keys:
        err = R.metric(dev[k], ex, k.replace("stream_", ""))
        err = err[~ex["constant"]] if k not in ("bm",) else err[~ex["constant"] & ~np.isnan(ex["bm"])]
        w[k] = float(err.max()) if err.size else 0.0
    print(f"chain_stats {what}: " + " ".join(f"{k}={v:.3g}" for k, v in w.items()))
    return w


def _assert_within(w, tol, what, tol_stream=None):
    assert tol <= R.CAP and (tol_stream is None or tol_stream <= R.CAP)
    for k, v in w.items():
        t = tol_stream if tol_stream is not None and k.startswith("stream_") else tol
        assert v <= t, (what, k, v, t)           # (NaN fails)


@pytest.mark.parametrize("maxlag", R.WINDOWS)
def test_selftest_windows_and_launch_splits(maxlag):
    """(a) 24 series (AR(1) 0.6, -0.6, white noise; dyadic grid), n = 200, every lag window that takes another kernel or another amount of a lag
    block, every launch split: one launch, all ones, 31 / 33 straddling the block delay, 32s, a first launch shorter than the window,
    [5, 1, 64, 130].  Every streaming and post-hoc estimator against exact.  Tolerance: chain_stats_ref.TOL["selftest"]
    (profiles/chain_stats_accuracy.txt, class a-c)."""
    V, ex = R.series_a(), _exact_a(maxlag)
    for name, sp in R.splits_a().items():
        out = selftest(V, 8, 3, maxlag, 7, sp)
        _assert_within(_worst(out, ex, f"a maxlag={maxlag} splits={name}"), R.TOL["selftest"], (maxlag, name))


@pytest.mark.parametrize("n", [2, 3, 4, 17, 40])
def test_selftest_fewer_samples_than_the_window(n):
    """(b) n below the window: maxlag = min(W - 1, n - 1), head and tail overlap, the lag blocks see only zeros beyond the series."""
    V = R.series_b(n)
    for maxlag in (127, 32):
        ex = R.exact_many(V, maxlag, 2)
        for name, sp in (("one", [n]), ("ones", [1] * n), ("1_rest", [1, n - 1])):
            out = selftest(V, 4, 6, maxlag, 2, sp)
            if n < 4:
                assert np.isnan(out["bm"]).all()              # fewer than two batches
            _assert_within(_worst(out, ex, f"b n={n} maxlag={maxlag} splits={name}", [k for k in KEYS if k != "bm" or n >= 4]), R.TOL["selftest"], (n, maxlag, name))


def test_selftest_grid_edge():
    """(c) 300 series: the second workgroup is partly empty."""
    V = R.series_c()
    ex = R.exact_many(V, 7, 5)
    out = selftest(V, 60, 5, 7, 5, [13, 27])
    _assert_within(_worst(out, ex, "c 300 series"), R.TOL["selftest"], "c")


@pytest.mark.parametrize("maxlag", [15, 40])
def test_selftest_shift_invariance(maxlag):
    """(d) the series of (a) plus 0, 90, 1e3, 1e4, 1e6, 1e8 sd (exactly representable: the shifted series is the same series, and the exact values are
    those of the unshifted one).  Streaming and post-hoc, inside the tolerance at every offset — chain_stats_ref.TOL["shift"]
    (profiles/chain_stats_accuracy.txt, class d).  The recurrences on raw samples fail from 1e4 sd on (and the two-pass post-hoc kernel centred on the
    rounded mean at 1e8 sd)."""
    V, ex = R.series_a(), _exact_a(maxlag)
    worst = {}
    for off in R.OFFSETS:
        Vs = V + off * R.SD
        assert np.array_equal(Vs - off * R.SD, V)
        worst[off] = _worst(selftest(Vs, 8, 3, maxlag, 7, R.splits_a()["5_1_64_130"]), ex, f"d maxlag={maxlag} offset={off:g} sd")
    for off in R.OFFSETS:
        _assert_within(worst[off], R.TOL["shift"], (maxlag, off))


def test_selftest_constant_and_almost_constant_series():
    """(e) c = 0.1, 1000.1, 2^20 and a series that changes once.  Constant: the exact value is 0 with a stop at the first pair; the post-hoc |imse|, |ipse|
    and iid at most (4 n u |c|)^2 (maxlag + 1) / n (a computed mean off by at most n u |c|), the streaming path exactly 0."""
    V = R.constant_series()
    n = V.shape[0]
    for maxlag in (15, 40):
        out = selftest(V, 2, 2, maxlag, 7, [7, 1, n - 8])
        for i, c in enumerate((0.1, 1000.1, 2.0 ** 20)):
            bound = R.constant_bound(c, n, maxlag)
            print(f"chain_stats e maxlag={maxlag} c={c:g}: " + " ".join(f"{k}={out[k][i]:.3g}" for k in KEYS) + f" bound={bound:.3g}")
            for k in ("iid", "imse", "ipse", "bm"):
                assert abs(out[k][i]) <= bound, (k, c)
            assert out["stream_imse"][i] == 0.0 and out["stream_ipse"][i] == 0.0, c
        ex = R.exact_many(V[:, 3:], maxlag, 7)
        _assert_within(_worst({k: out[k][3:] for k in KEYS}, ex, f"e maxlag={maxlag} one change"), R.TOL["shift"], "one change")


# ---------------------------------------------------------------- (f) jobs
@functools.lru_cache(maxsize=None)
def _twin(name):
    """the job with a full value history: (engine, V (nsaved x nchains*D))"""
    case = R.job_cases()[name]
    twin = K.Engine(**cases.engine_kwargs(case, monitor=L.MON_HISTORY | L.MON_SUMMARIES))
    twin.set_state(case["x0"])
    twin.run(case["nsteps"])
    V = np.stack([twin.chain(c) for c in range(case["nchains"])])           # (chains, D, n)
    return twin, np.ascontiguousarray(V.transpose(2, 0, 1).reshape(V.shape[2], -1))


@pytest.mark.parametrize("name,maxlag,spl,hist", R.JOB_RUNS)
def test_jobs_against_exact(name, maxlag, spl, hist):
    """(f) MH, MALA, HMC (one antithetic setting) and the slice sampler on a diagonal Gaussian with means (0, 90, 1e4, -1e6, 3) sigma, hmc_rats, and an
    MH job whose proposals are all rejected (a constant off-centre chain): 7 chains, 400 steps, thinning 2, the burn-in ending inside a launch, launches
    of 7 and 50 transitions, windows 12 and 40 with and without a value history (without: the estimator's own 32-column ring wraps), bm_batchlen 7, the
    run split into two calls.  Everything read through the API against exact on the read-back history of a full-history twin.

    Streaming batch means read the transition kernels' running sums (bit-exact against the oracle, not changed): their loss on off-centre chains is
    bounded, not fixed — chain_stats_ref.bm_stream_bound derives |error| from the recursive-summation bound on two running sums of nsaved terms
    carried through the difference and the variance; tests/test_chain_stats_host.py requires the bound to stay below 1e-3 of the exact value."""
    case = R.job_cases()[name]
    nsteps = case["nsteps"]
    twin, V = _twin(name)
    ex = R.exact_many(V, maxlag, R.JOB_BATCHLEN)
    eng = K.Engine(**cases.engine_kwargs(case, monitor=L.MON_SUMMARIES | (L.MON_HISTORY if hist else 0), acov_maxlag=maxlag, steps_per_launch=spl,
                                         bm_batchlen=R.JOB_BATCHLEN))
    eng.set_state(case["x0"])
    eng.run(150); eng.run(nsteps - 150)
    assert np.array_equal(eng.state()[0], twin.state()[0])                   # same job
    imse, ipse, ns = eng.chain_acov_mcvar()
    bm, nb = eng.chain_bm()
    assert ns == V.shape[0] == 188 and nb == 188 // R.JOB_BATCHLEN
    iid, ph_bm, ph_imse = twin.chain_mcvar(R.JOB_BATCHLEN, maxlag)
    dev = {"iid": iid, "bm": ph_bm, "imse": ph_imse, "ipse": twin.chain_mcvar_ipse(maxlag), "stream_imse": imse, "stream_ipse": ipse}
    dev = {k: v.ravel() for k, v in dev.items()}
    bound = R.bm_stream_bound(V, R.JOB_BATCHLEN, ex)
    bm_err = np.abs(bm.ravel() - ex["bm"])
    print(f"chain_stats f {name} maxlag={maxlag} spl={spl} hist={hist}: streaming bm error / bound = {(bm_err / bound).max():.3g}, "
          f"bound / bm = {np.nanmax(bound / ex['bm']) if not ex['constant'].all() else 0:.3g}")
    if name == "mh_constant":
        assert ex["constant"].all()
        for k in KEYS:
            assert np.all(dev[k] == 0.0), k                                  # exactly 0: the deviations from the first sample are
    else:
        _assert_within(_worst(dev, ex, f"f {name} maxlag={maxlag} spl={spl} hist={hist}"), R.TOL["jobs"], name, R.TOL["jobs_stream"])
    assert np.all(bm_err <= bound)
    eng.close()


@pytest.mark.parametrize("name", ["mh", "mh_constant"])
def test_job_api_ess_and_iact(name):
    """K.chain_ess / K.chain_iact / K.chain_mcvar on a job that stores its values, against exact on the values it hands back; a constant series gives
    NaN (0 / 0 in the reference's arithmetic), not a ratio of rounding noise."""
    case = R.job_cases()[name]
    p = K.BasicContMuvParameter("p", logtarget=case["target"])
    job = K.BasicMCJob(K.likelihood_model(p, False), K.MH(case["mh_sigma"]), K.BasicMCRange(nsteps=case["nsteps"], burnin=case["burnin"], thinning=case["thinning"]),
                       {"p": case["x0"]}, seed=20260927, steps_per_launch=50)
    K.run(job)
    chain = K.output(job)
    V = np.stack([chain.value(c) for c in range(case["nchains"])])
    V = np.ascontiguousarray(V.transpose(2, 0, 1).reshape(V.shape[2], -1))
    for maxlag in (12, None):
        ex = R.exact_many(V, maxlag, R.JOB_BATCHLEN)
        for vtype in ("imse", "ipse"):
            ess, iact = K.chain_ess(chain, vtype, maxlag=maxlag).ravel(), K.chain_iact(chain, vtype, maxlag=maxlag).ravel()
            if name == "mh_constant":
                assert np.isnan(ess).all() and np.isnan(iact).all()
                continue
            # ESS = n iid / mcvar and IACT = mcvar / iid: with mcvar off by e (IACT units, e * acv0 / n) and iid by a relative r, the IACT moves by
            # e n / (n - 1) + r IACT and the ESS by the same relative amount as the IACT
            tol = 2.0 * R.TOL["jobs"] * (1.0 + np.abs(ex["iact_" + vtype]))
            err_i = np.abs(iact - ex["iact_" + vtype])
            err_e = np.abs(ess / ex["ess_" + vtype] - 1.0) * np.abs(ex["iact_" + vtype])
            print(f"chain_stats f api {name} {vtype} maxlag={maxlag}: iact error {err_i.max():.3g}, ess error (IACT units) {err_e.max():.3g}")
            assert np.all(err_i <= tol) and np.all(err_e <= tol)
        bmv = K.chain_mcvar(chain, "bm", R.JOB_BATCHLEN).ravel()
        if name == "mh_constant":
            assert np.all(bmv == 0.0)
        else:
            assert R.metric(bmv, ex, "bm").max() <= R.TOL["jobs"]
    job.close()
