"""The pooled effective sample size on the device (klara_ess.hip, klara_gather_ess, klara_selftest_ess) against tests/ess_ref.py: bit for bit against the
mirror of the device's order of operations, within the derived bounds of the exact rational reference, and the job path against the self-test path."""
import numpy as np
import pytest

import klara_jl_amd as K
from klara_jl_amd import _lib as L

import cases as C
import ess_ref as E
import rhat_ref as H

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.mark.parametrize("case", E.cases(), ids=lambda c: "N%d-D%d-lag%d-n%d-off%g-%s-r%d" % c)
def test_selftest_against_mirror_and_exact(lib, case):
    """csum, wsum, mean, bsum, rho, tau, ess bit for bit equal to mirror / mirror_ranks; pairs equal to exact's; every continuous output within bound() of
    exact — streamed (fed launch by launch), history and split paths, whole and cut into ranks"""
    N, D, ml, ncols, _, kind, nranks = case
    hist, exs, _ = E.case_data(case)
    bounds = H.rank_bounds(N)[nranks]
    st, res = E.selftest(lib, hist, ml, E.launch_splits(ncols, kind), bounds)
    assert st == 0
    assert (("split", False) in res) == (ncols >= 8)
    worst = 0.0
    for split in exs:
        mir = E.mirror(hist, ml, split)
        mrk = E.mirror_ranks(bounds, hist, ml, split)
        for path in (("split",) if split else ("streamed", "history")):
            worst = max(worst, E.check(res[(path, False)], mir, exs[split], 1, (case, path)))
            worst = max(worst, E.check(res[(path, True)], mrk, exs[split], nranks, (case, path, "ranks")))
    print("largest error / bound:", worst)


@pytest.mark.parametrize("shape", [(3, 3, 7, 40), (257, 4, 33, 100), (5, 100, 127, 200)], ids=str)
def test_streamed_sums_do_not_depend_on_the_launches(lib, shape):
    N, D, ml, ncols = shape
    hist = E.make_hist(N, D, ncols, 1e4, 1)
    ref = None
    for kind in E.SPLIT_KINDS + ("ones",):
        splits = [1] * ncols if kind == "ones" else E.launch_splits(ncols, kind)
        st, res = E.selftest(lib, hist, ml, splits, [0, N])
        assert st == 0
        got = res[("streamed", False)]
        if ref is None:
            ref = got
            for k in ("csum", "wsum", "mean", "bsum", "rho", "tau", "ess", "pairs"):      # the history mode feeds the same kernels: the same bits
                assert np.array_equal(res[("history", False)][k], ref[k], equal_nan=True), (kind, k)
        for k in ("csum", "wsum", "mean", "bsum", "rho", "tau", "ess", "pairs"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), (kind, k)


def test_all_chains_at_one_state_give_nan(lib):
    """var+ = 0: NaN throughout, nothing clamped — as the mirror's IEEE arithmetic gives it"""
    hist = np.full((12, 5, 3), 2.5)
    st, res = E.selftest(lib, hist, 7, [12], [0, 2, 5])
    assert st == 0
    for split, path in ((False, "streamed"), (False, "history"), (True, "split")):
        mir = E.mirror(hist, 7, split)
        for ranks in (False, True):
            got = res[(path, ranks)]
            assert np.all(np.isnan(got["ess"])) and np.all(np.isnan(got["tau"])) and np.all(np.isnan(got["rho"][:, 1:])) and np.all(got["rho"][:, 0] == 1.0)
            assert not np.any(got["wsum"]) and not np.any(got["bsum"]) and not np.any(got["csum"])
            assert np.array_equal(got["pairs"], mir["pairs"])


# ---------------------------------------------------------------- the job path
def _job(name, nchains, acov_maxlag=15, ring=0, seed=11):
    case = C.make_case(name)
    kw = C.engine_kwargs(case, monitor=L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY, nchains=nchains, nsteps=200, burnin=0, thinning=1, seed=seed,
                         acov_maxlag=acov_maxlag, steps_per_launch=32, hist_ring_cols=ring)
    eng = K.Engine(**kw)
    if case["x0"] is None:
        eng.init_state_normal()
    else:
        eng.set_state(case["x0"][:1] + 0.1 * np.random.default_rng(seed).standard_normal((nchains, eng.ndims)))
    return eng


def _history(eng):
    v = np.stack([eng.chain(c) for c in range(eng.nchains)], axis=1)         # (D, N, n)
    return np.ascontiguousarray(np.transpose(v, (2, 1, 0)))                  # (n, N, D)


@pytest.mark.parametrize("name", ["mala_d100", "mala_swiss"])
def test_job_path_equals_selftest_and_only_reads(lib, name):
    """klara_gather_ess (streamed, history, split) on a MALA job equals klara_selftest_ess on the history read back, bit for bit; the job's state and running
    sums afterwards are those of a twin that never made the call"""
    N, steps = 300, 200
    eng, twin = _job(name, N), _job(name, N)
    eng.run(100); twin.run(100)
    mid = eng.pooled_ess("streamed")                                         # in the middle of the run, too
    assert mid["nper"] == 100 and mid["lags"] == 15
    eng.pooled_ess("history", 40); eng.pooled_ess("split", 9)
    eng.run(steps - 100); twin.run(steps - 100)
    got = {"streamed": eng.pooled_ess("streamed"), "history": eng.pooled_ess("history", 15), "split": eng.pooled_ess("split", 15)}
    for a, b in zip(eng.state(), twin.state()):
        assert np.array_equal(a, b)
    for a, b in zip(eng.chain_sums(), twin.chain_sums()):
        assert np.array_equal(a, b)
    hist = _history(eng)
    assert hist.shape == (steps, N, eng.ndims)
    st, res = E.selftest(lib, hist, 15, E.launch_splits(steps, "32s"), [0, N])
    assert st == 0
    for mode in got:
        ref = res[(mode, False)]
        for k in ("ess", "tau", "rho", "mean", "wsum", "bsum", "pairs"):
            assert np.array_equal(got[mode][k], ref[k], equal_nan=True), (mode, k)
        assert (got[mode]["nunits"], got[mode]["nper"], got[mode]["lags"]) == (ref["nunits"], ref["nper"], ref["lags"])
        assert np.array_equal(got[mode]["window_exhausted"], ref["pairs"] == 8)
    assert np.all(np.isfinite(got["streamed"]["ess"])) and np.all(got["streamed"]["ess"] > 0)
    a = K.stats.pooled_ess(hist, 15)
    assert np.allclose(got["history"]["ess"], a["ess"], rtol=1e-6) and np.array_equal(got["history"]["pairs"], a["pairs"])
    eng.close(); twin.close()


def test_wrong_mode_for_the_monitors_is_a_state_error():
    eng = _job("mala_d100", 64, acov_maxlag=0)
    eng.run(6)
    with pytest.raises(K.KlaraError) as ei:
        eng.pooled_ess("streamed")
    assert ei.value.status == L.ERR_STATE
    with pytest.raises(K.KlaraError) as ei:
        eng.pooled_ess("split")                                              # 6 saved steps: under 8
    assert ei.value.status == L.ERR_STATE
    assert eng.pooled_ess("history")["nper"] == 6
    eng.close()
    eng = _job("mala_d100", 64, acov_maxlag=0, ring=16)
    eng.run(40)
    with pytest.raises(K.KlaraError) as ei:
        eng.pooled_ess("history")
    assert ei.value.status == L.ERR_STATE
    eng.close()
    eng = _job("mala_d100", 64)
    out = eng.pooled_ess("streamed")                                         # before the first saved sample: NaN and zeros, no error
    assert out["nper"] == 0 and out["nunits"] == 0 and np.all(np.isnan(out["ess"])) and not np.any(out["wsum"])
    with pytest.raises(K.KlaraError) as ei:
        L.check(L.load().klara_gather_ess(eng._h, None, 3, 0, *([None] * 10)), "klara_gather_ess")
    assert ei.value.status == L.ERR_INVALID_ARG
    with pytest.raises(K.KlaraError) as ei:
        L.check(L.load().klara_gather_ess(eng._h, None, L.ESS_STREAMED, 5, *([None] * 10)), "klara_gather_ess")
    assert ei.value.status == L.ERR_INVALID_ARG
    with pytest.raises(K.KlaraError) as ei:
        L.check(L.load().klara_gather_ess(eng._h, None, L.ESS_HISTORY, 128, *([None] * 10)), "klara_gather_ess")
    assert ei.value.status == L.ERR_INVALID_ARG
    eng.close()
