"""GPU tests of the zero-variance control variates on the device (klara_get_chain_zv / klara_get_chain_zv_series, csrc/klara_zv.hip)
against the extended-precision restatement tests/zv_ref.py ON THE SAME HISTORY, read back chain by chain.

Error measure for coefficients: err = max|A - A_true| / max|A_true| <= 16 eps cond_2(S_ff) (zv_ref.coef_bound); for zv_mean and the
corrected series the propagated bound 16 eps cond_2 max|A| sum_k max_t|f_k|.  Every figure is printed before it is asserted."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import klara_jl_amd as K
from klara_jl_amd import _lib as L
from klara_jl_amd import stats as S

import cases
import zv_ref as Z

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]
ROOT = Path(__file__).resolve().parent.parent
MON = L.MON_HISTORY | L.MON_HIST_GRAD
SWISS_X0 = np.array([5.1, -0.9, 8.2, -4.5])


def _swiss_start(n):
    return SWISS_X0[None, :] + 0.1 * np.random.default_rng(4096).standard_normal((n, 4))


def _swiss_engine(nchains, x0, nsteps=1200, burnin=200, driftstep=0.1, run=True, **kw):
    X, y = cases.swiss_data()
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), nchains=nchains, nsteps=nsteps, burnin=burnin,
                   driftstep=driftstep, monitor=kw.pop("monitor", MON), seed=20131023, **kw)
    eng.set_state(x0)
    if run:
        eng.run(nsteps)
    return eng


def _history(eng, c):
    """(value, grad) of chain c as (n x D) matrices"""
    return np.ascontiguousarray(eng.chain(c).T), np.ascontiguousarray(eng.chain_fields(c, False, True)[1].T)


def _var_bound(pb, var_ref, n):
    """a series known to pb everywhere: |var - var_ref| <= 2 pb sd_ref sqrt(n / (n - 1)) + pb^2 n / (n - 1), plus the rounding of the sum itself"""
    return 2 * pb * np.sqrt(var_ref * n / (n - 1)) + pb * pb * n / (n - 1) + 8 * Z.EPS * var_ref


def _check_chain(eng, c, order, coef, zmean, zvar, label):
    """device results of one chain against the float80 truth on its own history; returns (truth, propagated bound, device series)"""
    v, g = _history(eng, c)
    t = Z.zv_truth(v, g, order)
    bound = Z.coef_bound(t["cond"])
    err = Z.coef_err(coef, t["a"])
    a_np = (S.lzv if order == 1 else S.qzv)(v, g)[1]
    print(f"{label} chain {c} order {order}: cond2 = {t['cond']:.3g}, bound = {bound:.3g}, device err = {err:.3g} "
          f"({err / (Z.EPS * t['cond']):.2f} eps cond2), NumPy restatement err = {Z.coef_err(a_np, t['a']):.3g}")
    assert err <= bound, (label, c, order, err, bound)
    pb = bound * np.abs(t["a"]).max() * t["fscale"]
    series = eng.chain_zv_series(c, order).T
    e_mean, e_series = np.abs(zmean - t["mean"]).max(), np.abs(series - t["series"]).max()
    print(f"{label} chain {c} order {order}: propagated bound = {pb:.3g}, zv_mean err = {e_mean:.3g}, series err = {e_series:.3g}, "
          f"max zv_var / var(x) = {(zvar / v.var(axis=0, ddof=1)).max():.3g}")
    assert series.shape == v.shape and e_mean <= pb and e_series <= pb, (label, c, order, e_mean, e_series, pb)
    assert np.all(np.abs(zvar - t["var"]) <= _var_bound(pb, t["var"], v.shape[0])), (label, c, order, zvar, t["var"])
    assert np.all(zvar <= v.var(axis=0, ddof=1)) and np.all(zvar >= 0), (label, c, order)
    return t, pb, series


@pytest.fixture(scope="module")
def swiss4096():
    eng = _swiss_engine(4096, _swiss_start(4096))
    assert eng.layout()[0] == 2 and eng.saved_steps() == 1000
    yield eng
    eng.close()


@pytest.mark.parametrize("order", [1, 2])
def test_accuracy_on_swiss_per_chain(swiss4096, order):
    eng = swiss4096
    coef, zm, zv, info, n = eng.chain_zv(order)
    assert n == 1000 and coef.shape == (4096, Z.nterms(4, order), 4) and np.all(info == 0) and np.all(np.isfinite(coef))
    for c in (0, 1, 511, 1366, 2047, 2731, 4094, 4095):          # first, last and spread
        _check_chain(eng, c, order, coef[c], zm[c], zv[c], "swiss")


@pytest.mark.parametrize("order", [1, 2])
def test_accuracy_on_swiss_pooled(order):
    eng = _swiss_engine(64, _swiss_start(64))
    coef, zm, zv, info, n = eng.chain_zv(order, pooled=True)
    assert coef.shape == (Z.nterms(4, order), 4) and np.all(info == 0) and n == 1000
    hist = [_history(eng, c) for c in range(64)]
    t = Z.zv_truth(np.concatenate([h[0] for h in hist]), np.concatenate([h[1] for h in hist]), order)
    err, bound = Z.coef_err(coef, t["a"]), Z.coef_bound(t["cond"])
    a_np = (S.lzv if order == 1 else S.qzv)(np.concatenate([h[0] for h in hist]), np.concatenate([h[1] for h in hist]))[1]
    print(f"swiss pooled (64 x 1000) order {order}: cond2 = {t['cond']:.3g}, bound = {bound:.3g}, device err = {err:.3g}, "
          f"NumPy restatement err = {Z.coef_err(a_np, t['a']):.3g}")
    assert err <= bound
    for c in (0, 17, 63):
        v, g = hist[c]
        ref = Z.apply_coef(v, g, order, t["a_ld"])
        pb = bound * np.abs(t["a"]).max() * ref["fscale"]
        series = eng.chain_zv_series(c, order, coef=coef).T
        print(f"swiss pooled chain {c} order {order}: propagated bound = {pb:.3g}, zv_mean err = {np.abs(zm[c] - ref['mean']).max():.3g}, "
              f"series err = {np.abs(series - ref['series']).max():.3g}")
        assert np.abs(zm[c] - ref["mean"]).max() <= pb and np.abs(series - ref["series"]).max() <= pb
        assert np.all(np.abs(zv[c] - ref["var"]) <= _var_bound(pb, ref["var"], v.shape[0]))
    eng.close()


def test_variance_reduction_matches_the_restatement(swiss4096):
    """zv_var <= var(x) for every chain and dimension; across the 4,096 chains the variance of the ZV means is smaller than that of the
    plain means in every dimension, and the ratio equals the NumPy restatement's on the same histories to the propagated tolerance."""
    eng = swiss4096
    hist = [_history(eng, c) for c in range(4096)]
    plain = np.stack([h[0].mean(axis=0) for h in hist])
    xvar = np.stack([h[0].var(axis=0, ddof=1) for h in hist])
    lines = ["zero-variance control variates on the swiss logistic regression (lambda = 100): MALA driftstep 0.1, 4,096 chains, burn-in 200, 1,000 saved steps",
             "across-chain variance of the per-chain means, plain / ZV, per dimension (device | NumPy restatement on the same histories)"]
    for order in (1, 2):
        _, zm, zv, info, _ = eng.chain_zv(order, want=("mean", "var"))
        assert np.all(info == 0) and np.all(zv <= xvar)
        fn = S.lzv if order == 1 else S.qzv
        m_np, pb = np.empty_like(zm), np.empty(4096)
        for c, (v, g) in enumerate(hist):
            corrected, a = fn(v, g)
            m_np[c] = corrected.mean(axis=0)
            fc = S.zv_controls(v, g, order)
            cond = np.linalg.cond((fc - fc.mean(axis=0)).T @ (fc - fc.mean(axis=0)), 2)
            pb[c] = Z.coef_bound(cond) * np.abs(a).max() * np.abs(fc).max(axis=0).sum()
        r_dev, r_np = plain.var(axis=0, ddof=1) / zm.var(axis=0, ddof=1), plain.var(axis=0, ddof=1) / m_np.var(axis=0, ddof=1)
        # both sets of means are within pb of the truth, so they differ by <= 2 max pb; a standard deviation moves by at most that much
        delta = 2 * pb.max() * np.sqrt(4096 / 4095) / np.sqrt(np.minimum(zm.var(axis=0, ddof=1), m_np.var(axis=0, ddof=1)))
        tol = r_np * (2 * delta + delta * delta) / (1 - delta) ** 2
        print(f"order {order}: ratios device {r_dev}, NumPy {r_np}, |difference| {np.abs(r_dev - r_np)}, tolerance {tol}; "
              f"mean within-chain var(x) / zv_var = {(xvar / zv).mean(axis=0)}")
        assert np.all(zm.var(axis=0, ddof=1) < plain.var(axis=0, ddof=1)) and np.all(delta < 0.5)
        assert np.all(np.abs(r_dev - r_np) <= tol)
        lines.append(f"order {order} ({'lzv' if order == 1 else 'qzv'}): device " + " ".join(f"{r:.1f}" for r in r_dev) + " | NumPy " + " ".join(f"{r:.1f}" for r in r_np)
                     + " | mean within-chain var(x) / zv_var " + " ".join(f"{r:.1f}" for r in (xvar / zv).mean(axis=0)))
    out = ROOT / "build"                          # git-ignored; the figures of profiles/zv_posthoc.txt section 2 are copied from here
    out.mkdir(exist_ok=True)
    (out / "zv_variance_ratios.txt").write_text("\n".join(lines) + "\n")


def _gauss_exact(eng, mu, cond_p, label):
    """gradlogtarget = -P (x - mu): lzv removes the variance altogether, every corrected sample is mu.  The device is held to the truth on the
    same history by the bounds used everywhere in this file, and therefore to mu within that bound plus the truth's own distance from mu;
    the host test's figure 64 eps cond_2(P) max|x - mu| is printed beside it."""
    coef, zm, zv, info, n = eng.chain_zv(1)
    assert np.all(info == 0)
    for c in (0, eng.nchains - 1):
        t, pb, series = _check_chain(eng, c, 1, coef[c], zm[c], zv[c], label)
        v, _ = _history(eng, c)
        own = np.abs(t["series"] - mu).max()
        print(f"{label} chain {c}: n = {n}, max|corrected - mu| = {np.abs(series - mu).max():.3g}, max|zv_mean - mu| = {np.abs(zm[c] - mu).max():.3g}, "
              f"truth's own {own:.3g}, bound {pb + own:.3g}, 64 eps cond2(P) max|x - mu| = {64 * Z.EPS * cond_p * np.abs(v - mu).max():.3g}, max zv_var = {zv[c].max():.3g}")
        assert np.abs(series - mu).max() <= pb + own and np.abs(zm[c] - mu).max() <= pb + own
        assert np.all(zv[c] <= 2 * (pb + own) ** 2)


def test_gaussian_exactness_dense_d100_hmc():
    """D = 100: 7 tiles of 16 with a ragged last one, 77 accumulator tiles on 8 wavefronts."""
    d = 100
    rng = np.random.default_rng(100)
    p = cases.compound_symmetric_precision(d)
    mu = rng.standard_normal(d)
    eng = K.Engine(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(p, mu=mu), nchains=48, nsteps=2100, burnin=100, leapstep=0.1, nleaps=8, monitor=MON)
    eng.set_state(mu[None, :] + rng.standard_normal((48, d)))
    eng.run(2100)
    assert eng.layout()[0] == 1
    _gauss_exact(eng, mu, np.linalg.cond(p, 2), "dense Gaussian D = 100, HMC")
    eng.close()


def test_gaussian_exactness_diag_d128_mala():
    """K = D = 128: 100 accumulator tiles, 13 to a wavefront; the history written by the pair-transposed kernels."""
    d = 128
    mu, sg = np.linspace(-2, 3, d), np.linspace(0.8, 1.25, d)
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.mvnormal(mu, sg), nchains=40, nsteps=2100, burnin=100, driftstep=0.2, monitor=MON)
    eng.set_state(mu[None, :] + sg[None, :] * np.random.default_rng(128).standard_normal((40, d)))
    eng.run(2100)
    assert eng.layout()[0] == 3                                   # the pair-transposed kernels
    _gauss_exact(eng, mu, (sg.max() / sg.min()) ** 2, "diagonal Gaussian D = 128, MALA")
    eng.close()


def _layout_case(kind):
    rng = np.random.default_rng(70 + kind)
    if kind == 0:
        mu, sg = np.linspace(-2, 3, 7), np.linspace(0.5, 2.0, 7)
        return dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.mvnormal(mu, sg), nchains=37, nsteps=300, burnin=20, driftstep=0.4), mu + rng.standard_normal((37, 7))
    if kind == 1:
        return (dict(sampler=L.SAMPLER_MALA, target=K.GaussDenseTarget(cases.compound_symmetric_precision(20, 0.3)), nchains=35, nsteps=300, burnin=20, driftstep=0.3),
                rng.standard_normal((35, 20)))
    if kind == 2:
        X, y = cases.swiss_data()
        return dict(sampler=L.SAMPLER_HMC, target=K.LogisticTarget(X, y, 100.0), nchains=65, nsteps=320, burnin=60, leapstep=0.05, nleaps=6), _swiss_start(65)
    if kind == 3:
        return dict(sampler=L.SAMPLER_HMC, target=K.GaussDiagTarget.negdot(100), nchains=70, nsteps=330, burnin=30, leapstep=0.1, nleaps=5), rng.standard_normal((70, 100))
    if kind == 4:
        t = cases.rats_target()
        return (dict(sampler=L.SAMPLER_HMC, target=t, nchains=37, nsteps=500, burnin=100, leapstep=0.01, nleaps=8),
                t.least_squares_start()[None, :] + 0.05 * rng.standard_normal((37, t.ndims)))
    if kind == 6:                                 # (with KLARA_DENSE_SPLIT=1: the workgroup-split kernels below D = 257, as tests/test_gpu_parity.py runs them)
        mu = rng.standard_normal(100)
        return (dict(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(cases.compound_symmetric_precision(100), mu=mu), nchains=35, nsteps=620, burnin=20, leapstep=0.1, nleaps=8),
                mu[None, :] + rng.standard_normal((35, 100)))
    d, nd = 20, 400
    X = rng.standard_normal((nd, d)); beta = rng.standard_normal(d)
    y = (rng.random(nd) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return dict(sampler=L.SAMPLER_HMC, target=K.LogisticTarget(X, y, 10.0), nchains=45, nsteps=330, burnin=30, leapstep=0.07, nleaps=5), 0.1 * rng.standard_normal((45, d))


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, 6])
def test_every_history_writing_layout(kind, monkeypatch):
    """hist_g is read the same way whichever kernel family wrote it: layout kinds 0 - 6, MALA and HMC, against the truth on the histories
    klara_get_chain / klara_get_chain_fields return.  Kind 6 (the workgroup-split dense kernels) serves D >= 257 by default; KLARA_DENSE_SPLIT=1
    puts a dense target of any size on it, here D = 100."""
    if kind == 6:
        monkeypatch.setenv("KLARA_DENSE_SPLIT", "1")
    kw, x0 = _layout_case(kind)
    eng = K.Engine(monitor=MON, **kw)
    eng.set_state(x0)
    eng.run(kw["nsteps"])
    assert eng.layout()[0] == kind, eng.layout()
    for order in ((1, 2) if eng.ndims <= 14 else (1,)):
        coef, zm, zv, info, _ = eng.chain_zv(order)
        for c in (0, eng.nchains - 1):
            assert info[c] == 0
            _check_chain(eng, c, order, coef[c], zm[c], zv[c], f"layout kind {kind}")
    eng.close()


def test_determinism_and_sharding(swiss4096):
    eng = swiss4096
    for order in (1, 2):
        a = eng.chain_zv(order)
        b = eng.chain_zv(order)
        assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4]))
        assert np.array_equal(eng.chain_zv_series(77, order), eng.chain_zv_series(77, order))
        pa, pb = eng.chain_zv(order, pooled=True), eng.chain_zv(order, pooled=True)
        assert all(np.array_equal(p, q) for p, q in zip(pa[:4], pb[:4]))
    # chains 1000 .. 1999 as a handle of their own: bit for bit the same per-chain results
    x0 = _swiss_start(4096)
    part = _swiss_engine(1000, x0[1000:2000], chain_offset=1000)
    assert np.array_equal(part.chain(3), eng.chain(1003))
    for order in (1, 2):
        full, sub = eng.chain_zv(order), part.chain_zv(order)
        for p, q in zip(full[:4], sub[:4]):
            assert np.array_equal(p[1000:2000], q)
        assert np.array_equal(eng.chain_zv_series(1999, order), part.chain_zv_series(999, order))
    part.close()
    # the same job in several klara_run calls and short launches
    split = _swiss_engine(1000, x0[1000:2000], chain_offset=1000, run=False, steps_per_launch=7)
    for k in (150, 333, 717):
        split.run(k)
    for order in (1, 2):
        for p, q in zip(eng.chain_zv(order)[:4], split.chain_zv(order)[:4]):
            assert np.array_equal(p[1000:2000], q)
    split.close()


def test_host_api_lzv_and_qzv_of_one_chain():
    """K.lzv / K.qzv(chains, chain=c): what the reference's lzv(s::ParameterNState) returns for that chain — (chain + f a (n x D), a) — from one fit of
    that chain on the device, bit for bit the all-chains call's coefficients and series; K.chain_lzv / K.chain_qzv for all chains."""
    X, y = cases.swiss_data()
    p = K.BasicContMuvParameter("p", logtarget=K.LogisticTarget(X, y, 100.0))
    job = K.BasicMCJob(K.likelihood_model(p, False), K.MALA(0.1), K.BasicMCRange(nsteps=500, burnin=100), {"p": _swiss_start(70)}, seed=20131023,
                       outopts={"monitor": ["value", "gradlogtarget"]})
    K.run(job)
    chains = K.output(job)
    eng = job.engine
    for order, one, every in ((1, K.lzv, K.chain_lzv), (2, K.qzv, K.chain_qzv)):
        zm, zv, coef, info = every(chains)
        assert np.all(info == 0) and coef.shape == (70, Z.nterms(4, order), 4) and zm.shape == zv.shape == (70, 4)
        for c in (0, 69):
            series, a = one(chains, chain=c)
            assert series.shape == (400, 4) and np.array_equal(a, coef[c]) and np.array_equal(series.T, eng.chain_zv_series(c, order))
            _check_chain(eng, c, order, a, zm[c], zv[c], "host API")
            assert np.allclose(series.mean(axis=0), zm[c], rtol=0, atol=8 * Z.EPS * np.abs(series).max())
        pm, pv, pcoef, pinfo = every(chains, pooled=True)
        assert pcoef.shape == (Z.nterms(4, order), 4) and np.all(pinfo == 0) and np.all(np.isfinite(pm)) and np.all(pv >= 0)
    v, a, info = eng.chain_zv_one(5, 2)
    assert info == 0 and v.shape == (4, 400)
    job.close()


def _status(fn):
    with pytest.raises(K.KlaraError) as ei:
        fn()
    return ei.value.status


def test_failure_modes():
    x0 = _swiss_start(16)
    # order outside {1, 2}
    eng = _swiss_engine(16, x0, nsteps=60, burnin=10)
    for order in (0, 3, -1):
        assert eng._lib.klara_get_chain_zv(eng._h, order, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
        assert eng._lib.klara_get_chain_zv_series(eng._h, 0, order, None, None, 0, None) == L.ERR_INVALID_ARG
    assert eng._lib.klara_get_chain_zv_series(eng._h, 16, 1, None, None, 0, None) == L.ERR_INVALID_ARG
    eng.close()
    # a monitor missing, a ring history, fewer than two saved steps: KLARA_ERR_STATE
    for kw in (dict(monitor=L.MON_HISTORY), dict(monitor=L.MON_HIST_GRAD), dict(monitor=MON, hist_ring_cols=8)):
        eng = _swiss_engine(16, x0, nsteps=60, burnin=10, **kw)
        assert _status(lambda: eng.chain_zv(1)) == L.ERR_STATE and _status(lambda: eng.chain_zv_series(0, 2)) == L.ERR_STATE
        eng.close()
    eng = _swiss_engine(16, x0, nsteps=60, burnin=10, run=False)
    assert _status(lambda: eng.chain_zv(1)) == L.ERR_STATE
    eng.run(11)
    assert eng.saved_steps() == 1 and _status(lambda: eng.chain_zv(1)) == L.ERR_STATE
    eng.close()
    # more than 128 control variates: D = 15 at order 2 (K = 135), D = 129 at order 1
    for d, order in ((15, 2), (129, 1)):
        eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(d), nchains=9, nsteps=40, burnin=0, driftstep=0.2, monitor=MON)
        eng.init_state_normal(); eng.run(40)
        assert _status(lambda: eng.chain_zv(order)) == L.ERR_UNSUPPORTED and _status(lambda: eng.chain_zv_series(0, order)) == L.ERR_UNSUPPORTED
        if d == 15:
            assert np.all(eng.chain_zv(1)[3] == 0)
        eng.close()
    # n <= K + 1: info = 2, NaN outputs, KLARA_OK; the pooled form of the same job has 16 n samples
    eng = _swiss_engine(16, x0, nsteps=25, burnin=10)            # n = 15, order 2: K = 14
    coef, zm, zv, info, n = eng.chain_zv(2)
    assert n == 15 and np.all(info == 2) and np.all(np.isnan(coef)) and np.all(np.isnan(zm)) and np.all(np.isnan(zv))
    assert np.all(np.isnan(eng.chain_zv_series(0, 2)))
    coef, zm, zv, info, n = eng.chain_zv(1)                      # K = 4: enough
    assert np.all(info == 0) and np.all(np.isfinite(zm))
    coef, zm, zv, info, n = eng.chain_zv(2, pooled=True)
    assert np.all(info == 0) and np.all(np.isfinite(coef)) and np.all(np.isfinite(zm))
    eng.close()
    eng = _swiss_engine(16, x0, nsteps=26, burnin=10)            # n = 16 = K + 2: no longer too few
    assert np.all(eng.chain_zv(2)[3] != 2)
    eng.close()


def test_a_chain_that_never_moves_is_reported_not_propagated():
    x0 = _swiss_start(16)
    stuck = _swiss_engine(16, x0, nsteps=80, burnin=10, driftstep=1e3)
    twin = _swiss_engine(16, x0, nsteps=80, burnin=10)
    assert np.array_equal(stuck.chain(5), np.repeat(x0[5][:, None], 70, axis=1))
    for order in (1, 2):
        coef, zm, zv, info, _ = stuck.chain_zv(order)
        assert np.all(info == 1) and np.all(np.isnan(coef)) and np.all(np.isnan(zm)) and np.all(np.isnan(zv))
        assert np.all(np.isnan(stuck.chain_zv_series(3, order)))
        _, _, _, pinfo, _ = stuck.chain_zv(order, pooled=True)
        assert np.all(pinfo == pinfo[0])
        coef, zm, zv, info, _ = twin.chain_zv(order)
        assert np.all(info == 0) and np.all(np.isfinite(coef)) and np.all(np.isfinite(zm)) and np.all(np.isfinite(zv))
    stuck.close(); twin.close()


_CANARY = r'''
import sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import klara_jl_amd as K
from klara_jl_amd import _lib as L
import cases
X, y = cases.swiss_data()
for target, kw, orders in ((K.LogisticTarget(X, y, 100.0), dict(sampler=L.SAMPLER_MALA, driftstep=0.1), (1, 2)),
                           (K.GaussDiagTarget.negdot(100), dict(sampler=L.SAMPLER_MALA, driftstep=0.2), (1,)),
                           (K.GaussDiagTarget.negdot(14), dict(sampler=L.SAMPLER_HMC, leapstep=0.2, nleaps=4), (2,))):
    e = K.Engine(target=target, nchains=1003, nsteps=181, burnin=20, monitor=L.MON_HISTORY | L.MON_HIST_GRAD, **kw)
    if isinstance(target, K.LogisticTarget):       # (the example's start: from N(0, I) some MALA chains sit still through all 181 transitions)
        e.set_state(np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(3).standard_normal((1003, 4)))
    else:
        e.init_state_normal()
    e.run(181)
    for order in orders:
        for pooled in (False, True):
            coef, zm, zv, info, n = e.chain_zv(order, pooled)
            assert n == 161 and np.all(info == 0) and np.all(np.isfinite(zm)), (order, pooled, int((info != 0).sum()), int(np.isnan(zm).sum()))
        assert np.all(np.isfinite(e.chain_zv_series(1002, order)))
    e.close()                      # raises when a canary of the job was damaged; the calls' own workspaces are checked as they are released
print("INTACT")
'''


def test_zv_between_canaries():
    env = dict(os.environ, KLARA_DEBUG_CANARY="1")
    r = subprocess.run([sys.executable, "-c", _CANARY.replace("ROOT", str(ROOT))], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("INTACT")
