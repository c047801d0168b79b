"""CPU tests of the zero-variance control variates (stats/variance/zv.jl): the NumPy restatement klara_jl_amd.stats.lzv / qzv and the
extended-precision helper tests/zv_ref.py against the 40-digit coefficients of tests/golden/zv_kat.npz, the structure of the control
variates, the univariate methods, exactness on a Gaussian, the least-squares property, and the library / host surface of the device form."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import klara_jl_amd as K
from klara_jl_amd import _lib as L
from klara_jl_amd import stats as S

import zv_ref as Z

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def kat():
    f = np.load(ROOT / "tests" / "golden" / "zv_kat.npz")
    assert f["value"].shape == (400, 4) and f["grad"].shape == (400, 4) and f["a1"].shape == (4, 4) and f["a2"].shape == (14, 4)
    return {k: f[k] for k in f.files}


@pytest.mark.parametrize("order", [1, 2])
def test_restatement_and_float80_helper_reproduce_the_40_digit_coefficients(kat, order):
    """err = max|A - A_true| / max|A_true| <= 16 eps cond_2(S_ff) for both the literal restatement (cov, inv, multiply) and the
    extended-precision Cholesky helper; the figures are printed beside the bound."""
    a_true = kat[f"a{order}"]
    truth = Z.zv_truth(kat["value"], kat["grad"], order)
    bound = Z.coef_bound(truth["cond"])
    fn = S.lzv if order == 1 else S.qzv
    corrected, a = fn(kat["value"], kat["grad"])
    err_np, err_ld = Z.coef_err(a, a_true), Z.coef_err(truth["a"], a_true)
    print(f"order {order}: cond2(S_ff) = {truth['cond']:.3g}, bound = {bound:.3g}, restatement err = {err_np:.3g} "
          f"({err_np / (Z.EPS * truth['cond']):.2f} eps cond2), float80 helper err = {err_ld:.3g}")
    assert a.shape == a_true.shape == (Z.nterms(4, order), 4)
    assert err_np <= bound and err_ld <= bound
    # the corrected series is chain + f a with that a
    f = S.zv_controls(kat["value"], kat["grad"], order)
    assert np.array_equal(corrected, kat["value"] + f @ a)
    scale = 16 * Z.EPS * truth["cond"] * np.abs(a_true).max() * truth["fscale"]
    assert np.abs(corrected - truth["series"]).max() <= scale


def test_control_variate_order_and_count():
    rng = np.random.default_rng(7)
    for d in (1, 2, 3, 5, 14):
        x, g = rng.standard_normal((9, d)), rng.standard_normal((9, d))
        f = S.zv_controls(x, g, 2)
        k = d * (d + 3) // 2
        assert f.shape == (9, k) == (9, S.zv_nterms(d, 2)) and S.zv_nterms(d, 1) == d
        z = -g / 2
        assert np.array_equal(f[:, :d], z) and np.array_equal(f[:, d:2 * d], 2 * z * x - 1)
        col = 2 * d
        for i in range(d - 1):                        # i outer, j inner (zv.jl:65-70)
            for j in range(i + 1, d):
                assert np.array_equal(f[:, col], x[:, i] * z[:, j] + x[:, j] * z[:, i]), (d, i, j)
                col += 1
        assert col == k
        assert np.array_equal(S.zv_controls(x, g, 1), -0.5 * g)
        # the helper forms the same columns in extended precision: at most three roundings of terms no larger than 2 max|x| max|z| + 1
        atol = 4 * Z.EPS * (2 * np.abs(x).max() * np.abs(z).max() + 1)
        assert np.abs(Z.controls(x.astype(Z.LD), g.astype(Z.LD), 2).astype(np.float64) - f).max() <= atol
    assert S.zv_nterms(14, 2) == 119 <= L.ZV_MAX_TERMS < S.zv_nterms(15, 2) and S.zv_nterms(128, 1) == L.ZV_MAX_TERMS


def test_one_dimension_reduces_to_the_univariate_methods(kat):
    x, g = kat["value"][:, 2], kat["grad"][:, 2]
    c1, a1 = S.lzv(x, g)                              # zv.jl:9-14
    cm, am = S.lzv(x[:, None], g[:, None])
    assert np.isscalar(a1) and am.shape == (1, 1) and a1 == pytest.approx(am[0, 0], rel=1e-13)
    assert np.allclose(c1, cm[:, 0], rtol=0, atol=1e-12 * np.abs(x).max())
    z = -0.5 * g
    assert a1 == pytest.approx(-np.cov(z, x)[0, 1] / z.var(ddof=1), rel=1e-12)
    c2, a2 = S.qzv(x, g)                              # zv.jl:42-48
    cq, aq = S.qzv(x[:, None], g[:, None])
    assert a2.shape == (2,) and aq.shape == (2, 1) and np.allclose(a2, aq[:, 0], rtol=1e-10)
    assert np.allclose(c2, cq[:, 0], rtol=0, atol=1e-10 * np.abs(x).max())
    t = Z.zv_truth(x[:, None], g[:, None], 2)
    assert Z.coef_err(aq, t["a"]) <= Z.coef_bound(t["cond"])


def _gaussian_history(d, n, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    p = (q * np.linspace(1.0, 6.0, d)) @ q.T          # cond_2(P) = 6
    p = (p + p.T) / 2
    mu = rng.standard_normal(d)
    x = mu + rng.standard_normal((n, d))
    return p, mu, x, -(x - mu) @ p


def test_lzv_is_exact_on_a_gaussian():
    """gradlogtarget = -P (x - mu): the linear control variates remove the variance altogether, every corrected sample is mu."""
    p, mu, x, g = _gaussian_history(32, 500, 11)
    corrected, a = S.lzv(x, g)
    tol = 64 * Z.EPS * np.linalg.cond(p, 2) * np.abs(x - mu).max()
    print(f"Gaussian D = 32: max|corrected - mu| = {np.abs(corrected - mu).max():.3g}, tolerance {tol:.3g}")
    assert np.abs(corrected - mu).max() <= tol
    assert np.abs(Z.zv_truth(x, g, 1)["series"] - mu).max() <= tol
    assert np.allclose(a, -2 * np.linalg.inv(p), rtol=0, atol=1e-10)


@pytest.mark.parametrize("order", [1, 2])
def test_least_squares_property(kat, order):
    """a minimises the sample variance of chain + f a in every dimension: it is never above the plain variance"""
    corrected, _ = (S.lzv if order == 1 else S.qzv)(kat["value"], kat["grad"])
    v0, v1 = kat["value"].var(axis=0, ddof=1), corrected.var(axis=0, ddof=1)
    print(f"order {order}: variance ratios {v0 / v1}")
    assert np.all(v1 <= v0)
    t = Z.zv_truth(kat["value"], kat["grad"], order)
    assert np.all(t["var"] <= v0)
    # NState-layout helpers (D x n in, n x D out)
    cn, an = (S.lzv_chain if order == 1 else S.qzv_chain)(kat["value"].T, kat["grad"].T)
    assert np.array_equal(cn, corrected) and an.shape == (Z.nterms(4, order), 4)


def test_library_exports_the_zv_entry_points(klib):
    for name in ("klara_get_chain_zv", "klara_get_chain_zv_series", "klara_get_chain_zv_one"):
        assert name in L.EXPORTS and hasattr(klib, name)
    assert len(klib.klara_get_chain_zv.argtypes) == 8 and len(klib.klara_get_chain_zv_series.argtypes) == 7
    header = (ROOT / "include" / "klara_hip.h").read_text()
    for name, val in (("KLARA_ZV_LINEAR", L.ZV_LINEAR), ("KLARA_ZV_QUADRATIC", L.ZV_QUADRATIC), ("KLARA_ZV_MAX_TERMS", L.ZV_MAX_TERMS)):
        assert f"#define {name} {val}\n" in header
    assert (L.ZV_LINEAR, L.ZV_QUADRATIC, L.ZV_MAX_TERMS) == (1, 2, 128)
    # NULL handle: refused before anything touches a device
    assert klib.klara_get_chain_zv(None, 1, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert klib.klara_get_chain_zv_series(None, 0, 1, None, None, 0, None) == L.ERR_INVALID_ARG
    assert klib.klara_get_chain_zv_one(None, 0, 1, None, None, None, 0, None) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("monitor, missing", [(L.MON_HISTORY, "gradlogtarget"), (L.MON_HIST_GRAD, "value"), (0, "value")])
def test_host_api_names_the_missing_monitor(monitor, missing):
    chains = K.MuvChains.__new__(K.MuvChains)
    chains._job = SimpleNamespace(engine=SimpleNamespace(monitor=monitor))
    for fn in (K.chain_lzv, K.chain_qzv, K.lzv, K.qzv):
        with pytest.raises(ValueError, match=missing):
            fn(chains)
    assert {"chain_lzv", "chain_qzv", "lzv", "qzv"} <= set(K.__all__)
