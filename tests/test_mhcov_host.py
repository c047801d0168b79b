"""MH with a full proposal covariance, MH(Σ), without a GPU: the id, scope and refusals of the C ABI, the run-time compilation of the new kernels of a
user's closure for gfx950, the CPU reference (tests/mhcov_ref.py) against what already exists (the oracle's MH job with a diagonal factor, its RAM job's
first transition with S0 = L) and against the independent NumPy restatement (tests/mhcov_mirror.py), the Python constructors, the mechanical checks of the
Julia mapping and the header text, and the statistical soundness of the reference."""
import re
from pathlib import Path

import numpy as np
import pytest

import autodiff_cases as ADC
import cases
import klara_jl_amd as K
import mhcov_cases as MC
import mhcov_ref as MR
import oracle_ffi as O
import ram_cases as RC
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent


def _status(**over):
    X, y = cases.swiss_data()
    kw = dict(target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=20, **MC.mhcov(0.3 * np.eye(4)))
    kw.update(over)
    if "target" in over and "mh_factor" not in over and kw["sampler"] == L.SAMPLER_MH_COV:
        kw["mh_factor"] = 0.3 * np.eye(kw["target"].ndims)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


def test_create_accepts_and_refuses_like_the_issue_says(klib, monkeypatch):
    assert L.SAMPLER_MH_COV == 12
    ok = (0, L.ERR_HIP)                                               # (without a GPU an accepted job gets as far as the device)
    assert _status() in ok                                            # swiss
    assert _status(verbose=True, period=7) in ok                      # Vanilla, verbose or not
    assert _status(monitor=MC.HIST) in ok
    for d, n in ((1, 50), (3, 40), (8, 200), (11, 70), (16, 300)):    # kinds 2 (row split) and 0, E = 2 .. 16
        X, y = cases.synthetic_logit(n, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) in ok, (d, n)
    for d in (1, 5, 16, 17, 32):                                      # whole-vector closures: plain, likelihood + prior and autodiff forms
        assert _status(target=MC.quad_target(0.5, np.eye(d))) in ok, d
        assert _status(target=MC.likprior_target(d, np.random.default_rng(d))) in ok, d
        assert _status(target=ADC.target(ADC.AD_NEGDOT, d)) in ok, d
    # 11 stays reserved, like 5, 7 and 9
    mh = dict(sampler=L.SAMPLER_MH, mh_sigma=np.ones(4), mh_factor=None)
    for s in (5, 7, 9, 11):
        assert _status(sampler=s, mh_factor=None) == L.ERR_INVALID_ARG, s
    assert _status(**mh) in ok
    # D = 33, and a logistic job beyond the row-split kernels
    assert _status(target=MC.quad_target(0.5, np.eye(33))) == L.ERR_UNSUPPORTED
    for d in (17, 20):
        X, y = cases.synthetic_logit(60, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) == L.ERR_UNSUPPORTED, d
    # pair closures, the Gaussian and hierarchical families
    assert _status(target=K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT)) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget.pairwise(20, cases.SRC_PAIR_NEGDOT)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDiagTarget.negdot(4)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDenseTarget(np.eye(4))) == L.ERR_UNSUPPORTED
    assert _status(target=cases.rats_target()) == L.ERR_UNSUPPORTED
    # more than one lane per chain
    monkeypatch.setenv("KLARA_CUSTOM_LANES", "4")
    assert _status(target=MC.quad_target(0.5, np.eye(3))) == L.ERR_UNSUPPORTED
    monkeypatch.delenv("KLARA_CUSTOM_LANES")
    # any tuner but Vanilla, and pooled tuning
    assert _status(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.3) == L.ERR_UNSUPPORTED
    assert _status(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.65, da_nadapt=8) == L.ERR_UNSUPPORTED
    assert _status(tuner=L.TUNER_ROBERTS_ROSENTHAL, targetrate=0.44) == L.ERR_UNSUPPORTED
    assert _status(tuner_mode=L.TUNE_POOLED) == L.ERR_UNSUPPORTED
    # mh_factor: required, every read entry finite, the diagonal positive, and sampler 12's alone
    assert _status(mh_factor=None) == L.ERR_INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        f = 0.3 * np.eye(4); f[2, 1] = bad
        assert _status(mh_factor=f) == L.ERR_INVALID_ARG, bad
    for bad in (0.0, -0.3, np.nan, np.inf):
        f = 0.3 * np.eye(4); f[2, 2] = bad
        assert _status(mh_factor=f) == L.ERR_INVALID_ARG, bad
    assert _status(**{**mh, "mh_factor": 0.3 * np.eye(4)}) == L.ERR_INVALID_ARG         # set together with sampler MH
    f = 0.3 * np.eye(4); f[1, 2] = np.nan                                                # above the diagonal: not read
    assert _status(mh_factor=f) in ok
    # mh_sigma is not read by sampler 12
    assert _status(mh_sigma=np.array([np.nan, -1.0, 0.0, 1.0])) in ok
    # the getter and the setter need a handle
    assert klib.klara_get_mh_factor(None, None) == L.ERR_INVALID_ARG
    assert klib.klara_set_mh_factor(None, None) == L.ERR_INVALID_ARG


def test_check_custom_target_compiles_the_new_kernels(klib):
    """klara_check_custom_target(src, KLARA_SAMPLER_MH_COV, D) compiles the MH(Σ) kernels of a user's closure for gfx950 (no GPU needed) at D = 1, 5, 16, 17, 32
    (E = 2, 8, 16, 32, 32), in the plain and the likelihood + prior form"""

    def check(src, d, sampler=L.SAMPLER_MH_COV):
        return klib.klara_check_custom_target(src.encode(), sampler, d)
    for d in (1, 5, 16, 17, 32):
        assert check(MC.SRC_QUAD, d) == 0, klib.klara_compile_log()
        assert check(MC.likprior_target(d, np.random.default_rng(d)).source, d) == 0, klib.klara_compile_log()
    assert check(ADC.target(ADC.AD_NEGDOT, 3).source, 3) == 0, klib.klara_compile_log()
    assert check(MC.SRC_QUAD, 33) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT).source, 4) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(20, cases.SRC_PAIR_NEGDOT).source, 20) == L.ERR_UNSUPPORTED
    for s in (5, 7, 9, 11):
        assert check(MC.SRC_QUAD, 3, sampler=s) == L.ERR_INVALID_ARG
    K.CustomTarget(3, MC.SRC_QUAD).check(L.SAMPLER_MH_COV)


@pytest.mark.parametrize("name", ["swiss_d4", "quad_d3", "quad_d17"])
def test_reference_with_a_diagonal_factor_is_the_oracles_mh_job(name):
    """L = diag(σ): the zero terms of a diagonal factor add exactly, so the reference reproduces OracleJob(sampler=SAMPLER_MH, mh_sigma=σ) bit for bit over the
    whole trajectory — states, log-targets, accept mask, running sums"""
    case = MC.make(name)
    n, d = 12, case["target"].ndims
    sigma = np.linspace(0.05, 0.25, d) if name == "swiss_d4" else np.linspace(0.6, 1.4, d) / np.sqrt(d)
    lay = MC.default_layout(case)
    ref = MC.ref_job(MC.with_factor(case, np.diag(sigma)), layout=lay, nchains=n, chain_offset=7, want_hist=True)
    orc = O.OracleJob(want_hist=True, **cases.oracle_kwargs(MC.as_mh(case, sigma), layout=lay, nchains=n, chain_offset=7))
    assert ref.set_state(case["x0"][:n]) == 0 and orc.set_state(case["x0"][:n]) == 0
    assert np.array_equal(ref.LT, orc.LT)
    for k in (13, case["nsteps"] - 13):
        assert ref.run(k) == 0 and orc.run(k) == 0
    assert np.array_equal(ref.accept, orc.accept) and 0.05 < ref.accept.mean() < 0.95, ref.accept.mean()
    assert np.array_equal(ref.X, orc.X) and np.array_equal(ref.LT, orc.LT)
    assert np.array_equal(ref.hist, orc.hist) and np.array_equal(ref.hist_lt, orc.hist_lt)
    assert np.array_equal(ref.sum, orc.sum) and np.array_equal(ref.sumsq, orc.sumsq) and np.array_equal(ref.naccept, orc.naccept)


@pytest.mark.parametrize("d", [3, 8])
def test_reference_first_transition_is_rams_with_the_same_factor(d):
    """a full L, D <= 8: the first transition equals the first transition of the oracle's RAM job with S0 = L — the same draws in the same order (R1)"""
    case = MC.make(f"quad_d{d}")
    n = 40
    lay = MC.default_layout(case)
    ref = MC.ref_job(case, layout=lay, nchains=n)
    ram = {k: v for k, v in case.items() if k != "mh_factor"}
    ram.update(sampler=L.SAMPLER_RAM, ram_S0=case["mh_factor"], ram_targetrate=0.234, ram_gamma=0.7)
    rj = RC.ref_job(ram, layout=lay, nchains=n)
    assert ref.set_state(case["x0"][:n]) == 0 and rj.set_state(case["x0"][:n]) == 0
    assert ref.run(1) == 0 and rj.run(1) == 0
    assert np.array_equal(ref.accept, rj.accept) and 0 < ref.accept.sum() < n
    assert np.array_equal(ref.X, rj.X) and np.array_equal(ref.LT, rj.LT)


@pytest.mark.parametrize("name", MC.CLOSURES)
def test_reference_matches_the_numpy_restatement(name):
    """full factors, 8 chains x 40 transitions at chain offset 1,000: every accept decision equal, the states within 1e-12 (the restatement's normals come
    from libm and its L z from NumPy's own summation order, a few ulp from the reference's)"""
    case = MC.make(name)
    n, off = 8, 1000
    ref = MC.ref_job(case, layout=MC.default_layout(case), nchains=n, chain_offset=off)
    assert ref.set_state(case["x0"][:n]) == 0 and ref.run(case["nsteps"]) == 0
    chains = MC.mirror_chains(case, nchains=n, chain_offset=off)
    for c in chains:
        c.run(case["nsteps"])
    acc = np.array([c.accepts for c in chains], dtype=np.uint8).T
    assert np.array_equal(acc, ref.accept), "accept decisions differ between the reference and the NumPy restatement"
    dx = np.abs(ref.X - np.array([c.x for c in chains])).max()
    dlt = np.abs(ref.LT - np.array([c.lt for c in chains])).max()
    print(f"{name}: acceptance {acc.mean():.3f}, states differ by {dx:.3e}, log-targets by {dlt:.3e}")
    assert dx <= 1e-12 and dlt <= 1e-12
    assert 0.05 < acc.mean() < 0.95                                   # the decisions are no constant
    assert np.abs(np.tril(case["mh_factor"], -1)).max() > 0.0         # ... and the factor is no diagonal


def test_tune_counts_by_hand():
    """VanillaMCTuner(period=3, verbose=true) with burn-in 5: totproposed 3 -> 6 at the first report; 6 > 5 closes no further report"""
    acc = np.array([[1], [0], [1], [1], [0], [0], [1]], np.uint8)
    a, p, t = MR.tune_counts(acc, 3, 5)
    assert (a[0], p[0], t[0]) == (2, 4, 6)
    a, p, t = MR.tune_counts(acc, 3, 100)
    assert (a[0], p[0], t[0]) == (1, 1, 9)


def test_python_constructors():
    s = K.MH(0.5)                                                     # MH(σ::Real), MH(σ::Vector): as before
    assert s.kind == L.SAMPLER_MH and np.array_equal(s.sigma, [0.5]) and s.symmetric and s.normalised and not hasattr(s, "factor")
    s = K.MH(np.array([0.5, 1.0, 2.0]))
    assert s.kind == L.SAMPLER_MH and np.array_equal(s.sigma, [0.5, 1.0, 2.0]) and s.symmetric and s.normalised and not hasattr(s, "cov")
    assert K.MH.kind == L.SAMPLER_MH
    S = np.array([[1.0, 0.9, 0.0], [0.9, 1.0, 0.2], [0.0, 0.2, 0.5]])
    s = K.MH(S)                                                       # MH(Σ::Matrix)
    assert s.kind == L.SAMPLER_MH_COV and np.array_equal(s.cov, S) and np.array_equal(s.factor, np.linalg.cholesky(S)) and s.symmetric and s.normalised
    sig = np.array([0.5, 1.0, 2.0])
    f = K.MH(np.diag(sig ** 2)).factor                                # a vector holds standard deviations, a matrix a covariance
    assert np.allclose(f, np.diag(sig), rtol=1e-15, atol=0.0)
    with pytest.raises(AssertionError, match="must be symmetric"):
        K.MH(np.array([[1.0, 0.5], [0.4, 1.0]]))
    with pytest.raises(AssertionError, match="must be a square matrix"):
        K.MH(np.ones((2, 3)))
    with pytest.raises(AssertionError, match="must be positive definite"):
        K.MH(np.array([[1.0, 2.0], [2.0, 1.0]]))
    g = K.MH.from_factor(np.array([[2.0, 7.0], [0.5, 1.0]]))          # the lower triangle is read
    assert g.kind == L.SAMPLER_MH_COV and np.array_equal(g.factor, [[2.0, 0.0], [0.5, 1.0]]) and np.array_equal(g.cov, g.factor @ g.factor.T)
    with pytest.raises(AssertionError, match="positive diagonal"):
        K.MH.from_factor(np.array([[1.0, 0.0], [0.5, 0.0]]))
    for d in (1, 4, 32):
        assert np.allclose(K.rwm_factor(np.eye(d)), 2.38 / np.sqrt(d) * np.eye(d), rtol=1e-15, atol=0.0)
    assert np.allclose(K.rwm_factor(S, scale=4.0), 2.0 * np.linalg.cholesky(S), rtol=1e-14, atol=1e-16)
    assert "rwm_factor" in K.__all__ and "MH" in K.__all__


def test_basic_mc_job_hands_the_factor_to_the_engine(monkeypatch):
    import klara_jl_amd.api as A
    seen = {}

    class FakeEngine:
        def __init__(self, **kw):
            seen.clear(); seen.update(kw)

        def set_state(self, x):
            pass

    monkeypatch.setattr(A, "Engine", FakeEngine)
    X, y = cases.swiss_data()
    p = K.BasicContMuvParameter("p", logtarget=K.LogisticTarget(X, y, 100.0))
    rng = K.BasicMCRange(nsteps=50, burnin=10)
    S = 0.01 * (np.full((4, 4), 0.5) + 0.5 * np.eye(4))
    K.BasicMCJob(K.likelihood_model(p), K.MH(S), rng, {"p": MC.SWISS_X0}, tuner=K.VanillaMCTuner(period=7, verbose=True))
    assert seen["sampler"] == L.SAMPLER_MH_COV and np.array_equal(seen["mh_factor"], np.linalg.cholesky(S))
    assert seen["tuner"] == L.TUNER_VANILLA and (seen["period"], seen["verbose"]) == (7, True)
    assert "mh_sigma" not in seen and "ram_S0" not in seen and "tuner_mode" not in seen
    K.BasicMCJob(K.likelihood_model(p), K.MH(np.full(4, 0.1)), rng, {"p": MC.SWISS_X0})       # the vector form: as before
    assert seen["sampler"] == L.SAMPLER_MH and np.array_equal(seen["mh_sigma"], np.full(4, 0.1)) and "mh_factor" not in seen
    with pytest.raises(NotImplementedError):
        K.BasicMCJob(K.likelihood_model(p), K.MH(S), rng, {"p": MC.SWISS_X0}, tuner=K.AcceptanceRateMCTuner(0.3))


def test_julia_binding_maps_the_matrix_form():
    """mechanical check of julia/KlaraHIP: the MH branch reads the proposal's covariance, takes the vector path only behind the diagonal test and the factor
    path otherwise; mhfactor and setmhfactor! are exported, one ccall each"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"const\s+SAMPLER_MH_COV\s*=\s*Int32\(12\)", src)
    m = re.search(r"elseif isa\(sampler,\s*MH\)(.*?)\n    else\n", src, re.S)
    assert m, "no MH branch in the sampler mapping"
    body = m.group(1)
    assert "Distributions.cov(prop)" in body
    i_if, i_var, i_else = body.index("\n        if "), body.index("sqrt.(Distributions.var(prop))"), body.index("\n        else")
    assert i_if < i_var < i_else and body.count("sqrt.(Distributions.var(prop))") == 1 and src.count("sqrt.(Distributions.var(prop))") == 1
    diag_test = body[i_if:body.index("\n", i_if + 1)]
    assert "i == j ||" in diag_test and "== 0" in diag_test                     # the diagonal test guards the vector path
    tail = body[i_else:]
    for f in ("SAMPLER_MH_COV", "lowerfactor(Sigma)", "kw[:mh_factor]"):
        assert f in tail, f
    assert "SAMPLER_MH_COV" not in body[:i_else] and "kw[:mh_sigma]" not in tail
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    names = {t for t in re.split(r"[,\s]+", export) if t}
    assert {"mhfactor", "setmhfactor!"} <= names
    for fn, sym in (("mhfactor", "klara_get_mh_factor"), ("setmhfactor!", "klara_set_mh_factor")):
        fm = re.search(rf"^function {re.escape(fn)}\(job::HIPMCJob.*?^end", src, re.M | re.S)
        assert fm and fm.group(0).count("ccall(") == 1 and f":{sym}" in fm.group(0), fn
        assert src.count(f":{sym}") == 1
    assert "MH with a vector or a matrix" in src                                # the sampler list of the error message
    # the struct, the keyword constructor and its positional call list the new field in the header's place
    jstruct = re.search(r"struct KlaraDesc\n(.*?)\nend", src, re.S).group(1)
    jnames = [n for n, _ in re.findall(r"(\w+)::([\w{}]+)", jstruct)]
    assert jnames == [n for n, _ in L.KlaraDesc._fields_]
    assert jnames[jnames.index("amwg_logsigma0") + 1] == "mh_factor"
    assert "mhfactor" in (ROOT / "INTEGRATION.md").read_text()


def test_header_states_the_sampler(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    assert re.search(r"KLARA_SAMPLER_MH_COV\s*=\s*12", hdr)
    assert re.search(r"#define\s+KLARA_ABI_VERSION\s+6\b", hdr) and L.KLARA_ABI_VERSION == 6 and klib.klara_abi_version() == 6
    body = hdr[hdr.index("typedef struct klara_desc"):hdr.index("} klara_desc;")]
    cnames = [n for _, n in re.findall(r"^\s{4}((?:const\s+)?\w+\*?)\s+(\w+);", body, re.M)]
    assert cnames == [n for n, _ in L.KlaraDesc._fields_] and cnames[-1] == "stream"
    assert L.KlaraDesc.mh_factor.offset == L.KlaraDesc.amwg_logsigma0.offset + 8 and L.KlaraDesc.mh_factor.size == 8
    assert L.KlaraDesc.mh_sigma.offset == 48
    for fn in ("klara_get_mh_factor", "klara_set_mh_factor"):
        assert fn in L.EXPORTS and hasattr(klib, fn) and re.search(rf"klara_status {fn}\(", hdr)
    for w in ("C1-C3", "k = 1 .. i ascending", "KLARA_ERR_UNSUPPORTED", "mh_sigma is not read"):
        assert w in hdr[hdr.index("MH(Σ::Matrix)"):hdr.index("KLARA_SAMPLER_MH_COV = 12")], w
    design = (ROOT / "DESIGN.md").read_text()
    assert "MH(Σ)" in design and "C1" in design and "C3" in design


def test_reference_is_statistically_sound():
    """N(0, Σ), D = 4, unit variances and every correlation 0.9, proposal factor rwm_factor(Σ): 64 chains started in equilibrium, 500 transitions of
    burn-in and 2,000 kept.  The pooled means and second moments lie within five standard errors of 0 and diag(Σ) = 1, the standard error taken from the
    across-chain spread of the chains' own averages (the bound of tests/test_gpu_smmala.py's whitened-MALA test); the acceptance is that of
    random-walk Metropolis at the 2.38 / sqrt(D) scaling in four dimensions, between 0.2 and 0.5."""
    d, n, burn, keep = 4, 64, 500, 2000
    target, S = MC.correlated_gaussian(d, 0.9)
    x0 = np.random.default_rng(2026).standard_normal((n, d)) @ np.linalg.cholesky(S).T
    case = dict(target=target, nchains=n, nsteps=burn + keep, burnin=burn, seed=123, **MC.mhcov(K.rwm_factor(S)))
    job = MC.ref_job(case)
    assert job.set_state(x0) == 0 and job.run(burn + keep) == 0
    m, m2 = job.sum / keep, job.sumsq / keep
    se_m, se_v = m.std(axis=0, ddof=1) / np.sqrt(n), m2.std(axis=0, ddof=1) / np.sqrt(n)
    rate = job.accept[burn:].mean()
    print(f"acceptance {rate:.3f}, pooled means {m.mean(axis=0)} (se {se_m}), second moments {m2.mean(axis=0)} (se {se_v})")
    assert np.all(np.abs(m.mean(axis=0)) <= 5.0 * se_m), (m.mean(axis=0), se_m)
    assert np.all(np.abs(m2.mean(axis=0) - np.diag(S)) <= 5.0 * se_v), (m2.mean(axis=0), se_v)
    assert 0.2 < rate < 0.5, rate
