"""The MH(Σ) kernels (KLARA_SAMPLER_MH_COV) on the GPU: against the MH kernels with a diagonal factor (no reference between them), bit for bit against the
CPU reference (tests/mhcov_ref.py) on full factors — every E with D < E and D = E, the logistic target on both its layouts, 70 and 130 chains, two chain
offsets, the three launch forms — and on the non-finite MH jobs of tests/nonfinite_cases.py, against the RAM kernels' first transition, the factor's getter,
setter and reset, monitored against unmonitored chains, and a statistical check on a correlated Gaussian.  Small shapes: 70 chains (one full and one
partial wavefront at a chain per lane) and 130, 40 transitions, burn-in 5, thinning 2.  A case's reference is computed once (mhcov_cases.reference) on 130
chains and shared: chain c draws from stream offset + c, so a 70-chain job is its first 70 chains."""
import numpy as np
import pytest

import cases
import klara_jl_amd as K
import mhcov_cases as MC
import mhcov_ref as MR
import nonfinite_cases as NF
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = MC.HIST


def _engine(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, **over):
    n = case["nchains"] if nchains is None else nchains
    eng = K.Engine(**MC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n, **over))
    eng.set_state(case["x0"][:n])
    return eng


def _snapshot(eng, monitor=HIST, chains=()):
    x, lt, _ = eng.state()
    out = dict(X=x, LT=lt, naccept=eng.accept_counts()[0])
    if monitor & L.MON_ACCEPT:
        out["accept"] = eng.accept_mask()
    if monitor & L.MON_SUMMARIES:
        out["sum"], out["sumsq"], _ = eng.chain_sums()
    if monitor & L.MON_HISTORY:
        out["hist"] = [eng.chain(c) for c in chains]
        out["hist_lt"] = [eng.chain_fields(c, logtarget=True)[0] for c in chains]
    return out


def _assert_same(eng, job, n, monitor=HIST):
    """the engine's n chains against the first n chains of the reference"""
    chains = sorted({0, n // 2, n - 1})
    g = _snapshot(eng, monitor, chains)
    assert np.array_equal(g["X"], job.X[:n]) and np.array_equal(g["LT"], job.LT[:n]), "state differs from the reference"
    assert np.array_equal(g["naccept"], job.naccept[:n]) and eng.accept_counts()[1] == job.t
    if monitor & L.MON_ACCEPT:
        assert np.array_equal(g["accept"], job.accept[:, :n]), "accept mask differs from the reference"
    if monitor & L.MON_SUMMARIES:
        assert np.array_equal(g["sum"], job.sum[:n]) and np.array_equal(g["sumsq"], job.sumsq[:n]), "running sums differ from the reference"
    if monitor & L.MON_HISTORY:
        for c, v, h in zip(chains, g["hist"], g["hist_lt"]):
            assert v.shape[1] > 0 and np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            assert np.array_equal(h, job.hist_lt[:h.size, c]), f"log-target history of chain {c} differs"


# ---------------------------------------------------------------- 8: against MH, with no reference between them
DIAG_CASES = ["swiss_d4", "logit_d9", "quad_d3", "quad_d17", "quad_d32"]      # kind 2; kind 0 at E = 16; closures at E = 4, 32, 32


@pytest.mark.parametrize("spl", [0, 1, 7])
@pytest.mark.parametrize("name", DIAG_CASES)
def test_diagonal_factor_is_the_mh_kernel(gpu_required, name, spl):
    """mh_factor = diag(σ) against the MH job with mh_sigma = σ: the same bits in the final state, log-target, accept mask, running sums and value history"""
    case = MC.make(name)
    n, d = 70, case["target"].ndims
    sigma = np.linspace(0.05, 0.25, d) if name == "swiss_d4" else np.linspace(0.1, 0.2, d) if name == "logit_d9" else np.linspace(0.6, 1.4, d) / np.sqrt(d)
    chains = (0, 35, 69)
    got = []
    for c in (MC.with_factor(case, np.diag(sigma)), MC.as_mh(case, sigma)):
        eng = _engine(c, steps_per_launch=spl, nchains=n)
        if name in ("swiss_d4", "logit_d9"):
            assert eng.layout() == {"swiss_d4": (2, 4, 4), "logit_d9": (0, 1, 16)}[name]
        else:
            assert eng.layout() == (0, 1, max(2, 1 << (d - 1).bit_length()))
        eng.run(case["nsteps"])
        got.append(_snapshot(eng, HIST, chains))
        eng.close()
    a, b = got
    for k in ("X", "LT", "naccept", "accept", "sum", "sumsq"):
        assert np.array_equal(a[k], b[k]), f"{k} differs between the diag(σ)-factor job and the MH job"
    for va, vb, ha, hb in zip(a["hist"], b["hist"], a["hist_lt"], b["hist_lt"]):
        assert va.shape[1] == 18 and np.array_equal(va, vb) and np.array_equal(ha, hb)
    assert 0.05 < a["accept"].mean() < 0.95, a["accept"].mean()


# ---------------------------------------------------------------- 9: against the reference, full factors
FORMS = {"nomon": dict(monitor=0, steps_per_launch=1),                          # nothing monitored, one transition per launch: the COMMIT = false path, straight to memory
         "plain": dict(monitor=HIST, steps_per_launch=0),
         "verbose": dict(monitor=HIST, steps_per_launch=0, verbose=True, period=7)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n,off", [(70, 0), (130, 0), (70, 1000), (130, 1000)])
@pytest.mark.parametrize("name", MC.ALL)
def test_bit_exact_against_the_reference(gpu_required, name, n, off, form):
    case = MC.make(name)
    kw = FORMS[form]
    eng = _engine(case, chain_offset=off, nchains=n, **kw)
    assert eng.layout() == MC.default_layout(case), (eng.layout(), MC.default_layout(case))
    job = MC.reference(name, off)
    eng.run(case["nsteps"])
    _assert_same(eng, job, n, monitor=kw["monitor"])
    if form == "verbose":                                             # Vanilla counts as it does for MH
        _, a, p, t = eng.tune()
        ea, ep, et = MR.tune_counts(job.accept[:, :n], 7, case["burnin"])
        assert np.array_equal(a, ea) and np.array_equal(p, ep) and np.array_equal(t, et)
    eng.close()
    # a kernel that drops the off-diagonals, never moves or always moves cannot pass
    assert np.abs(np.tril(case["mh_factor"], -1)).max() > 0.0 and 0.05 < job.accept.mean() < 0.95
    assert case["burnin"] > 1 and case["thinning"] > 1


@pytest.mark.parametrize("spl", [0, 7])
@pytest.mark.parametrize("name", ["quad_d5", "quad_d32", "logit_d11"])
def test_monitored_launch_lengths(gpu_required, name, spl):
    """every monitor with launches of any length and of 7 transitions: the folds do not depend on the cut"""
    case = MC.make(name)
    eng = _engine(case, steps_per_launch=spl, nchains=130)
    for k in (13, case["nsteps"] - 13):
        eng.run(k)
    _assert_same(eng, MC.reference(name, 0), 130)
    eng.close()


@pytest.mark.parametrize("name", ["closure_gamma_inf_mh", "closure_gamma_nan_mh", "logit_swiss_mh"])
def test_non_finite_proposals_are_rejected_as_the_reference_rejects_them(gpu_required, name):
    """the MH jobs of tests/nonfinite_cases.py that lie in this sampler's scope, run with mh_factor = diag(mh_sigma): a proposal whose log-target is NaN or
    -inf is rejected, nothing of it survives, and the job equals the reference bit for bit"""
    job = NF.jobs()[name]
    kw = {k: v for k, v in job["kw"].items() if k not in ("sampler", "mh_sigma")}
    case = dict(nchains=job["n"], nsteps=job["nsteps"], seed=NF.SEED, x0=job["x0"], **kw, **MC.mhcov(np.diag(job["kw"]["mh_sigma"])))
    ref = MC.ref_job(case, layout=job["layout"], want_hist=True)
    assert ref.set_state(job["x0"]) == 0 and ref.run(job["nsteps"]) == 0
    for spl in job["spl"]:
        eng = _engine(case, steps_per_launch=spl)
        assert tuple(eng.layout()) == job["layout"]
        eng.run(job["nsteps"])
        _assert_same(eng, ref, job["n"])
        assert np.all(np.isfinite(eng.state()[0])) and np.all(np.isfinite(eng.state()[1]))
        eng.close()
    assert 0.0 < ref.accept.mean() < 1.0


# ---------------------------------------------------------------- 10: against RAM
@pytest.mark.parametrize("d", [3, 8])
def test_first_transition_is_rams_with_the_same_factor(gpu_required, d):
    """one transition with S0 = L: the state and the accept mask of the RAM job (its factor update comes after the decision)"""
    case = MC.make(f"quad_d{d}")
    n = 70
    ram = {k: v for k, v in case.items() if k != "mh_factor"}
    ram.update(sampler=L.SAMPLER_RAM, ram_S0=case["mh_factor"], ram_targetrate=0.234, ram_gamma=0.7)
    got = []
    for c in (case, ram):
        eng = _engine(c, monitor=L.MON_ACCEPT, nchains=n)
        eng.run(1)
        got.append(_snapshot(eng, L.MON_ACCEPT))
        eng.close()
    a, b = got
    assert np.array_equal(a["accept"], b["accept"]) and 0 < a["accept"].sum() < n
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["LT"], b["LT"])


# ---------------------------------------------------------------- 11: the factor's getter, setter and reset
def test_factor_getter_setter_reset_and_set_state(gpu_required):
    name = "quad_d9"
    case = MC.make(name)
    n, k1 = 70, 17
    f0 = np.tril(case["mh_factor"])
    f1 = MC.full_factor(9, 991, scale=0.1)
    noisy = f1 + np.triu(np.full((9, 9), np.nan), 1)                  # above the diagonal: not read, zeros come back
    eng = _engine(case, nchains=n)
    assert np.array_equal(eng.mh_factor(), f0)
    ref = MC.ref_job(case, layout=eng.layout(), nchains=n, want_hist=True)
    assert ref.set_state(case["x0"][:n]) == 0
    eng.run(k1); assert ref.run(k1) == 0
    bad = f1.copy(); bad[4, 4] = 0.0
    with pytest.raises(K.KlaraError) as e:
        eng.set_mh_factor(bad)
    assert e.value.status == L.ERR_INVALID_ARG and np.array_equal(eng.mh_factor(), f0)
    eng.set_mh_factor(noisy); ref.set_factor(f1)                      # in effect from transition k1 on
    assert np.array_equal(eng.mh_factor(), f1)
    eng.run(case["nsteps"] - k1); assert ref.run(case["nsteps"] - k1) == 0
    _assert_same(eng, ref, n)
    assert not np.array_equal(ref.X, MC.reference(name, 0).X[:n])     # ... and the switch mattered
    # klara_set_state keeps the factor
    eng.set_state(case["x0"][:n]); assert ref.set_state(case["x0"][:n]) == 0
    assert np.array_equal(eng.mh_factor(), f1)
    eng.run(11); assert ref.run(11) == 0
    _assert_same(eng, ref, n)
    # klara_reset puts the descriptor's factor back; the run after it equals a fresh job's on the next key
    eng.reset(case["x0"][:n]); assert ref.reset(case["x0"][:n]) == 0
    assert np.array_equal(eng.mh_factor(), f0)
    eng.run(case["nsteps"]); assert ref.run(case["nsteps"]) == 0
    _assert_same(eng, ref, n)
    key, epoch = eng.stream_key()
    eng.close()
    fresh = _engine(dict(case, seed=key), nchains=n)
    fresh.run(case["nsteps"])
    _assert_same(fresh, ref, n)
    fresh.close()
    # the setter on a job in flight takes effect behind the transitions queued before it
    eng = _engine(case, nchains=n, monitor=0)
    eng.run_async(k1); eng.set_mh_factor(f1); eng.run_async(case["nsteps"] - k1); eng.synchronize()
    ref2 = MC.ref_job(case, layout=eng.layout(), nchains=n)
    assert ref2.set_state(case["x0"][:n]) == 0 and ref2.run(k1) == 0
    ref2.set_factor(f1); assert ref2.run(case["nsteps"] - k1) == 0
    _assert_same(eng, ref2, n, monitor=0)
    # another sampler's handle has no factor
    eng.close()
    mh = _engine(MC.as_mh(case, np.full(9, 0.1)), nchains=n)
    for call in (mh.mh_factor, lambda: mh.set_mh_factor(f1)):
        with pytest.raises(K.KlaraError) as e:
            call()
        assert e.value.status == L.ERR_INVALID_ARG
    mh.close()


# ---------------------------------------------------------------- 12: monitored and unmonitored chains
@pytest.mark.parametrize("name", ["swiss_d4", "quad_d17"])
def test_monitored_and_unmonitored_chains_are_the_same_bits(gpu_required, name):
    case = MC.make(name)
    got = []
    for mon, spl in ((HIST, 0), (0, 0), (0, 1), (L.MON_ACCEPT, 7)):
        eng = _engine(case, monitor=mon, steps_per_launch=spl)
        eng.run(case["nsteps"])
        got.append(_snapshot(eng, 0))
        eng.close()
    for g in got[1:]:
        assert np.array_equal(g["X"], got[0]["X"]) and np.array_equal(g["LT"], got[0]["LT"]) and np.array_equal(g["naccept"], got[0]["naccept"])


# ---------------------------------------------------------------- 13: statistics
def test_correlated_gaussian_is_sampled_with_the_right_mean_and_covariance(gpu_required):
    """N(0, Σ), D = 8, unit variances and every correlation 0.9, proposal factor rwm_factor(Σ): 4,096 chains started in equilibrium, 600 transitions, burn-in
    200.  The pooled mean and every entry of the pooled covariance (accumulated on the device: the monitor bit of covariance=True) lie within five standard
    errors of 0 and Σ.  The standard error of an entry is the across-chain spread of the chains' own averages over sqrt(chains): of x_i from every chain's
    running sums, of x_i x_j from the value histories of every eighth chain (512 chains give the spread to 3 %; reading 4,096 histories one by one would
    take longer than the job)."""
    d, n, steps, burn = 8, 4096, 600, 200
    target, S = MC.correlated_gaussian(d, 0.9)
    x0 = np.random.default_rng(88).standard_normal((n, d)) @ np.linalg.cholesky(S).T
    eng = K.Engine(target=target, nchains=n, nsteps=steps, burnin=burn, seed=2027, monitor=L.MON_SUMMARIES | L.MON_HISTORY | L.MON_COVARIANCE,
                   **MC.mhcov(K.rwm_factor(S)))
    eng.set_state(x0); eng.run(steps)
    mean, m2, ns, nch = eng.pooled_covariance()
    cov = m2 / (ns - 1)
    assert ns == n * (steps - burn) and nch == n
    s, q, k = eng.chain_sums()
    rate = eng.accept_counts()[0].mean() / steps
    sub = np.arange(0, n, 8)                                          # the chains' own averages of x_i x_j, from the device's value history
    prod = np.empty((sub.size, d, d))
    for j, c in enumerate(sub):
        v = eng.chain(int(c))                                         # (D, saved)
        prod[j] = (v @ v.T) / v.shape[1]
    eng.close()
    m = s / k
    se_m = m.std(axis=0, ddof=1) / np.sqrt(n)
    se_c = prod.std(axis=0, ddof=1) / np.sqrt(n)
    print(f"acceptance {rate:.3f}; pooled mean {mean}; se {se_m}; largest covariance error {np.abs(cov - S).max():.4f} (se up to {se_c.max():.4f})")
    assert np.allclose(mean, m.mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(np.einsum("cii->ci", prod), (q / k)[sub], rtol=1e-12, atol=0)      # the histories are the chains the sums come from
    assert np.all(np.abs(mean) <= 5.0 * se_m), (mean, se_m)
    assert np.all(np.abs(cov - S) <= 5.0 * se_c), (np.abs(cov - S).max(), se_c.max())
    assert 0.15 < rate < 0.45, rate
