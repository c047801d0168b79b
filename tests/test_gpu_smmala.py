"""The SMMALA kernels on the GPU: bit for bit against the CPU reference (oracle/klara_oracle.c ko_smmala), launch-length and sharding invariance,
klara_reset, the pooled tuner, and a posterior check against the MALA kernel that needs no reference."""
import numpy as np
import pytest

import cases
import klara_jl_amd as K
import smmala_cases as SC
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT | L.MON_HIST_GRAD


def _run_pair(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, runs=None):
    n = case["nchains"] if nchains is None else nchains
    x0 = case["x0"][chain_offset:chain_offset + n]
    eng = K.Engine(**SC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    job = SC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
    eng.set_state(x0)
    assert job.set_state(x0) == 0
    for k in (runs or [case["nsteps"]]):
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_same(eng, job, hist=True):
    x, lt, g = eng.state()
    assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT) and np.array_equal(g, job.G), "state differs from the reference"
    s, q, nsaved = eng.chain_sums()
    assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    step = eng.tune()[0]
    ref_step = job.step if job.step.size == job.N else np.full(job.N, job.step[0])
    assert np.array_equal(step, ref_step), "tuned steps differ"
    if hist:
        for c in (0, job.N // 2, job.N - 1):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, g_h = eng.chain_fields(c, logtarget=True, gradlogtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"
            assert np.array_equal(g_h, job.hist_g[:g_h.shape[1], c, :].T), f"gradient history of chain {c} differs"


@pytest.mark.parametrize("name", ["swiss_example", "logit_d1", "logit_d3", "logit_d8", "logit_d3_unsplit", "logit_d8_verbose",
                                  "logit_d4_thin_4099", "swiss_pooled", "bivariate_example", "custom_gauss_d3", "custom_gauss_d3_rate",
                                  "custom_gauss_d6_pooled"])
def test_bit_exact_against_the_reference(gpu_required, name):
    case = SC.make(name)
    eng, job = _run_pair(case)
    _assert_same(eng, job)
    assert 0.0 < job.accept.mean() < 1.0
    eng.close()


@pytest.mark.parametrize("monitor", [0, L.MON_ACCEPT, HIST])
def test_launch_length_does_not_change_the_bits(gpu_required, monitor):
    """steps_per_launch 1 / 7 / 32: the factor state is formed again at every launch start from x and its gradient"""
    case = SC.make("swiss_example")
    out = []
    for spl in (1, 7, 32):
        eng = K.Engine(**SC.engine_kwargs(case, monitor=monitor, steps_per_launch=spl))
        eng.set_state(case["x0"])
        eng.run(case["nsteps"])
        out.append(eng.state() + ((eng.accept_mask(),) if monitor & L.MON_ACCEPT else ()))
        eng.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)
    # ... and an untuned job, whose one-transition launches take the single-step kernel
    case = SC.make("logit_d3")
    ref = None
    for spl in (1, 7, 32):
        eng = K.Engine(**SC.engine_kwargs(case, monitor=monitor, steps_per_launch=spl))
        eng.set_state(case["x0"]); eng.run(case["nsteps"])
        st = eng.state()
        eng.close()
        if ref is None:
            ref = st
        else:
            assert all(np.array_equal(a, b) for a, b in zip(ref, st))


def test_split_runs_and_reset(gpu_required):
    case = SC.make("swiss_example")
    eng, job = _run_pair(case, runs=[13, 1, 26])
    _assert_same(eng, job)
    # reset(job): the next Philox key, the tuner rewound; the factor state follows the values
    eng.reset(); assert job.reset() == 0
    eng.run(17); assert job.run(17) == 0
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT) and np.array_equal(g, job.G)
    assert np.array_equal(eng.accept_mask(), job.accept)
    x1 = SC.SWISS_X0[None, :] + np.zeros((case["nchains"], 4))
    eng.reset(x1); assert job.reset(x1) == 0
    eng.run(9); assert job.run(9) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.accept_mask(), job.accept)
    eng.close()


def test_chain_offset_sharding(gpu_required):
    """two shards with chain_offset draw what one job of all chains draws"""
    case = SC.make("logit_d8")
    whole = K.Engine(**SC.engine_kwargs(case))
    whole.set_state(case["x0"]); whole.run(case["nsteps"])
    xw = whole.state()[0]
    whole.close()
    parts = []
    for off, n in ((0, 20), (20, case["nchains"] - 20)):
        e = K.Engine(**SC.engine_kwargs(case, chain_offset=off, nchains=n))
        e.set_state(case["x0"][off:off + n]); e.run(case["nsteps"])
        parts.append(e.state()[0]); e.close()
    assert np.array_equal(np.concatenate(parts), xw)
    eng, job = _run_pair(case, chain_offset=20, nchains=case["nchains"] - 20)
    _assert_same(eng, job)
    eng.close()


def test_nonfinite_start_state_is_refused(gpu_required):
    """a NaN start value: KLARA_ERR_NONFINITE_INIT from the SMMALA start-state kernel, and the job goes on from valid values"""
    case = SC.make("logit_d3")
    eng = K.Engine(**SC.engine_kwargs(case))
    x0 = case["x0"].copy(); x0[5, 1] = np.nan
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.set_state(case["x0"])                     # ... and the job goes on from valid values
    eng.run(3)
    eng.close()


def test_start_state_without_a_positive_definite_metric_is_refused(gpu_required):
    """DESIGN.md section 2, SMMALA deviation 5: a user's tensor that is indefinite at the start state (finite log-target and gradient)"""
    P = np.eye(3)
    bad = SC.quad_target(0.5, P, np.diag([1.0, -2.0, 1.0]))
    eng = K.Engine(sampler=L.SAMPLER_SMMALA, target=bad, nchains=5, nsteps=4, driftstep=0.5)
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(np.zeros((5, 3)))
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.close()


@pytest.mark.parametrize("fname", ["smmala_swiss", "smmala_bivariate"])
def test_goldens(gpu_required, fname):
    """tests/golden/make_golden_smmala.py: the committed reference vectors, bit for bit"""
    from pathlib import Path
    g = np.load(Path(__file__).resolve().parent / "golden" / f"{fname}.npz")
    case = SC.make({"smmala_swiss": "swiss_example", "smmala_bivariate": "bivariate_example"}[fname])
    eng = K.Engine(**SC.engine_kwargs(case))
    eng.set_state(g["x0"]); eng.run(case["nsteps"])
    x, lt, gr = eng.state()
    assert np.array_equal(eng.accept_mask(), g["accept"])
    assert np.array_equal(x, g["X"]) and np.array_equal(lt, g["LT"]) and np.array_equal(gr, g["G"])
    assert np.array_equal(eng.tune()[0], g["step"])
    eng.close()


def test_constant_metric_gaussian_is_whitened_mala(gpu_required):
    """no reference needed: on N(0, P^-1) with the metric P (D = 6, condition number 1e4), SMMALA(eps) in the coordinates y = L' x (P = L L')
    is MALA(eps) on N(0, I).  Its acceptance rate over 65,536 chains matches the MALA kernel's on the standard normal within 4 standard
    errors, and its means and variances are those of P^-1 within their Monte Carlo error."""
    d, n, steps, eps = 6, 65536, 200, 1.0
    P = SC.conditioned_precision(d, 1e4, seed=31)
    Lc = np.linalg.cholesky(P)
    z0 = np.random.default_rng(12).standard_normal((n, d))
    x0 = np.linalg.solve(Lc.T, z0.T).T                              # y0 = L' x0 = z0 ~ N(0, I): both chains start in equilibrium
    runs = {}
    for name, target, start in (("smmala", SC.quad_target(0.5, P, P), x0), ("mala", K.GaussDiagTarget.mvnormal(np.zeros(d), 1.0), z0)):
        eng = K.Engine(sampler=L.SAMPLER_SMMALA if name == "smmala" else L.SAMPLER_MALA, target=target, nchains=n, nsteps=steps,
                       driftstep=eps, monitor=L.MON_SUMMARIES, seed=4242 + len(name))
        eng.set_state(start); eng.run(steps)
        acc, _ = eng.accept_counts()
        s, q, ns = eng.chain_sums()
        eng.close()
        runs[name] = (acc / steps, s / ns, q / ns)
    a1, a2 = runs["smmala"][0], runs["mala"][0]
    se = np.sqrt(a1.var(ddof=1) / n + a2.var(ddof=1) / n)
    assert abs(a1.mean() - a2.mean()) < 4.0 * se, f"acceptance {a1.mean():.4f} (SMMALA) vs {a2.mean():.4f} (MALA), se {se:.2e}"
    _, m, m2 = runs["smmala"]
    cov = np.linalg.inv(P)
    assert np.all(np.abs(m.mean(axis=0)) < 5.0 * m.std(axis=0, ddof=1) / np.sqrt(n)), "means differ from 0"
    v = m2.mean(axis=0)
    assert np.all(np.abs(v - np.diag(cov)) < 5.0 * m2.std(axis=0, ddof=1) / np.sqrt(n)), f"variances {v} vs {np.diag(cov)}"
    assert np.linalg.cond(P) > 0.99e4                              # (the scales the metric has to take out: eigenvalues 1 .. 1e4)


def test_swiss_posterior_means_agree_with_mala(gpu_required):
    """no reference needed: SMMALA (the swiss example's AcceptanceRateMCTuner(0.5) during burn-in) and cfg 4's MALA kernel (driftstep 0.1)
    sample the same swiss posterior from the example's start; each pooled mean's Monte Carlo error is the batch-means variance
    (mcvar(:bm), streaming, 20 batches of 50) of every chain, summed over the chains"""
    X, y = cases.swiss_data()
    n, burn, keep = 16384, 1000, 1000
    x0 = SC.SWISS_X0[None, :] + 0.05 * np.random.default_rng(9).standard_normal((n, 4))
    res = {}
    for sampler, kw in ((L.SAMPLER_SMMALA, dict(driftstep=0.02, tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5)), (L.SAMPLER_MALA, dict(driftstep=0.1))):
        eng = K.Engine(sampler=sampler, target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=burn + keep, burnin=burn,
                       monitor=L.MON_SUMMARIES, bm_batchlen=50, seed=77 + sampler, **kw)
        eng.set_state(x0); eng.run(burn + keep)
        s, _, ns = eng.chain_sums()
        bm, nb = eng.chain_bm()
        acc, _ = eng.accept_counts()
        eng.close()
        assert nb == keep // 50
        res[sampler] = ((s / ns).mean(axis=0), np.sqrt(bm.sum(axis=0)) / n, acc.mean() / (burn + keep))
    (m1, e1, a1), (m2, e2, a2) = res[L.SAMPLER_SMMALA], res[L.SAMPLER_MALA]
    assert 0.2 < a1 < 0.99 and 0.2 < a2 < 0.99
    z = np.abs(m1 - m2) / np.sqrt(e1 ** 2 + e2 ** 2)
    assert np.all(z < 5.0), f"posterior means differ: SMMALA {m1}, MALA {m2}, z {z}"
