"""The SMMALA kernels with the softabs transform of the metric on the GPU: bit for bit against the CPU reference (oracle/klara_oracle.c ko_smmala),
launch-length, split-run and sharding invariance (a chain does not depend on its wavefront neighbours), non-finite metrics, the two routes to the
BivariateNormal example, and a posterior check against the MALA kernel that needs no reference."""
from pathlib import Path

import numpy as np
import pytest

import autodiff_cases as AC
import klara_jl_amd as K
import smmala_cases as SC
import softabs_cases as SAC
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT | L.MON_HIST_GRAD
GOLDEN = Path(__file__).resolve().parent / "golden"


def _run_pair(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, runs=None):
    n = case["nchains"] if nchains is None else nchains
    x0 = case["x0"][chain_offset:chain_offset + n]
    eng = K.Engine(**SAC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    job = SAC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
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


def _final(case, monitor=L.MON_ACCEPT, **kw):
    n = kw.get("nchains", case["nchains"])
    off = kw.get("chain_offset", 0)
    eng = K.Engine(**SAC.engine_kwargs(case, monitor=monitor, **kw))
    eng.set_state(case["x0"][off:off + n]); eng.run(case["nsteps"])
    out = eng.state() + ((eng.accept_mask(),) if monitor & L.MON_ACCEPT else ())
    eng.close()
    return out


@pytest.mark.parametrize("name", SAC.NAMES)
def test_bit_exact_against_the_reference(gpu_required, name):
    case = SAC.make(name)
    eng, job = _run_pair(case)
    _assert_same(eng, job)
    assert 0.0 < job.accept.mean() < 1.0
    eng.close()


@pytest.mark.parametrize("name", ["doublewell_d3", "doublewell_d8", "banana_ad2"])
def test_launch_length_does_not_change_the_bits(gpu_required, name):
    """steps_per_launch 1 / 7 / 32 (a tuned job, a verbose one, and an untuned one whose one-transition launches take the single-step kernel)"""
    case = SAC.make(name)
    for monitor in (0, HIST):
        out = [_final(case, monitor=monitor, steps_per_launch=spl) for spl in (1, 7, 32)]
        for o in out[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(out[0], o))


def test_split_runs_and_reset(gpu_required):
    case = SAC.make("doublewell_d3")
    eng, job = _run_pair(case, runs=[13, 1, 16])
    _assert_same(eng, job)
    whole = _final(case)
    assert all(np.array_equal(a, b) for a, b in zip(eng.state(), whole[:3])), "split runs differ from a single run"
    # reset(job): the next Philox key, the tuner rewound; the transformed factor state follows the values
    eng.reset(); assert job.reset() == 0
    eng.run(17); assert job.run(17) == 0
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT) and np.array_equal(g, job.G)
    assert np.array_equal(eng.accept_mask(), job.accept)
    x1 = np.zeros((case["nchains"], 3))                              # the origin: minus the Hessian is negative definite there
    eng.reset(x1); assert job.reset(x1) == 0
    eng.run(9); assert job.run(9) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.accept_mask(), job.accept)
    eng.close()


def test_a_chain_does_not_depend_on_its_wavefront_neighbours(gpu_required):
    """mixed_4099: lanes of one wavefront stop after different numbers of sweeps.  Chains 0 .. 4,098 in one handle = two handles with chain_offset;
    and 100 chains from the middle, alone in their own wavefronts, take the same bits"""
    case = SAC.make("mixed_4099")
    xw, ltw, gw, accw = _final(case)
    parts = [_final(case, chain_offset=off, nchains=n) for off, n in ((0, 2000), (2000, case["nchains"] - 2000))]
    for k, whole in enumerate((xw, ltw, gw)):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole)
    assert np.array_equal(np.concatenate([p[3] for p in parts], axis=1), accw)
    xs, lts, gs, accs = _final(case, chain_offset=1717, nchains=100)
    assert np.array_equal(xs, xw[1717:1817]) and np.array_equal(lts, ltw[1717:1817]) and np.array_equal(gs, gw[1717:1817])
    assert np.array_equal(accs, accw[:, 1717:1817])
    eng, job = _run_pair(case, chain_offset=1717, nchains=100)
    _assert_same(eng, job)
    eng.close()


# N(0, I) whose tensor carries a NaN off the diagonal where x_0 > data[0]
SRC_NAN_METRIC = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + x[i] * x[i];
    return -0.5 * s;
}
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    for (int i = 0; i < KLARA_D; ++i) g[i] = -x[i];
}
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G)
{
    for (int k = 0; k < KLARA_D * KLARA_D; ++k) G[k] = 0.0;
    for (int i = 0; i < KLARA_D; ++i) G[i * KLARA_D + i] = (i & 1) ? -1.0 : 1.0;
    G[0 * KLARA_D + (KLARA_D - 1)] = x[0] > data[0] ? kd_u2d(0x7ff8000000000000ull) : 0.25;
}
"""


def _nan_case(threshold, x0):
    n, d = x0.shape
    return dict(sampler=L.SAMPLER_SMMALA, target=K.CustomTarget(d, SRC_NAN_METRIC, data=np.array([threshold])), nchains=n, nsteps=30, driftstep=0.9,
                smmala_softabs=2.0, x0=x0, name="nan_metric")


def test_start_state_with_a_nan_metric_entry_is_refused(gpu_required):
    x0 = np.zeros((37, 3)); x0[11, 0] = 6.0
    case = _nan_case(5.0, x0)
    eng = K.Engine(**SAC.engine_kwargs(case))
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT                    # the transform does not turn the NaN into a finite matrix (T4, S5)
    assert SAC.ref_job(case, layout=eng.layout()).set_state(x0) == L.ERR_NONFINITE_INIT
    x0[11, 0] = 0.0
    eng.set_state(x0); eng.run(3)                                     # ... and the job goes on from valid values
    eng.close()


def test_proposal_with_a_nan_metric_is_rejected(gpu_required):
    x0 = 0.3 * np.random.default_rng(5).standard_normal((37, 3))
    case = _nan_case(0.6, x0)                                         # a good share of the proposals land where the metric is not finite
    eng, job = _run_pair(case)
    _assert_same(eng, job)                                            # rejected (S4), and the chain goes on
    assert np.all(eng.state()[0][:, 0] <= 0.6) and 0.0 < job.accept.mean() < 1.0
    free = _final(_nan_case(1e9, x0))
    assert np.any(free[0][:, 0] > 0.6), "without the NaN region the same chains do go there"
    eng.close()


def test_bivariate_device_against_the_host_formed_golden(gpu_required):
    """smmala_bivariate.npz was made with softabs(-2C) formed on the host and handed over as data; here the tensor is the raw -2C and the device
    transforms it: the two routes to the same job take the same decisions and agree to 1e-9 over its 40 steps"""
    g = np.load(GOLDEN / "smmala_bivariate.npz")
    case = SAC.make("bivariate_device")
    eng = K.Engine(**SAC.engine_kwargs(case))
    eng.set_state(g["x0"]); eng.run(case["nsteps"])
    x, lt, gr = eng.state()
    assert np.array_equal(eng.accept_mask(), g["accept"])
    np.testing.assert_allclose(x, g["X"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(lt, g["LT"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(gr, g["G"], rtol=0, atol=1e-9)
    eng.close()


def test_without_the_transform_nothing_changes(gpu_required):
    """smmala_softabs = 0: existing SMMALA jobs return the bits they returned before (their committed vectors)"""
    for fname, name in (("smmala_swiss", "swiss_example"), ("smmala_bivariate", "bivariate_example")):
        g = np.load(GOLDEN / f"{fname}.npz")
        case = SC.make(name)
        eng = K.Engine(**SC.engine_kwargs(case, smmala_softabs=0.0))
        eng.set_state(g["x0"]); eng.run(case["nsteps"])
        x, lt, gr = eng.state()
        assert np.array_equal(eng.accept_mask(), g["accept"])
        assert np.array_equal(x, g["X"]) and np.array_equal(lt, g["LT"]) and np.array_equal(gr, g["G"]) and np.array_equal(eng.tune()[0], g["step"])
        eng.close()


def test_banana_start_is_refused_without_the_transform(gpu_required):
    case = SAC.make("banana_ad2")
    eng = K.Engine(**SAC.engine_kwargs(case, smmala_softabs=0.0))
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(case["x0"])
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.close()


@pytest.mark.parametrize("fname", ["softabs_banana", "softabs_doublewell_d8", "softabs_diag_d4"])
def test_goldens(gpu_required, fname):
    """tests/golden/make_golden_softabs.py: the committed reference vectors, bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_softabs", GOLDEN / "make_golden_softabs.py")
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    g = np.load(GOLDEN / f"{fname}.npz")
    case = SAC.make(mg.GOLDEN[fname])
    eng = K.Engine(**SAC.engine_kwargs(case))
    eng.set_state(g["x0"]); eng.run(case["nsteps"])
    x, lt, gr = eng.state()
    assert np.array_equal(eng.accept_mask(), g["accept"])
    assert np.array_equal(x, g["X"]) and np.array_equal(lt, g["LT"]) and np.array_equal(gr, g["G"])
    assert np.array_equal(eng.tune()[0] if g["step"].size > 1 else eng.tune()[0][:1], g["step"])
    eng.close()


def test_banana_posterior_means_agree_with_mala(gpu_required):
    """no reference needed: SMMALA with softabs(., 20) of minus the Hessian, 4,096 chains x 2,000 steps after burn-in, and the MALA kernel sample the same
    autodiff banana (x_0 ~ N(1, 10), x_1 | x_0 ~ N(x_0^2, 1/2): means 1 and 11); the error of each pooled mean is the streaming batch-means variance
    (mcvar(:bm)) of every chain, summed over the chains, and the two must agree within 5 standard errors, as test_gpu_smmala's swiss check.
    Both start from exact draws of the target, so neither pooled mean carries a start-up bias.  What the batch means have to see is the chains' autocorrelation,
    and on this target that is long (a NumPy restatement of both samplers, 4,096 chains from the same start, measured the honest across-chain error of the
    pooled means next to the batch-means one):
      * MALA does not mix on this target: in the narrow tails of the ridge (|x_0| beyond 3 or 4) it needs h < 0.005 to move at all.  Over 2,000 steps at
        h = 0.4 / 0.1 / 0.03 / 0.01 the across-chain error of its pooled mean was that of ONE independent draw per chain (0.047, 0.25) while 20 batches of 100
        claimed (0.003, 0.007); over 200,000 steps at h = 0.03 it was (0.030, 0.19) against (0.0074, 0.030) from 20 batches of 10,000, and 400,000 steps at
        h = 0.005 or 0.002 mixed no better.  Its run here is that 200,000-step one, the longest a test can afford; its batch-means error is understated about
        fourfold.  An understated error inflates z: it makes this check stricter than its 5 standard errors say, never weaker.
      * SMMALA with a = 1 caps the step along the ridge (1 / a is the smallest metric eigenvalue) and mixed as slowly; with a = 20, h = 1 its across-chain error
        was (0.021, 0.087) against (0.016, 0.072) from 4 batches of 500: the batch means still fall short by a fifth, so 5 of these standard errors are 4
        honest ones.  That is the configuration here.  Measured on the device: SMMALA (0.984, 10.88) +- (0.016, 0.072), MALA (1.009, 10.90) +- (0.007, 0.030),
        z = (1.4, 0.3)."""
    n, burn, keep = 4096, 200, 2000
    rng = np.random.default_rng(9)
    x00 = 1.0 + np.sqrt(10.0) * rng.standard_normal(n)
    x0 = np.stack([x00, x00 * x00 + np.sqrt(0.5) * rng.standard_normal(n)], axis=1)
    res = {}
    for sampler, target, keep_s, batch, kw in ((L.SAMPLER_SMMALA, AC.target(AC.AD_BANANA, 2, order=2), keep, 500, dict(driftstep=1.0, smmala_softabs=20.0)),
                                               (L.SAMPLER_MALA, AC.target(AC.AD_BANANA, 2), 100 * keep, 10000, dict(driftstep=0.03, steps_per_launch=1000))):
        eng = K.Engine(sampler=sampler, target=target, nchains=n, nsteps=burn + keep_s, burnin=burn, monitor=L.MON_SUMMARIES, bm_batchlen=batch,
                       seed=77 + sampler, **kw)
        eng.set_state(x0); eng.run(burn + keep_s)
        s, _, ns = eng.chain_sums()
        bm, nb = eng.chain_bm()
        acc, _ = eng.accept_counts()
        eng.close()
        assert nb == keep_s // batch and np.all(ns == keep_s)
        res[sampler] = ((s / ns).mean(axis=0), np.sqrt(bm.sum(axis=0)) / n, acc.mean() / (burn + keep_s))
    (m1, e1, a1), (m2, e2, a2) = res[L.SAMPLER_SMMALA], res[L.SAMPLER_MALA]
    z = np.abs(m1 - m2) / np.sqrt(e1 ** 2 + e2 ** 2)
    print(f"banana: SMMALA+softabs means {m1} +- {e1} (acceptance {a1:.3f}), MALA {m2} +- {e2} (acceptance {a2:.3f}), z {z}")
    assert 0.2 < a1 < 0.99 and 0.2 < a2 < 0.99
    assert np.all(z < 5.0), f"posterior means differ: SMMALA {m1}, MALA {m2}, z {z}"
