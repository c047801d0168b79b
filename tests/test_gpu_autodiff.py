"""Forward-mode autodiff of user-defined targets on the GPU (KLARA_USER_AUTODIFF, klara.jl_amd/csrc/klara_autodiff.h): bit for bit against the host build
of the same header (tests/autodiff_ref.py) stepped by the CPU oracle and the SMMALA reference, against the hand-written gradients on the device, and
invariant under launch length, sharding and the width of a sweep."""
import ctypes as C

import numpy as np
import pytest

import autodiff_cases as A
import autodiff_ref as R
import cases
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

SUMS = L.MON_ACCEPT | L.MON_SUMMARIES
HIST = SUMS | L.MON_HISTORY | L.MON_HIST_LT | L.MON_HIST_GRAD
NOGRAD = (L.SAMPLER_MH, L.SAMPLER_SLICE)


def _monitor(case):
    return (HIST & ~L.MON_HIST_GRAD) if case["sampler"] in NOGRAD else HIST


def _run_pair(case, monitor=None, steps_per_launch=0, chain_offset=0, nchains=None):
    monitor = _monitor(case) if monitor is None else monitor
    n = case["nchains"] if nchains is None else nchains
    x0 = case["x0"][chain_offset:chain_offset + n]
    eng = K.Engine(**cases.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    job = R.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
    eng.set_state(x0)
    assert job.set_state(x0) == 0
    eng.run(case["nsteps"])
    assert job.run(case["nsteps"]) == 0
    return eng, job


def _assert_same(eng, job, hist=True, grad=True):
    x, lt, g = eng.state()
    assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    if grad:
        assert np.array_equal(g, job.G), "gradient differs from the reference"
    s, q, _ = eng.chain_sums()
    assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    step = eng.tune()[0]
    ref_step = job.step if job.step.size == job.N else np.full(job.N, job.step[0])
    assert np.array_equal(step, ref_step, equal_nan=True), "tuned steps differ"           # (the slice sampler has no step: NaN on both sides)
    if hist:
        for c in (0, job.N // 2, job.N - 1):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, g_h = eng.chain_fields(c, logtarget=True, gradlogtarget=grad)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"
            if grad:
                assert np.array_equal(g_h, job.hist_g[:g_h.shape[1], c, :].T), f"gradient history of chain {c} differs"


LAYOUTS = {"mala_negdot_d33": (4, 10), "mala_negdot_d100": (8, 14), "mala_negdot_d520": (64, 10), "hmc_quartic_d33": (4, 10), "hmc_quartic_d100": (8, 14)}


# ---- 7. bit for bit against the host build
@pytest.mark.parametrize("name", ["mala_negdot_d2", "mala_negdot_d3", "mala_negdot_d9", "mala_negdot_d32", "mala_negdot_d33", "mala_negdot_d100",
                                  "mala_negdot_d520", "mala_banana", "mala_logit_swiss_rate", "mala_logit_swiss_pooled", "hmc_quartic_d33",
                                  "hmc_quartic_d100", "hmc_erf", "hmc_logit_d9_da", "mh_banana", "slice_banana", "smmala_logit_swiss", "smmala_gauss_d3"])
def test_bit_exact_against_the_host_build(gpu_required, name):
    case = A.make(name)
    eng, job = _run_pair(case)
    if name in LAYOUTS:
        assert eng.layout()[1:] == LAYOUTS[name]           # staged: G lanes per chain, E elements per lane
    else:
        assert eng.layout()[1] == 1                        # one chain per lane
    _assert_same(eng, job, grad=case["sampler"] not in NOGRAD)
    if case["sampler"] == L.SAMPLER_SLICE:
        assert job.accept.mean() == 1.0                    # (a slice transition always moves: there is nothing to reject)
    else:
        assert 0.0 < job.accept.mean() < 1.0
    eng.close()


def test_likelihood_prior_form_with_its_monitors(gpu_required):
    """two evaluations composed as klara_custom_compose.h does; the :loglikelihood / :logprior histories are the double instantiations"""
    case = A.make("mala_nn_parts")
    eng, job = _run_pair(case, monitor=HIST | L.MON_HIST_LLLP)
    _assert_same(eng, job)
    assert 0.0 < job.accept.mean() < 1.0
    t = case["target"]
    lib = R.build(t.source, t.ndims)
    dp = C.POINTER(C.c_double)
    for f in (lib.klara_user_loglikelihood, lib.klara_user_logprior):
        f.restype, f.argtypes = C.c_double, [dp, C.c_int, dp, C.c_longlong]
    for c in (0, case["nchains"] - 1):
        v = eng.chain(c); lt_h, _ = eng.chain_fields(c); ll, lp = eng.chain_likelihood_prior(c)
        assert np.array_equal(ll + lp, lt_h)
        for i in range(v.shape[1]):
            xi = np.ascontiguousarray(v[:, i])
            assert ll[i] == lib.klara_user_loglikelihood(xi.ctypes.data_as(dp), t.ndims, t.data.ctypes.data_as(dp), t.data.size)
            assert lp[i] == lib.klara_user_logprior(xi.ctypes.data_as(dp), t.ndims, t.data.ctypes.data_as(dp), t.data.size)
    eng.close()


# ---- 8. against the hand-written gradient on the device
@pytest.mark.parametrize("sampler", [L.SAMPLER_MALA, L.SAMPLER_HMC])
@pytest.mark.parametrize("d", [3, 100])
def test_negdot_matches_the_hand_written_gradient_on_the_device(gpu_required, sampler, d):
    n, steps = 37, 30
    x0 = 0.7 * np.random.default_rng(d).standard_normal((n, d))
    kw = dict(sampler=sampler, nchains=n, nsteps=steps, driftstep=0.9 / d ** (1.0 / 3.0), leapstep=0.5 / d ** 0.25, nleaps=5, monitor=SUMS)
    out = []
    for target in (K.CustomTarget(d, cases.SRC_NEGDOT), K.CustomTarget.autodiff(d, A.AD_NEGDOT)):
        eng = K.Engine(target=target, **kw)
        eng.set_state(x0); eng.run(steps)
        out.append(eng.state() + (eng.accept_mask(),))
        eng.close()
    assert 0.0 < out[0][3].mean() < 1.0
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_logit_start_state_gradient_agrees_with_the_hand_written_one(gpu_required):
    """cases.SRC_LOGIT accumulates X' (y - logistic) row by row, the duals differentiate the log-target's own sums: different roundings of the same
    gradient, apart by no more than the cap of tests/test_autodiff_host.py (4 x 2.313 eps x sum |terms|)"""
    blk = A.swiss_block()
    case = A.make("mala_logit_swiss_rate")
    g = []
    for target in (K.CustomTarget(4, cases.SRC_LOGIT, blk), K.CustomTarget.autodiff(4, A.AD_LOGIT, blk)):
        eng = K.Engine(sampler=L.SAMPLER_MALA, target=target, nchains=case["nchains"], nsteps=4, driftstep=0.1)
        eng.set_state(case["x0"])
        g.append(eng.state()[2]); eng.close()
    for x, gh, ga in zip(case["x0"], *g):
        _, mag = A.truth_logit(x, blk)
        ratio = float(np.max(np.abs(ga.astype(A.LD) - gh.astype(A.LD)) / (A.EPS * mag)))
        assert ratio <= 4.0 * A.MEASURED["logit_swiss"], ratio


# ---- 9. invariance
@pytest.mark.parametrize("name", ["mala_logit_swiss_rate", "hmc_quartic_d33", "smmala_logit_swiss"])
def test_launch_length_does_not_change_the_bits(gpu_required, name):
    case = A.make(name)
    out = []
    for spl in (1, 7, 32):
        eng = K.Engine(**cases.engine_kwargs(case, monitor=SUMS, steps_per_launch=spl))
        eng.set_state(case["x0"]); eng.run(case["nsteps"])
        out.append(eng.state() + (eng.accept_mask(),))
        eng.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["mala_negdot_d9", "hmc_quartic_d33"])
def test_chain_offset_sharding(gpu_required, name):
    case = A.make(name)
    whole = K.Engine(**cases.engine_kwargs(case))
    whole.set_state(case["x0"]); whole.run(case["nsteps"])
    xw = whole.state()[0]
    whole.close()
    parts = []
    for off, n in ((0, 20), (20, case["nchains"] - 20)):
        e = K.Engine(**cases.engine_kwargs(case, chain_offset=off, nchains=n))
        e.set_state(case["x0"][off:off + n]); e.run(case["nsteps"])
        parts.append(e.state()[0]); e.close()
    assert np.array_equal(np.concatenate(parts), xw)


@pytest.mark.parametrize("name,chunk", [("mala_negdot_d9", 1), ("hmc_logit_d9_da", 4), ("hmc_quartic_d33", 1), ("hmc_quartic_d33", 10)])
def test_the_chunk_width_does_not_change_the_bits(gpu_required, name, chunk):
    """KLARA_USER_AUTODIFF_CHUNK against the library's choice (invariant A2): one chain per lane at D = 9, and the staged form"""
    case = A.make(name)
    t = case["target"]
    text = t.source.split("\n", 1)[1]
    out = []
    for target in (t, K.CustomTarget.autodiff(t.ndims, text, t.data, chunksize=chunk)):
        eng = K.Engine(**cases.engine_kwargs(dict(case, target=target)))
        eng.set_state(case["x0"]); eng.run(case["nsteps"])
        out.append(eng.state() + (eng.accept_mask(),))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 10. refusals
def test_refusals_through_the_engine(gpu_required):
    def status(**kw):
        try:
            K.Engine(nchains=8, nsteps=4, **kw).close()
        except K.KlaraError as e:
            return e.status
        return 0
    assert status(sampler=L.SAMPLER_MALA, target=K.CustomTarget.autodiff(20, A.AD_PAIR)) == L.ERR_UNSUPPORTED
    assert status(sampler=L.SAMPLER_SMMALA, target=K.CustomTarget.autodiff(9, A.AD_LOGIT, A.logit_block(), order=2)) == L.ERR_UNSUPPORTED
    assert status(sampler=L.SAMPLER_SMMALA, target=K.CustomTarget(5, A.marked(A.AD_NN_LL + A.AD_NN_LP, 2, parts=True), A.nn_block(5))) == L.ERR_UNSUPPORTED
    assert status(sampler=L.SAMPLER_MALA, target=K.CustomTarget.autodiff(3, A.AD_NO_FUNCTION)) == L.ERR_COMPILE
    assert status(sampler=L.SAMPLER_MALA, target=K.CustomTarget.autodiff(3, A.AD_NEGDOT)) == 0


@pytest.mark.parametrize("name", ["mala_negdot_d3", "hmc_quartic_d33", "smmala_gauss_d3"])
def test_nonfinite_start_state_is_refused(gpu_required, name):
    case = A.make(name)
    eng = K.Engine(**cases.engine_kwargs(case))
    x0 = case["x0"].copy(); x0[5, 1] = np.nan
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.set_state(case["x0"])                     # ... and the job goes on from valid values
    eng.run(3)
    eng.close()
