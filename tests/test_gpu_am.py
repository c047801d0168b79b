"""The AM kernels on the GPU: bit for bit against the CPU reference (oracle/klara_oracle.c ko_am) — the covariances, the running means and the fallback count
included —, launch-length and sharding invariance, runs split around t0, klara_reset, the getter's refusals.  Small shapes: 96 - 131 chains (a last
wavefront with idle lanes), 30 - 40 transitions with t0 in {2, 5, 10}, so that every run has transitions before, at and after t0."""
import numpy as np
import pytest

import am_cases as AC
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = AC.HIST


def _run_pair(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, runs=None):
    n = case["nchains"] if nchains is None else nchains
    x0 = case["x0"][chain_offset:chain_offset + n]
    eng = K.Engine(**AC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    job = AC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
    eng.set_state(x0)
    assert job.set_state(x0) == 0
    for k in (runs or [case["nsteps"]]):
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_am_state(eng, job):
    Cm, m, m2, fallbacks = eng.am_state()
    assert np.array_equal(Cm, job.C), "covariances differ from the reference"
    assert np.array_equal(m, job.lastmean) and np.array_equal(m2, job.secondlastmean), "running means differ from the reference"
    assert fallbacks == job.fallbacks, (fallbacks, job.fallbacks)


def _assert_same(eng, job, hist=True):
    x, lt, _ = eng.state()
    assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    _assert_am_state(eng, job)
    s, q, _ = eng.chain_sums()
    assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    _, a, p, t = eng.tune()
    assert np.array_equal(a, job.accepted) and np.array_equal(p, job.proposed) and np.array_equal(t, job.totproposed), "tuner counters differ"
    if hist:
        for c in (0, job.N // 2, job.N - 1):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, _ = eng.chain_fields(c, logtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"


@pytest.mark.parametrize("name", AC.ALL + [AC.FALLBACK])
def test_bit_exact_against_the_reference(gpu_required, name):
    case = AC.make(name)
    eng, job = _run_pair(case)
    if name in AC.LOGIT:
        d, kind = case["target"].ndims, int(name[-1])
        assert eng.layout() == ((2, 4) if kind == 2 else (0, 1)) + (2 if d <= 2 else 4 if d <= 4 else 8,), eng.layout()
    _assert_same(eng, job)
    assert 0.0 < job.accept.mean() < 1.0
    assert case["am_t0"] + 1 < case["nsteps"]
    if name == "logit_d8_verbose":
        assert job.proposed.max() > 0 and job.totproposed.min() > case["period"], "the verbose tuner counted nothing"
    if name == AC.FALLBACK:
        assert job.fallbacks > 0, "the t0 = 2 case fell back nowhere"
    else:
        assert job.fallbacks == 0
    # the covariance moved away from C0 and the two means differ: a kernel that never adapts cannot pass
    C0 = np.asarray(case["am_C0"], dtype=float)
    assert not np.array_equal(job.C[0], np.diag(C0) if C0.ndim == 1 else C0) and not np.array_equal(job.lastmean, job.secondlastmean)
    eng.close()


@pytest.mark.parametrize("name", ["swiss_example", "quad_d3"])
def test_job_without_a_monitor(gpu_required, name):
    """monitor 0 of a plain job: MODE 3, and in one-transition launches MODE 7 (the kernel that writes an accepted proposal straight to memory)"""
    case = AC.make(name)
    for spl in (0, 1):
        eng, job = _run_pair(case, monitor=0, steps_per_launch=spl)
        x, lt, _ = eng.state()
        assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), f"state differs from the reference at steps_per_launch = {spl}"
        _assert_am_state(eng, job)
        a, n = eng.accept_counts()
        assert np.array_equal(a, job.naccept) and n == case["nsteps"]
        eng.close()


@pytest.mark.parametrize("monitor", [0, L.MON_ACCEPT, HIST])
@pytest.mark.parametrize("name", ["swiss_example", "logit_d5_k2", "likprior_d5"])
def test_launch_length_does_not_change_the_bits(gpu_required, name, monitor):
    """steps_per_launch 1 / 7 / 32: the covariances and the means travel through memory between launches, and t0 (10, 5, 5) falls inside a launch of 7 and
    of 32"""
    case = AC.make(name)
    out = []
    for spl in (1, 7, 32):
        eng = K.Engine(**AC.engine_kwargs(case, monitor=monitor, steps_per_launch=spl))
        eng.set_state(case["x0"])
        eng.run(case["nsteps"])
        x, lt, _ = eng.state()
        Cm, m, m2, fb = eng.am_state()
        out.append((x, lt, Cm, m, m2, np.int64(fb)) + ((eng.accept_mask(),) if monitor & L.MON_ACCEPT else ()))
        eng.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)
    job = AC.ref_job(case)
    assert job.set_state(case["x0"]) == 0 and job.run(case["nsteps"]) == 0
    assert np.array_equal(out[0][0], job.X) and np.array_equal(out[0][2], job.C) and np.array_equal(out[0][3], job.lastmean)


@pytest.mark.parametrize("name", ["swiss_example", "logit_d3_k0", AC.FALLBACK])
def test_runs_split_around_t0(gpu_required, name):
    """runs of [t0 - 1, 1, 1, rest]: the last transition before the adaptation, the first of it and the next are launches of their own"""
    case = AC.make(name)
    t0 = case["am_t0"]
    eng, job = _run_pair(case, runs=[t0 - 1, 1, 1, case["nsteps"] - t0 - 1])
    _assert_same(eng, job)
    whole = AC.ref_job(case)
    assert whole.set_state(case["x0"]) == 0 and whole.run(case["nsteps"]) == 0
    assert np.array_equal(job.X, whole.X) and np.array_equal(job.C, whole.C) and job.fallbacks == whole.fallbacks
    eng.close()


def test_reset(gpu_required):
    case = AC.make("swiss_example")
    n = case["nchains"]
    eng, job = _run_pair(case, runs=[13, 1, 26])
    _assert_same(eng, job)
    C0 = np.broadcast_to(np.eye(4), (n, 4, 4))
    # reset(job): the next Philox key; C = C0, both means = the state, the count and the counter restart (AM.jl:292-304)
    eng.reset(); assert job.reset() == 0
    Cm, m, m2, fb = eng.am_state()
    x = eng.state()[0]
    assert np.array_equal(Cm, C0) and np.array_equal(m, x) and np.array_equal(m2, x) and fb == 0
    eng.run(17); assert job.run(17) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.state()[1], job.LT) and np.array_equal(eng.accept_mask(), job.accept)
    _assert_am_state(eng, job)
    x1 = AC.SWISS_X0[None, :] + np.zeros((n, 4))
    eng.reset(x1); assert job.reset(x1) == 0
    Cm, m, m2, fb = eng.am_state()
    assert np.array_equal(Cm, C0) and np.array_equal(m, x1) and np.array_equal(m2, x1) and fb == 0
    eng.run(14); assert job.run(14) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.accept_mask(), job.accept)
    _assert_am_state(eng, job)
    eng.close()


def test_reset_clears_the_fallback_counter(gpu_required):
    case = AC.make(AC.FALLBACK)
    eng, job = _run_pair(case, runs=[10])
    assert eng.am_state()[3] == job.fallbacks > 0
    eng.set_state(case["x0"]); assert job.set_state(case["x0"]) == 0
    assert eng.am_state()[3] == 0
    eng.run(10); assert job.run(10) == 0
    _assert_am_state(eng, job)
    eng.close()


def test_chain_offset_sharding(gpu_required):
    """two shards with chain_offset draw and adapt what one job of all chains does"""
    case = AC.make("logit_d8_k2")
    n = case["nchains"]
    whole = K.Engine(**AC.engine_kwargs(case))
    whole.set_state(case["x0"]); whole.run(case["nsteps"])
    xw, sw = whole.state()[0], whole.am_state()
    whole.close()
    xs, ss = [], []
    for off, k in ((0, 50), (50, n - 50)):
        e = K.Engine(**AC.engine_kwargs(case, chain_offset=off, nchains=k))
        e.set_state(case["x0"][off:off + k]); e.run(case["nsteps"])
        xs.append(e.state()[0]); ss.append(e.am_state()); e.close()
    assert np.array_equal(np.concatenate(xs), xw)
    for i in range(3):
        assert np.array_equal(np.concatenate([s[i] for s in ss]), sw[i])
    assert sum(s[3] for s in ss) == sw[3]
    eng, job = _run_pair(case, chain_offset=50, nchains=n - 50)
    _assert_same(eng, job)
    eng.close()


def test_getter_refusals(gpu_required):
    case = AC.make("logit_d3_k2")
    eng = K.Engine(**AC.engine_kwargs(case))
    with pytest.raises(K.KlaraError) as ei:                       # before set_state
        eng.am_state()
    assert ei.value.status == L.ERR_STATE
    x0 = case["x0"].copy(); x0[5, 1] = np.nan
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.set_state(case["x0"])                                     # ... and the job goes on from valid values
    eng.run(3)
    Cm, m, m2, fb = eng.am_state()
    assert np.all(np.isfinite(Cm)) and fb == 0
    eng.close()
    kw = AC.engine_kwargs(case)
    kw.update(sampler=L.SAMPLER_MH, mh_sigma=np.ones(3), am_C0=None, am_corescale=0.0, am_minorscale=0.0, am_c=0.0, am_t0=0)
    mh = K.Engine(**kw)
    mh.set_state(case["x0"])
    with pytest.raises(K.KlaraError) as ei:
        mh.am_state()
    assert ei.value.status == L.ERR_INVALID_ARG
    mh.close()
    kw.update(sampler=L.SAMPLER_RAM, mh_sigma=None, ram_S0=np.eye(3), ram_targetrate=0.234, ram_gamma=0.7)
    ram = K.Engine(**kw)
    ram.set_state(case["x0"])
    with pytest.raises(K.KlaraError) as ei:
        ram.am_state()
    assert ei.value.status == L.ERR_INVALID_ARG
    ram.close()
