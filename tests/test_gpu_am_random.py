"""The AM kernels over the random jobs of am_cases.random_case: bit for bit against the CPU reference (oracle/klara_oracle.c ko_am) at every D in 1 .. 8 (E = 2 / 4 / 8
with and without padding elements), logistic and user-defined targets, both sides of the 64-row edge of the row split, chain counts around one
wavefront and one workgroup, every kernel MODE, monitor word, launch length, split run and shard offset, t0 from 2 on, c in {0, 0.05, 0.5} and both
scales; and one job per precompiled (E, MODE) instantiation.  It follows tests/test_gpu_matrix_samplers.py."""
import numpy as np
import pytest

import am_cases as AC
import cases
import klara_jl_amd as K
import matrix_sampler_random as MR
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu


def _run_pair(case, monitor, steps_per_launch, chain_offset, runs):
    eng = K.Engine(**AC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset))
    eng.set_state(case["x0"])
    job = AC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, want_hist=bool(monitor & L.MON_HISTORY))
    assert job.set_state(case["x0"]) == 0
    for k in runs:
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_same(eng, job, monitor):
    """as far as the monitor word keeps it: without a monitor the state and the sampler's own state alone"""
    x, lt, _ = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    Cm, m, m2, fallbacks = eng.am_state()
    assert np.array_equal(Cm, job.C), "covariances differ from the reference"
    assert np.array_equal(m, job.lastmean) and np.array_equal(m2, job.secondlastmean), "running means differ from the reference"
    assert fallbacks == job.fallbacks, (fallbacks, job.fallbacks)
    if monitor & L.MON_ACCEPT:
        assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    if monitor & L.MON_SUMMARIES:
        s, q, _ = eng.chain_sums()
        assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    if monitor != 0:
        _, a, p, t = eng.tune()
        assert np.array_equal(a, job.accepted) and np.array_equal(p, job.proposed) and np.array_equal(t, job.totproposed), "tuner counters differ"
    if monitor & L.MON_HISTORY:
        for c in sorted({0, job.N // 2, job.N - 1}):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, _ = eng.chain_fields(c, logtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"


@pytest.mark.parametrize("seed", range(AC.RANDOM_NSEEDS))
def test_random_configurations(gpu_required, seed):
    case = AC.random_case(seed)
    r = case.run
    eng, job = _run_pair(case, r["monitor"], r["steps_per_launch"], r["chain_offset"], r["runs"])
    rows = MR.nrows(case)
    split = rows is not None and rows >= 64                                     # kind 2: RS = 4 lanes share a chain's rows
    assert eng.layout() == ((2, 4) if split else (0, 1)) + (MR.pad_of(case["target"].ndims),), (eng.layout(), rows)
    _assert_same(eng, job, r["monitor"])
    eng.close()


_INST = [(e, mode) for e in (2, 4, 8) for mode in (0, 1, 3, 7)]


@pytest.mark.parametrize("e,mode", _INST, ids=[f"E{a}-MODE{b}" for a, b in _INST])
def test_every_instantiation(gpu_required, e, mode):
    """k_transitions<AM, LOGISTIC, E, 1, MODE> of klara_am.hip, each once: D = 2 (E = 2, no padding), 3 (E = 4, one padding element) and 7 (E = 8, one), 65
    chains, 66 rows (the row split), t0 = 4 of 14 transitions.  MODE 0: a counting job with every monitor; 1: a plain job with every monitor; 3: a plain
    job without a monitor, all its transitions in one launch; 7: that job in one-transition launches."""
    d, n, nrows = {2: 2, 4: 3, 8: 7}[e], 65, 66
    rng = np.random.default_rng(100 * e + mode + 25)
    X, y = cases.synthetic_logit(nrows, d, seed=e + mode)
    c = MR.Case(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=14, burnin=2, thinning=2, seed=5252 + 10 * e + mode, x0=0.3 * rng.standard_normal((n, d)),
                am_C0=0.09 * np.eye(d), name=f"inst_am_{e}_{mode}", **AC.am(d, 4, c=0.2, minorscale=0.05))
    if mode == 0:
        c.update(verbose=True, period=4)
    monitor = 0 if mode in (3, 7) else AC.HIST
    spl = 1 if mode == 7 else 0
    eng, job = _run_pair(c, monitor, spl, 0, [c["nsteps"]])
    assert eng.layout() == (2, 4, e), eng.layout()
    if monitor:
        assert 0.05 < job.accept.mean() < 0.95, job.accept.mean()
    _assert_same(eng, job, monitor)
    eng.close()
