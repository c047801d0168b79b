"""The oracle's dispatch to SMMALA, RAM and AM at the limits of what it serves: E <= 8 padded elements per chain.  D = 9 (one past the last
dimension served; its layout has E = 16) is KLARA_ERR_UNSUPPORTED; D = 1 and D = 8 (the edges of the padded E: 2 and 8) run, and a run of 5
transitions equals 2 followed by 3 bit for bit — the sampler state (RAM's factors, AM's covariances and means, the counters) included, and
SMMALA's factor state, which is formed again at the start of every call."""
import numpy as np
import pytest

import am_cases as AC
import ram_cases as RC
import smmala_cases as SC
import softabs_cases as SAC
from klara_jl_amd import _lib as L

N, STEPS = 3, 5
SAMPLERS = {
    "smmala": (SC, lambda d: dict(sampler=L.SAMPLER_SMMALA, driftstep=0.8)),
    "softabs": (SAC, lambda d: dict(sampler=L.SAMPLER_SMMALA, driftstep=0.8, smmala_softabs=2.0)),
    "ram": (RC, lambda d: dict(sampler=L.SAMPLER_RAM, ram_S0=np.full(d, 0.7), ram_targetrate=0.234, ram_gamma=0.7)),
    "am": (AC, lambda d: dict(am_C0=np.full(d, 0.4), **AC.am(d, 2))),
}
STATE = ("X", "G", "LT", "accept", "_sum", "_sumsq", "held", "naccept", "step", "accepted", "proposed", "totproposed", "hist", "hist_lt", "hist_g",
         "_P", "lastmean", "secondlastmean", "_skipped", "_fallbacks")


def _job(family, d):
    mod, kw = SAMPLERS[family]
    P = SC.conditioned_precision(d, 10.0, seed=40 + d)
    case = dict(target=SC.quad_target(0.5, P, P), nchains=N, nsteps=STEPS, verbose=True, period=2,
                x0=0.5 * np.random.default_rng(d).standard_normal((N, d)), **kw(d))
    return mod.ref_job(case, want_hist=True), case


@pytest.mark.parametrize("family", list(SAMPLERS))
def test_one_past_the_last_dimension_served_is_unsupported(family):
    job, case = _job(family, 9)
    assert job.layout.E == 16
    assert job.set_state(case["x0"]) == L.ERR_UNSUPPORTED
    assert job.run(STEPS) == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("family", list(SAMPLERS))
def test_a_split_run_is_the_whole_run_bit_for_bit(family, d):
    whole, case = _job(family, d)
    split, _ = _job(family, d)
    assert whole.layout.E == (2 if d == 1 else 8)
    assert whole.set_state(case["x0"]) == 0 and split.set_state(case["x0"]) == 0
    assert whole.run(5) == 0
    assert split.run(2) == 0 and split.run(3) == 0
    assert whole.t == split.t == STEPS and whole.accept.shape == (STEPS, N)
    for name in STATE:
        a, b = getattr(whole, name, None), getattr(split, name, None)
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{family}, D = {d}: {name} differs between run(5) and run(2) + run(3)"
    assert np.isfinite(whole.X).all() and np.isfinite(whole.LT).all()
