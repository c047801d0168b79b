"""GPU tests (-m gpu) of the exact folds in the unit-diagonal kernels (klara.jl_amd/csrc/klara_diagt.h).

On lt = -|x|^2 the MALA kernels form both means as x + (-h) * x and the HMC kernels kick with fma(-2 kf, x, m): the gradient -2.0 * x
they no longer form is an exact scaling, so no bit of any result may move (tests/test_exact_folds_host.py has the arithmetic).  Every
instantiation the change touches runs here against the oracle, which keeps the unfolded formulas: 50 chains (the last chain group of every
layout is partial: 16, 8 and 4 chains per wavefront) and 40 transitions (a launch of 32 and one of 8), values, log-targets, gradients, accept
masks and counts and the running sums bit for bit.  A job without a saved-sample monitor keeps no running sums: there the rest is compared.
Two jobs on a diagonal whose weights are not powers of two show that the unfolded path still is what it was."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

NCHAINS, NSTEPS = 50, 40
SUMS = L.MON_ACCEPT | L.MON_SUMMARIES


def _unit(d):
    return K.GaussDiagTarget.negdot(d)


def _nonunit(d):
    t = K.GaussDiagTarget.mvnormal(np.linspace(-1.0, 1.0, d), np.linspace(0.7, 1.5, d))
    w = np.asarray(t.w, dtype=np.float64)
    assert np.all(np.frexp(w)[0] != 0.5) and np.count_nonzero(np.asarray(t.mu)) >= d - 1       # no weight is a power of two; non-zero means
    return t


def _mala(d, **kw):
    return dict(sampler=L.SAMPLER_MALA, target=_unit(d), driftstep=0.3, **kw)


def _hmc(d, **kw):
    return dict(sampler=L.SAMPLER_HMC, target=_unit(d), leapstep=0.1, nleaps=3, **kw)


# name -> (case settings, monitor, steps per launch (0: the default), lanes per chain of the layout, launches on the 4-lane kernels or None)
FOLD_CASES = {
    "mala_d17_q4_half_pair": (_mala(17, sparse_moves=1), SUMS, 0, 8, 2),                # 4 lanes per chain (sums in the 8-lane order), odd D
    "mala_d100_q4_sums": (_mala(100, sparse_moves=1), SUMS, 0, 8, 2),                   # the headline kernel: sums folded into memory
    "mala_d100_q8_sums": (_mala(100, sparse_moves=2), SUMS, 0, 8, 0),                   # its 8-lane sibling: resident sums
    "mala_d100_onestep": (_mala(100, sparse_moves=1), L.MON_ACCEPT, 1, 8, NSTEPS),      # one transition per launch, no saved-sample monitor
    # (the tuner works during the burn-in: 20 of the 40 transitions, four tuning events per chain, so the step — and -h — is per chain)
    "mala_d100_tuned": (_mala(100, tuner=L.TUNER_ACCEPT_RATE, targetrate=0.574, period=5, burnin=20), SUMS, 0, 8, None),
    "mala_d130_q16": (_mala(130), SUMS, 0, 16, None),
    "hmc_d17": (_hmc(17), SUMS, 0, 8, None),
    "hmc_d100_q4": (_hmc(100), L.MON_ACCEPT, 0, 8, 2),                                  # no saved-sample monitor: 4 lanes per chain
    "hmc_d100_q8_sums": (_hmc(100), SUMS, 0, 8, None),
    "hmc_d100_dualavg": (dict(sampler=L.SAMPLER_HMC, target=_unit(100), leapstep=0.2, nleaps=4, tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.7,
                              da_nadapt=30), SUMS, 0, 8, None),                         # per-chain trajectory lengths within a wavefront
    "mala_d20_nonunit": (dict(sampler=L.SAMPLER_MALA, target=_nonunit(20), driftstep=0.3), SUMS, 0, 8, None),
    "hmc_d20_nonunit": (dict(sampler=L.SAMPLER_HMC, target=_nonunit(20), leapstep=0.1, nleaps=3), SUMS, 0, 8, None),
}


@pytest.mark.parametrize("name", list(FOLD_CASES))
def test_exact_folds_bit_for_bit_against_the_oracle(name):
    kw, monitor, spl, lanes, n4 = FOLD_CASES[name]
    case = dict(dict(burnin=0), **kw, nchains=NCHAINS, nsteps=NSTEPS, x0=None, seed=20260927, name=name)
    eng = K.Engine(**cases.engine_kwargs(case, monitor=monitor, steps_per_launch=spl))
    layout = eng.layout()
    assert layout[:2] == (3, lanes), layout
    job = O.OracleJob(**cases.oracle_kwargs(case, layout=layout))
    eng.init_state_normal(); assert job.init_state_normal() == 0
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT) and np.array_equal(g, job.G), f"{name}: initial state differs"
    eng.run(NSTEPS); assert job.run(NSTEPS) == 0
    if n4 is not None:
        assert int(eng.launch_modes()[0][0]) == n4, (name, eng.launch_modes()[0])        # the kernel family the case is about ran
    mask = eng.accept_mask()
    assert np.array_equal(mask, job.accept), f"{name}: accept mask differs at {np.argwhere(mask != job.accept)[:5]}"
    assert 0 < int(mask.sum()) < mask.size, f"{name}: accepted {int(mask.sum())} of {mask.size}"      # both the commit and the reject path ran
    x, lt, g = eng.state()
    assert np.array_equal(x.view(np.uint64), job.X.view(np.uint64)), f"{name}: values differ"
    assert np.array_equal(lt.view(np.uint64), job.LT.view(np.uint64)), f"{name}: log-target differs"
    assert np.array_equal(g.view(np.uint64), job.G.view(np.uint64)), f"{name}: gradient differs"
    na, nst = eng.accept_counts()
    assert np.array_equal(na, job.naccept) and nst == NSTEPS, f"{name}: accept counts differ"
    if monitor & L.MON_SUMMARIES:
        s, q, nsaved = eng.chain_sums()
        assert nsaved == NSTEPS - case["burnin"]
        assert np.array_equal(s.view(np.uint64), job.sum.view(np.uint64)) and np.array_equal(q.view(np.uint64), job.sumsq.view(np.uint64)), \
            f"{name}: running sums differ"
    if case.get("tuner", 0) != 0:
        step = eng.tune()[0]
        assert np.array_equal(step, job.step), f"{name}: tuned step differs"
        assert np.unique(step).size > 1, f"{name}: every chain kept the same step"       # -h / -eps really are per lane
    if case.get("tuner", 0) == L.TUNER_DUAL_AVERAGING:
        eb, hb = eng.dual_averaging()
        assert np.array_equal(eb, job.da_epsbar) and np.array_equal(hb, job.da_hbar), f"{name}: dual-averaging state differs"
    eng.close()
