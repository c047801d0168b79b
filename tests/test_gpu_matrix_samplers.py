"""The samplers that carry a per-chain matrix in registers — SMMALA, SMMALA with the softabs transform, RAM — over the random jobs of
tests/matrix_sampler_random.py: bit for bit against the CPU oracle (oracle/klara_oracle.c: ko_smmala, ko_ram) at every D in 1 .. 8
(E = 2 / 4 / 8 with and without padding elements), both sides of the 64-row edge of the row split, chain counts around one wavefront and one workgroup,
every tuner, monitor word, launch length and shard offset; one job per precompiled (sampler, E, MODE) instantiation; and launch-length, sharding and
split-run invariance on random jobs.  tests/test_matrix_samplers_host.py holds the references to the NumPy restatements on the same seeds."""
import numpy as np
import pytest

import cases
import klara_jl_amd as K
import matrix_sampler_random as MR
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

SEEDS = [(f, s) for f in MR.FAMILIES for s in range(MR.NSEEDS[f])]
GRAD = {"smmala": True, "softabs": True, "ram": False}


def _engine(family, case, monitor, steps_per_launch, chain_offset, lo=0, n=None):
    """the Engine of chains [lo, lo + n) of the case, whose chain 0 is global chain `chain_offset`, with its start state set"""
    n = case["nchains"] - lo if n is None else n
    eng = K.Engine(**MR.MODULES[family].engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset + lo, nchains=n))
    eng.set_state(case["x0"][lo:lo + n])
    return eng


def _run_pair(family, case, monitor, steps_per_launch, chain_offset, runs):
    eng = _engine(family, case, monitor, steps_per_launch, chain_offset)
    job = MR.MODULES[family].ref_job(case, layout=eng.layout(), chain_offset=chain_offset, want_hist=bool(monitor & L.MON_HISTORY))
    assert job.set_state(case["x0"]) == 0
    for k in runs:
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_same(family, eng, job, monitor):
    """what test_gpu_smmala.py / test_gpu_softabs.py / test_gpu_ram.py compare, as far as the monitor word keeps it: without a monitor the state alone"""
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    if GRAD[family]:
        assert np.array_equal(g, job.G), "gradient differs from the reference"
    else:
        S, skipped = eng.ram_factor()
        assert np.array_equal(S, job.S), "factors differ from the reference"
        assert skipped == job.skipped == 0
    if monitor & L.MON_ACCEPT:
        assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    if monitor & L.MON_SUMMARIES:
        s, q, _ = eng.chain_sums()
        assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    if monitor != 0:
        step, a, p, t = eng.tune()
        if GRAD[family]:
            assert np.array_equal(step, job.step if job.step.size == job.N else np.full(job.N, job.step[0])), "tuned steps differ"
        else:
            assert np.array_equal(a, job.accepted) and np.array_equal(p, job.proposed) and np.array_equal(t, job.totproposed), "tuner counters differ"
    if monitor & L.MON_HISTORY:
        for c in sorted({0, job.N // 2, job.N - 1}):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, g_h = eng.chain_fields(c, logtarget=True, gradlogtarget=GRAD[family])
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"
            if GRAD[family]:
                assert np.array_equal(g_h, job.hist_g[:g_h.shape[1], c, :].T), f"gradient history of chain {c} differs"


@pytest.mark.parametrize("family,seed", SEEDS, ids=[f"{f}-{s}" for f, s in SEEDS])
def test_random_configurations(gpu_required, family, seed):
    case = MR.random_case(seed, family)
    r = case.run
    eng, job = _run_pair(family, case, r["monitor"], r["steps_per_launch"], r["chain_offset"], r["runs"])
    rows = MR.nrows(case)
    split = rows is not None and rows >= 64                                     # kind 2: RS = 4 lanes share a chain's rows
    assert eng.layout() == ((2, 4) if split else (0, 1)) + (MR.instantiation(case)[1],), (eng.layout(), MR.instantiation(case), rows)
    _assert_same(family, eng, job, r["monitor"])
    eng.close()


# ---------------------------------------------------------------- one job per precompiled instantiation
_INST = [(smp, e, mode) for smp in ("smmala", "ram") for e in (2, 4, 8) for mode in (0, 1, 3, 7)]


@pytest.mark.parametrize("smp,e,mode", _INST, ids=[f"{a}-E{b}-MODE{c}" for a, b, c in _INST])
def test_every_instantiation(gpu_required, smp, e, mode):
    """k_transitions<SMMALA | RAM, LOGISTIC, E, 1, MODE> of klara_smmala.hip / klara_ram.hip, each once: D = 2 (E = 2, no padding), 3 (E = 4, one padding
    element) and 7 (E = 8, one), 65 chains (the row split puts 16 on a wavefront: a second workgroup whose one wavefront holds one chain), 66 rows (the row
    split: 8 full rounds of RS x the two-row batch and two rows more), at a step where a good share of the proposals is rejected and a good share accepted.
    MODE 0: a counting job (SMMALA: AcceptanceRateMCTuner, RAM: verbose) with every monitor; 1: a plain job with every monitor; 3: a plain job without a
    monitor, all its transitions in one launch; 7: that job in one-transition launches."""
    d, n, nrows = {2: 2, 4: 3, 8: 7}[e], 65, 66
    rng = np.random.default_rng(100 * e + mode + (50 if smp == "ram" else 0))
    X, y = cases.synthetic_logit(nrows, d, seed=e + mode)
    c = MR.Case(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=14, burnin=2, thinning=2, seed=4242 + 10 * e + mode, x0=0.3 * rng.standard_normal((n, d)),
                name=f"inst_{smp}_{e}_{mode}")
    if smp == "smmala":
        c.update(sampler=L.SAMPLER_SMMALA, driftstep=1.4)
        if mode == 0:
            c.update(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5, period=4)
    else:
        S0 = np.diag(np.full(d, 0.35)) + np.tril(0.1 * rng.standard_normal((d, d)), -1)
        c.update(sampler=L.SAMPLER_RAM, ram_S0=S0, ram_targetrate=0.3, ram_gamma=0.6)
        if mode == 0:
            c.update(verbose=True, period=4)
    monitor = 0 if mode in (3, 7) else MR.HIST_SMMALA if smp == "smmala" else MR.HIST_RAM
    spl = 1 if mode == 7 else 0
    assert MR.instantiation(c, monitor, spl) == (c["sampler"], e, mode)
    eng, job = _run_pair(smp, c, monitor, spl, 0, [c["nsteps"]])
    assert eng.layout() == (2, 4, e), eng.layout()
    assert 0.05 < job.accept.mean() < 0.95, job.accept.mean()                   # both the commit and the re-read are exercised
    _assert_same(smp, eng, job, monitor)
    eng.close()


# ---------------------------------------------------------------- invariance on random jobs
def _invariance_seeds(family, count=3):
    """the family's first seeds whose job has at least 31 chains and a tuner state per chain (a shard of a pooled job pools over fewer chains)"""
    out = [s for s in range(MR.NSEEDS[family]) if (lambda c: c["nchains"] >= 31 and not MR.is_pooled(c))(MR.random_case(s, family))]
    return out[:count]


INVARIANCE = [(f, s) for f in MR.FAMILIES for s in _invariance_seeds(f)]


def _final(family, case, monitor, steps_per_launch, chain_offset, runs, lo=0, n=None):
    eng = _engine(family, case, monitor, steps_per_launch, chain_offset, lo, n)
    for k in runs:
        eng.run(k)
    x, lt, g = eng.state()
    out = dict(x=x, lt=lt)
    if GRAD[family]:
        out["g"] = g
    else:
        out["S"] = eng.ram_factor()[0]
    if monitor & L.MON_ACCEPT:
        out["accept"] = eng.accept_mask().T                                     # (chains first, like the others)
    eng.close()
    return out


@pytest.mark.parametrize("family,seed", INVARIANCE, ids=[f"{f}-{s}" for f, s in INVARIANCE])
def test_invariance(gpu_required, family, seed):
    """the same bits at 1 / 7 / 32 transitions per launch; chains [k, k + m) as a handle of their own with chain_offset are those chains of the whole job;
    a run in three pieces is the whole run"""
    case = MR.random_case(seed, family)
    r, nsteps, n = case.run, case["nsteps"], case["nchains"]
    mon, off = r["monitor"], r["chain_offset"]
    whole = _final(family, case, mon, 32, off, [nsteps])
    for spl in (1, 7):
        got = _final(family, case, mon, spl, off, [nsteps])
        assert all(np.array_equal(whole[f], got[f]) for f in whole), f"{spl} transitions per launch change the bits"
    k, m = n // 3, min(n - n // 3, 70)                                          # (from inside one wavefront into the next)
    part = _final(family, case, mon, r["steps_per_launch"], off, [nsteps], lo=k, n=m)
    assert all(np.array_equal(whole[f][k:k + m], part[f]) for f in whole), "a shard differs from its chains of the whole job"
    pieces = _final(family, case, mon, r["steps_per_launch"], off, [nsteps // 3, 1, nsteps - nsteps // 3 - 1])
    assert all(np.array_equal(whole[f], pieces[f]) for f in whole), "a run in three pieces differs from the whole run"
