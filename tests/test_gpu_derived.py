"""The derived quantities on the device (klara_derived.h's k_derived_update compiled with the user's closure behind every launch of a job with
klara_desc.derived_nout > 0; klara_get_derived_sums, klara_gather_derived_*) against tests/derived_ref.py: the same C text built by gcc, evaluated on the
same array and summed in the stated order — every comparison of sums and values is bit for bit (two NaNs equal).  Through klara_selftest_derived at the
shapes at which the kernel can go wrong — a partial wavefront, a partial second workgroup, the widest LDS rows, one dimension and one output, the largest
output count, 37 columns cut three ways — and through small jobs: a built-in target, the logistic regression with the math tables in the closure, a
user-defined target (two run-time modules in one handle).  The reductions are the coordinates' own: their mirrors and bounds apply unchanged."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import derived_cases as DC
import derived_ref as R
import klara_jl_amd as K
import pooled_ref as P
import rhat_ref as RH
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]
ROOT = Path(__file__).resolve().parent.parent


def check(hist, src, nout, data, what, splits_list):
    rs, rq, ry = R.reference(src, nout, hist, data)
    for name, splits in splits_list:
        s, q, v = R.selftest(hist, splits, src, nout, data)
        d = (R.bits_differ(s, rs), R.bits_differ(q, rq), R.bits_differ(v, ry))
        print(f"derived {what}, splits {name}: {v.size} values; sums, sums of squares, values differing {d}")
        assert d == (0, 0, 0), (what, name)
    s, q, v = R.selftest(hist, splits_list[0][1], src, nout, data, values=False)          # the kernel without staging: the same sums
    assert v is None and R.bits_differ(s, rs) == 0 and R.bits_differ(q, rq) == 0, what
    return rs, rq, ry


# ---------------------------------------------------------------- through the self test
@pytest.mark.parametrize("N, D, nout, name", [(70, 3, 2, "A"), (300, 17, 5, "E"), (9, 1024, 2, "B"), (64, 1, 1, "C"), (130, 100, 64, "E")])
def test_selftest_shapes(N, D, nout, name):
    """(70, 3, 2): a partial wavefront; (300, 17, 5): two workgroups, the second partial; (9, 1024, 2): 7 chains per workgroup, the LDS rows at their
    widest, the whole row read; (64, 1, 1): one dimension, one output, kd_exp's tables in LDS; (130, 100, 64): the largest output count"""
    ch = R.geometry(N, D, nout)[0]
    assert {(70, 3): ch > N and N % 64, (300, 17): ch < N < 2 * ch, (9, 1024): ch == 7, (64, 1): True, (130, 100): ch < N}[(N, D)]
    hist = DC.history(5, N, D, seed=N)
    check(hist, getattr(DC, "SRC_" + name), nout, DC.covariate_row(D) if name == "C" else None, f"N={N} D={D} K={nout}", [("5", [5]), ("2+0+3", [2, 0, 3])])


def test_selftest_every_cut_gives_the_same_bits():
    """37 saved steps — beyond the 32 columns of one kernel launch — as 32 + 5, as 1 + 5 + 31, as thirty-seven ones and as one launch that goes in pieces"""
    hist = DC.history(37, 70, 3, seed=37)
    check(hist, DC.SRC_A, DC.K_A, None, "37 columns", [("32+5", [32, 5]), ("1+5+31", [1, 5, 31]), ("37 x 1", [1] * 37), ("37", [37])])


def test_selftest_nan_flows_through_where_the_host_has_it():
    hist = DC.half_negative_history(6, 70, 3, seed=2)
    rs, rq, ry = check(hist, DC.SRC_D, DC.K_D, None, "NaN", [("6", [6]), ("1+5", [1, 5])])
    odd = np.arange(70) % 2 == 1
    assert np.array_equal(np.isnan(rs[:, 0]), odd) and np.array_equal(np.isnan(rq[:, 0]), odd)     # chains without a negative x0 are untouched


def test_selftest_wide_rows_with_the_math_tables():
    """D = 479: 16 chains per workgroup, 61,312 bytes of rows beside the 8 KB of kd_exp's tables"""
    assert R.geometry(20, 479, 1)[0] == 16
    hist = DC.history(3, 20, 479, seed=479, scale=0.05)
    check(hist, DC.SRC_C, DC.K_C, DC.covariate_row(479), "N=20 D=479 K=1", [("3", [3])])


# ---------------------------------------------------------------- through jobs
NCH, BURNIN, THIN, NSTEPS, SPL = 70, 10, 3, 50, 7
NSAVED = (NSTEPS - BURNIN - 1) // THIN + 1
DER_A = K.Derived(DC.K_A, DC.SRC_A, marginals=K.Marginals(16, [-3.0, -2.0], [3.0, 2.0]))


def _mala(monitor, derived=DER_A, run=None, spl=SPL):
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(3), driftstep=0.3, nsteps=NSTEPS, nchains=NCH, burnin=BURNIN, thinning=THIN,
                   monitor=monitor, seed=20261020, steps_per_launch=spl, derived=derived)
    eng.init_state_normal()
    for n in ([NSTEPS] if run is None else run):
        eng.run(n)
    return eng


def _history(eng):
    """(nsaved, N, D) from the read-back chains"""
    return np.ascontiguousarray(np.stack([eng.chain(c) for c in range(eng.nchains)], axis=0).transpose(2, 0, 1))


def _sums_equal_reference(eng, what):
    dq = eng.derived
    s, q, n = eng.derived_sums()
    hist = _history(eng)
    rs, rq, ry = R.reference(dq.source, dq.nout, hist, dq.data)
    d = (R.bits_differ(s, rs), R.bits_differ(q, rq))
    print(f"derived job {what}: {n} saved steps x {eng.nchains} chains x {dq.nout} outputs; sums, sums of squares differing {d}")
    assert n == hist.shape[0] and d == (0, 0), what
    return s, q, n, ry


def _inputs(s, q, n):
    """the derived sums as the coordinate reductions see them: nothing held back, no accepts"""
    return {"sum": s, "sumsq": q, "X": s, "held": np.zeros(s.shape[0], dtype=np.int64), "naccept": np.zeros(s.shape[0], dtype=np.uint64), "nsaved": int(n)}


@pytest.fixture(scope="module")
def first_job():
    eng = _mala(L.MON_HISTORY | L.MON_ACCEPT | L.MON_SUMMARIES)
    yield eng
    eng.close()


def test_job_sums_are_the_reference_on_the_history(first_job):
    """MALA on the diagonal Gaussian, D = 3, 70 chains, 50 steps, burn-in 10, thinning 3, 7 transitions per launch, closure (a)"""
    s, q, n, _ = _sums_equal_reference(first_job, "MALA d3")
    assert n == NSAVED and s.shape == (NCH, 2)


def test_job_moments_and_rhat_are_the_coordinate_reductions(first_job):
    s, q, n = first_job.derived_sums()
    inp = _inputs(s, q, n)
    mean, m2, ns, nc = first_job.derived_moments()
    mm, mq = P.mirror(inp)
    assert (ns, nc) == (NSAVED * NCH, NCH) and R.bits_differ(mean, mm) == 0 and R.bits_differ(m2, mq) == 0
    ex = P.exact(inp)
    rel, absmean = P.bound(NCH, ex)
    print(f"derived moments: worst M2 error / bound {np.max(np.abs(m2 - ex['M2']) / ex['M2'] / rel):.3g}, mean error / bound {np.max(np.abs(mean - ex['mean']) / absmean):.3g}")
    assert np.all(rel <= P.CAP) and np.all(np.abs(m2 - ex["M2"]) <= rel * ex["M2"]) and np.all(np.abs(mean - ex["mean"]) <= absmean)
    got = first_job.derived_rhat()
    worst = RH.check(got, RH.mirror(inp=inp), RH.exact(inp=inp), what="derived rhat")
    print(f"derived rhat {got['rhat']}: worst error / bound {worst:.3g}")
    assert got["nchains"] == NCH and got["nper"] == NSAVED and np.all(np.isfinite(got["rhat"])) and np.all(got["rhat"] > 0.9)


def test_job_histogram_is_the_histogram_of_the_host_values(first_job):
    _, _, _, ry = _sums_equal_reference(first_job, "MALA d3 (histogram)")
    m = first_job.derived.marginals
    counts, edges, ns, nc = first_job.derived_histogram()
    want = K.stats.pooled_hist(ry, m.nbins, m.lo, m.hi)
    assert (ns, nc) == (NSAVED * NCH, NCH) and counts.shape == (2, 18) and edges.shape == (2, 17)
    assert np.array_equal(counts, want) and np.all(counts.sum(axis=1) == ns)
    probs = [0.025, 0.5, 0.975]
    assert R.bits_differ(K.histogram_quantiles(counts, m.nbins, m.lo, m.hi, probs), K.stats.hist_quantiles(want, m.nbins, m.lo, m.hi, probs)) == 0


def test_job_invariances(first_job):
    """the value ring instead of a history, a run cut as 13 + 37, another launch length: the same sums and counts; the chains do not learn of the closure;
    reset clears; a job without the feature gets KLARA_ERR_STATE from the four calls"""
    s, q, n = first_job.derived_sums()
    counts = first_job.derived_histogram()[0]
    state, acc, csum = first_job.state(), first_job.accept_counts(), first_job.chain_sums()
    for what, kw in (("ring of 32", dict(monitor=L.MON_ACCEPT | L.MON_SUMMARIES)), ("13 + 37", dict(monitor=L.MON_HISTORY | L.MON_ACCEPT | L.MON_SUMMARIES, run=[13, 37])),
                     ("ring, default launch length", dict(monitor=L.MON_ACCEPT | L.MON_SUMMARIES, spl=0))):
        eng = _mala(**kw)
        s2, q2, n2 = eng.derived_sums()
        assert n2 == n and R.bits_differ(s2, s) == 0 and R.bits_differ(q2, q) == 0 and np.array_equal(eng.derived_histogram()[0], counts), what
        eng.close()
    plain = _mala(L.MON_HISTORY | L.MON_ACCEPT | L.MON_SUMMARIES, derived=None)
    for a, b in zip(state, plain.state()):
        assert R.bits_differ(a, b) == 0
    assert np.array_equal(acc[0], plain.accept_counts()[0])
    for a, b in zip(csum[:2], plain.chain_sums()[:2]):
        assert R.bits_differ(a, b) == 0
    lib, h = plain._lib, plain._h
    assert lib.klara_get_derived_sums(h, None, None, None) == L.ERR_STATE and lib.klara_gather_derived_moments(h, None, None, None, None, None) == L.ERR_STATE
    assert lib.klara_gather_derived_rhat(h, None, None, None, None, None, None, None) == L.ERR_STATE
    assert lib.klara_gather_derived_histogram(h, None, None, None, None) == L.ERR_STATE
    plain.close()
    nohist = _mala(L.MON_SUMMARIES, derived=K.Derived(DC.K_A, DC.SRC_A), run=[BURNIN])
    assert nohist._lib.klara_gather_derived_histogram(nohist._h, None, None, None, None) == L.ERR_STATE      # derived_nbins = 0
    s0, q0, n0 = nohist.derived_sums()                                        # before the first saved sample: zeros, NaN for R-hat, KLARA_OK
    assert n0 == 0 and not s0.any() and not q0.any() and nohist.derived_moments()[2] == 0 and np.all(np.isnan(nohist.derived_rhat()["rhat"]))
    nohist.run(NSTEPS - BURNIN)
    assert R.bits_differ(nohist.derived_sums()[0], s) == 0                    # (the kernel without staging, in a job)
    nohist.reset()
    s0, q0, n0 = nohist.derived_sums()
    assert n0 == 0 and not s0.any() and not q0.any()
    nohist.close()
    eng = _mala(L.MON_SUMMARIES)
    eng.reset()
    assert eng.derived_sums()[2] == 0 and not eng.derived_sums()[0].any() and not eng.derived_histogram()[0].any()
    eng.close()


def test_job_swiss_predictive_probability():
    """the swiss logistic regression, MALA, 128 chains, 40 steps, closure (c) at a covariate row: kd_exp's tables in the closure's kernel"""
    X, y = cases.swiss_data()
    x0 = np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(1).standard_normal((128, 4))
    row = X[3].copy()
    der = K.Derived(DC.K_C, DC.SRC_C, data=row, marginals=K.Marginals(64, 0.0, 1.0))
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), nchains=128, nsteps=40, burnin=10, driftstep=0.1, seed=20261020,
                   monitor=L.MON_HISTORY | L.MON_SUMMARIES, derived=der)
    eng.set_state(x0); eng.run(40)
    s, q, n, ry = _sums_equal_reference(eng, "swiss")
    assert n == 30 and np.all((ry > 0.0) & (ry < 1.0))
    counts = eng.derived_histogram()[0]
    assert np.array_equal(counts, K.stats.pooled_hist(ry, 64, 0.0, 1.0)) and counts[0, 0] == counts[0, -1] == 0
    mean = eng.derived_moments()[0]
    assert abs(mean[0] - ry.mean()) < 1e-12
    eng.close()


def test_job_user_defined_target_holds_two_modules():
    """cases.py's quartic as KLARA_TARGET_CUSTOM with closure (a): the target's run-time module and the closure's in one handle"""
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.CustomTarget(10, cases.SRC_QUARTIC_CHAIN, [0.1, 0.7]), nchains=70, nsteps=30, burnin=5, driftstep=0.05,
                   seed=20261020, monitor=L.MON_HISTORY | L.MON_SUMMARIES, derived=K.Derived(DC.K_A, DC.SRC_A))
    eng.init_state_normal(); eng.run(30)
    _, _, n, _ = _sums_equal_reference(eng, "quartic")
    assert n == 25
    eng.close()


def test_job_through_the_klara_api():
    p = K.BasicContMuvParameter("p", logtarget=K.GaussDiagTarget.negdot(3))
    job = K.BasicMCJob(K.likelihood_model(p, False), K.MALA(0.3), K.BasicMCRange(nsteps=60, burnin=10), {"p": np.zeros((64, 3))},
                       derived=K.Derived(DC.K_A, DC.SRC_A, marginals=K.Marginals(16, -3.0, 3.0)), outopts={"destination": "none"})
    K.run(job)
    mean, var, rh, qt = K.derived_mean(job), K.derived_var(job), K.derived_rhat(job), K.derived_quantiles(job, [0.025, 0.5, 0.975])
    assert mean.shape == var.shape == rh.shape == (2,) and qt.shape == (2, 3) and np.all(var > 0) and np.all(np.abs(mean) < 0.5)
    assert np.all(qt[:, 0] < qt[:, 1]) and np.all(qt[:, 1] < qt[:, 2])
    job.close()


_CANARY = r'''
import sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import klara_jl_amd as K
import derived_cases as DC
from klara_jl_amd import _lib as L
e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(3), driftstep=0.3, nsteps=50, nchains=70, burnin=10, thinning=3,
             monitor=L.MON_HISTORY | L.MON_ACCEPT | L.MON_SUMMARIES, seed=20261020, steps_per_launch=7,
             derived=K.Derived(DC.K_A, DC.SRC_A, marginals=K.Marginals(16, [-3.0, -2.0], [3.0, 2.0])))
e.init_state_normal(); e.run(50)
s, q, n = e.derived_sums()
counts, _, ns, nc = e.derived_histogram()
assert n == 14 and np.all(np.isfinite(s)) and np.all(counts.sum(axis=1) == ns) and e.derived_moments()[2] == ns and e.derived_rhat()["nper"] == n
e.close()                                                 # klara_destroy: KLARA_OK only with every canary intact
print("INTACT")
'''


def test_job_between_canaries():
    """the first job once more with every device array between canaries (KLARA_DEBUG_CANARY=1, a child process as tests/test_gpu_canary.py runs its own):
    klara_destroy returns KLARA_OK, so neither kernel wrote outside its arrays"""
    env = dict(os.environ, KLARA_DEBUG_CANARY="1")
    r = subprocess.run([sys.executable, "-c", _CANARY.replace("ROOT", str(ROOT))], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("INTACT"), r.stdout
