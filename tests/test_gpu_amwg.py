"""The AMWG kernels on the GPU: bit for bit against the CPU reference (tests/amwg_ref.py) — X, LT, logσ, the window counts, the accepted proposals per
coordinate, the coordinate masks, the running sums and the histories —, launch-length and sharding invariance, a tuning event on a launch boundary,
klara_reset, the warm start, more than one chain group per wavefront, the getters' refusals and one job under the device arrays' canaries.  Small shapes:
1, 70 and 200 chains (a short last group), 40 - 60 transitions with period 5 (eight or more tuning events), burn-in and thinning above 1.  The
reference of a case is computed once (amwg_cases.reference) and shared."""
import numpy as np
import pytest

import amwg_cases as WC
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = WC.HIST


def _engine(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None):
    n = case["nchains"] if nchains is None else nchains
    eng = K.Engine(**WC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    eng.set_state(case["x0"][chain_offset:chain_offset + n])
    return eng


def _run_pair(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, runs=None):
    n = case["nchains"] if nchains is None else nchains
    eng = _engine(case, monitor, steps_per_launch, chain_offset, nchains)
    job = WC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
    assert job.set_state(case["x0"][chain_offset:chain_offset + n]) == 0
    for k in (runs or [case["nsteps"]]):
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_amwg_state(eng, job):
    ls, acc, nacc = eng.amwg_state()
    assert np.array_equal(ls, job.logsigma), "log proposal scales differ from the reference"
    assert np.array_equal(acc, job.accepted), "window counts differ from the reference"
    assert np.array_equal(nacc, job.naccept_coord), "accepted proposals per coordinate differ from the reference"


def _assert_same(eng, job, monitor=HIST):
    x, lt, _ = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    _assert_amwg_state(eng, job)
    a, n = eng.accept_counts()
    assert np.array_equal(a, job.naccept) and n == job.t
    if monitor & L.MON_ACCEPT:
        assert np.array_equal(eng.amwg_accept_mask(), job.masks), "coordinate masks differ from the reference"
        assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    if monitor & L.MON_SUMMARIES:
        s, q, _ = eng.chain_sums()
        assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    if monitor & L.MON_HISTORY:
        for c in sorted({0, job.N // 2, job.N - 1}):
            v = eng.chain(c)
            assert v.shape[1] > 0 and np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, _ = eng.chain_fields(c, logtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"


@pytest.mark.parametrize("name", WC.ALL)
def test_bit_exact_against_the_reference(gpu_required, name):
    case = WC.make(name)
    eng = _engine(case)
    assert eng.layout() == WC.default_layout(case), (eng.layout(), WC.default_layout(case))
    job = WC.reference(name)
    eng.run(case["nsteps"])
    _assert_same(eng, job)
    d = case["target"].ndims
    if name in WC.LOGIT:
        assert eng.layout() == {"swiss_d4": (2, 4, 4), "logit_d3": (0, 1, 4), "logit_d8": (2, 4, 8), "logit_d11": (2, 4, 16)}[name]
    else:
        assert eng.layout() == (0, 1, max(2, 1 << (d - 1).bit_length()))
    # a kernel that never adapts, never moves or always moves cannot pass: eight or more tuning events, every coordinate accepted and rejected somewhere
    assert case["nsteps"] // case["period"] >= 8
    assert not np.array_equal(job.logsigma, np.broadcast_to(case["amwg_logsigma0"], job.logsigma.shape))
    for i in range(d):
        assert 0.0 < ((job.masks >> i) & 1).mean() < 1.0, i
    assert case["burnin"] > 1 and case["thinning"] > 1
    eng.close()


@pytest.mark.parametrize("name", ["swiss_d4", "quad_d17"])
def test_job_without_a_monitor(gpu_required, name):
    """monitor 0: MODE 3, and in one-transition launches MODE 7"""
    case = WC.make(name)
    job = WC.reference(name)
    for spl in (0, 1):
        eng = _engine(case, monitor=0, steps_per_launch=spl)
        eng.run(case["nsteps"])
        _assert_same(eng, job, monitor=0)
        eng.close()


@pytest.mark.parametrize("name", ["logit_d8", "likprior_d5", "quad_d32"])
def test_one_transition_per_launch(gpu_required, name):
    """steps_per_launch 1 and 7 with every monitor: the scales and counts travel through memory between launches, the fold does not depend on the cut"""
    case = WC.make(name)
    job = WC.reference(name)
    for spl in (1, 7):
        eng = _engine(case, steps_per_launch=spl)
        eng.run(case["nsteps"])
        _assert_same(eng, job)
        eng.close()


def test_tuning_event_on_a_launch_boundary(gpu_required):
    """period 7: run(7); run(13) equals run(20), and both equal the reference (one tuning event ends the first run, the next falls inside the second)"""
    case = WC.make("quad_d3_p7")
    eng, job = _run_pair(case, runs=[7, 13])
    _assert_same(eng, job)
    whole = WC.reference("quad_d3_p7")
    assert np.array_equal(job.X, whole.X) and np.array_equal(job.logsigma, whole.logsigma) and np.array_equal(job.masks, whole.masks)
    one = _engine(case)
    one.run(20)
    _assert_same(one, whole)
    ls7 = WC.ref_job(case, layout=eng.layout())
    assert ls7.set_state(case["x0"]) == 0 and ls7.run(7) == 0
    assert not ls7.accepted.any() and not np.array_equal(ls7.logsigma, np.broadcast_to(case["amwg_logsigma0"], ls7.logsigma.shape))
    eng.close(); one.close()


def test_reset_and_warm_start(gpu_required):
    case = WC.make("logit_d3")
    n, d = case["nchains"], 3
    eng, job = _run_pair(case, runs=[13, 1, 9])
    _assert_same(eng, job)
    ls0 = np.broadcast_to(case["amwg_logsigma0"], (n, d))
    # reset(job): the next Philox key; logσ = logσ0, the counts and the schedule restart (W3)
    eng.reset(); assert job.reset() == 0
    ls, acc, nacc = eng.amwg_state()
    assert np.array_equal(ls, ls0) and not acc.any() and not nacc.any()
    eng.run(17); assert job.run(17) == 0
    _assert_same(eng, job)
    assert np.array_equal(job.logsigma != ls0, np.ones((n, d), bool))              # three tuning events in 17 transitions moved every scale
    # set_amwg_logsigma: a warm start from per-chain scales; the count, the window and the schedule are kept
    warm = np.log(np.random.default_rng(5).uniform(0.2, 1.5, (n, d)))
    eng.set_amwg_logsigma(warm); job.logsigma[...] = warm
    assert np.array_equal(eng.amwg_state()[0], warm) and np.array_equal(eng.amwg_state()[1], job.accepted)
    eng.run(6); assert job.run(6) == 0
    _assert_same(eng, job)
    with pytest.raises(K.KlaraError) as ei:
        bad = warm.copy(); bad[3, 1] = np.inf
        eng.set_amwg_logsigma(bad)
    assert ei.value.status == L.ERR_INVALID_ARG
    x1 = 0.1 * np.ones((n, d))
    eng.reset(x1); assert job.reset(x1) == 0
    assert np.array_equal(eng.amwg_state()[0], ls0)
    eng.run(11); assert job.run(11) == 0
    _assert_same(eng, job)
    eng.close()


@pytest.mark.parametrize("name", ["swiss_d4", "likprior_d16"])
def test_chain_offset_sharding(gpu_required, name):
    """two handles with chain_offset draw, move and adapt what one job of all chains does"""
    case = WC.make(name)
    n = case["nchains"]
    whole = WC.reference(name)
    cut = 33
    parts = []
    for off, k in ((0, cut), (cut, n - cut)):
        e = _engine(case, chain_offset=off, nchains=k)
        e.run(case["nsteps"])
        parts.append((e.state()[0], e.state()[1]) + e.amwg_state() + (e.amwg_accept_mask(),) + e.chain_sums()[:2])
        e.close()
    for i, ref in enumerate((whole.X, whole.LT, whole.logsigma, whole.accepted, whole.naccept_coord)):
        assert np.array_equal(np.concatenate([p[i] for p in parts]), ref), i
    assert np.array_equal(np.concatenate([p[5] for p in parts], axis=1), whole.masks)
    assert np.array_equal(np.concatenate([p[6] for p in parts]), whole.sum) and np.array_equal(np.concatenate([p[7] for p in parts]), whole.sumsq)


@pytest.mark.parametrize("name", ["swiss_d4", pytest.param(WC.WALK, id="quad_d5")])
def test_several_chain_groups_per_wavefront(gpu_required, monkeypatch, name):
    """KLARA_GROUPS_PER_WAVE=2: a persistent wavefront walks over two chain groups (13 groups of 16 chains on 8 wavefronts, 5 groups of 64 on 4), in fused
    and in one-transition launches"""
    monkeypatch.setenv("KLARA_GROUPS_PER_WAVE", "2")
    case = WC.make(name)
    job = WC.reference(name)
    for spl in (0, 1):
        eng = _engine(case, steps_per_launch=spl)
        groups = -(-case["nchains"] // (64 // eng.layout()[1]))
        assert groups > 4 * -(-(-(-groups // 2)) // 4), "no wavefront takes a second group"      # (workgroups of four wavefronts)
        eng.run(case["nsteps"])
        _assert_same(eng, job)
        eng.close()


def test_python_job_and_per_coordinate_acceptance(gpu_required):
    """BasicMCJob with MuvAMWG and RobertsRosenthalMCTuner: acceptance() gives the per-coordinate rates of naccept_coord"""
    case = WC.make("swiss_d4")
    t = case["target"]
    p = K.BasicContMuvParameter("p", logtarget=t)
    job = K.BasicMCJob(K.likelihood_model(p), K.MuvAMWG(np.full(4, 0.5)), K.BasicMCRange(nsteps=45, burnin=5, thinning=2), {"p": case["x0"]},
                       tuner=K.RobertsRosenthalMCTuner(period=5), seed=case.get("seed", 20260927), outopts={"diagnostics": ["accept"]})
    nrun = job.range.nsteps
    assert nrun == 44                                             # Julia's StepRange normalises `last`: the range 6:2:45 ends at 44 (BasicMCRange.jl:20)
    K.run(job)
    ref = WC.ref_job(case, layout=job.engine.layout())
    assert ref.set_state(case["x0"]) == 0 and ref.run(nrun) == 0
    rates = K.acceptance(K.output(job))
    assert rates.shape == (200, 4) and np.array_equal(rates, ref.naccept_coord.astype(np.float64) / float(nrun))
    assert np.array_equal(job.engine.amwg_state()[0], ref.logsigma) and np.array_equal(job.engine.state()[0], ref.X)
    job.close()


def test_getter_refusals(gpu_required):
    case = WC.make("logit_d3")
    eng = K.Engine(**WC.engine_kwargs(case, monitor=0))
    with pytest.raises(K.KlaraError) as ei:                       # before set_state
        eng.amwg_state()
    assert ei.value.status == L.ERR_STATE
    with pytest.raises(K.KlaraError) as ei:
        eng.set_amwg_logsigma(np.zeros(3))
    assert ei.value.status == L.ERR_STATE
    x0 = case["x0"].copy(); x0[5, 1] = np.nan
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.set_state(case["x0"])
    eng.run(3)
    with pytest.raises(K.KlaraError) as ei:                       # no KLARA_MON_ACCEPT: no coordinate masks
        eng.amwg_accept_mask()
    assert ei.value.status == L.ERR_STATE
    eng.close()
    kw = WC.engine_kwargs(case)
    kw.update(sampler=L.SAMPLER_MH, mh_sigma=np.ones(3), amwg_logsigma0=None, tuner=L.TUNER_VANILLA, targetrate=0.0)
    mh = K.Engine(**kw)
    mh.set_state(case["x0"])
    for call in (mh.amwg_state, mh.amwg_accept_mask, lambda: mh.set_amwg_logsigma(np.zeros(3))):
        with pytest.raises(K.KlaraError) as ei:
            call()
        assert ei.value.status == L.ERR_INVALID_ARG
    mh.close()


_CANARY_PROBE = r"""
import ctypes as C, sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import amwg_cases as WC
import klara_jl_amd as K
from klara_jl_amd import _lib as L
lib = L.load()
case = WC.make("logit_d11")
job = WC.reference("logit_d11")
eng = K.Engine(**WC.engine_kwargs(case, monitor=WC.HIST, steps_per_launch=7))
eng.set_state(case["x0"]); eng.run(case["nsteps"])
ls, acc, nacc = eng.amwg_state()
assert np.array_equal(eng.state()[0], job.X) and np.array_equal(ls, job.logsigma) and np.array_equal(acc, job.accepted) and np.array_equal(nacc, job.naccept_coord)
assert np.array_equal(eng.amwg_accept_mask(), job.masks)
na, nc = C.c_int64(0), C.c_int64(0)
L.check(lib.klara_selftest_canary(0, C.byref(na), C.byref(nc)), "klara_selftest_canary")
assert na.value >= 12 and nc.value == 0, (na.value, nc.value)
eng.close()                                                   # klara_destroy checks every array of the handle: raises on a damaged canary
print("INTACT", na.value)
"""


def test_amwg_arrays_under_the_canaries(gpu_required):
    """KLARA_DEBUG_CANARY=1 (read once per process: a child process) puts guard words around every device array of a handle — the AMWG scales, counts and
    coordinate masks are DeviceArrays allocations like the rest.  One job with every monitor, 70 chains on the row split (a short last group) and launches
    of 7: the results are the reference's, klara_selftest_canary finds nothing damaged and klara_destroy neither."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, "-c", _CANARY_PROBE.replace("ROOT", str(root))], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, KLARA_DEBUG_CANARY="1"), cwd=str(root))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].startswith("INTACT"), r.stdout
