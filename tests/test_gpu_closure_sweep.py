"""The run-time compiled closure kernels over every plan shape (-m gpu): one job per class of tests/closure_sweep.py, every comparison bit for bit against
the CPU oracle (oracle_ffi.OracleJob) or, for the autodiff jobs, against the host build stepped by it (autodiff_ref.ref_job).  Both compile the same C
text with the host compiler and sum in the (0, G, E) order the device reports, so no tolerance appears anywhere in this file.

 (a) two rows of LDS per chain (x, gradient), the quartic chain: the 24 (G, E, wpb) classes of klara_plan.h custom_layout over D = 33 .. 1024;
 (b) three rows (x, gradloglikelihood, gradlogprior), the COUPLED likelihood + prior closure: the 23 classes, at a D whose row stride carries the 2-double
     pad wherever the class has one and at an unpadded neighbour — 40 plans.  The named likelihood + prior case (staged_normal_normal_mala_d48) is separable:
     no lane needs another lane's element of a row, so a `ts` row that is one element short, or aliased onto the next chain's x, can stay silent there
     (tests/test_closure_sweep_host.py test_a_shifted_third_row_is_silent_on_a_separable_target shows it on the host).  Here every gradient element reads its
     two neighbours, the first and last element of every lane included;
 (c) the same job at 2 and at 4 wavefronts per workgroup: nothing but a chain's row index inside its workgroup differs;
 (d) staged forward-mode autodiff (CustomTarget::ad_staged) at E = 8, 10, 12, 14, 16, at wpb = 2, at G = 64, in the likelihood + prior form, and at a chunk
     width that divides neither E nor the default;
 (e) pair closures on the few-lanes kernels (k_diagt<.., USERPAIR>) at the dimensions of the built-in target's sweep.

Every job has one full workgroup, one full wavefront of a second and one chain in a third, runs all its transitions in ONE launch with running sums and
value / log-target / gradient histories on, and has passed its acceptance window on the oracle alone in tests/test_closure_sweep_host.py."""
import ctypes as C

import numpy as np
import pytest

import autodiff_ref as R
import cases
import closure_sweep as S
import klara_jl_amd as K
import oracle_ffi as O
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

NOGRAD = (L.SAMPLER_MH, L.SAMPLER_SLICE)


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in ("KLARA_CUSTOM_LANES", "KLARA_CUSTOM_WPB"):
        monkeypatch.delenv(name, raising=False)


def _run(case, mon, ad=False, spl=0):
    eng = K.Engine(**cases.engine_kwargs(case, monitor=mon, steps_per_launch=spl, **(dict(nstreams=1) if spl == 0 else {})))
    layout = eng.layout()
    job = (R.ref_job(case, layout=layout, want_hist=True) if ad else O.OracleJob(**cases.oracle_kwargs(case, layout=layout), want_hist=True))
    eng.set_state(case["x0"]); assert job.set_state(case["x0"]) == 0
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), f"{case['name']}: initial state differs"
    if case["sampler"] not in NOGRAD:
        assert np.array_equal(g, job.G), f"{case['name']}: initial gradient differs"
    eng.run(case["nsteps"]); assert job.run(case["nsteps"]) == 0
    return eng, job


def _assert_same(eng, job, case):
    """what tests/test_gpu_parity.py _assert_same compares, and the histories of the first, a middle and the last chain"""
    name, grad = case["name"], case["sampler"] not in NOGRAD
    mask = eng.accept_mask()
    assert mask.shape == job.accept.shape
    assert np.array_equal(mask, job.accept), f"{name}: accept mask differs at {np.argwhere(mask != job.accept)[:5]}"
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X), f"{name}: values differ at {np.argwhere(x != job.X)[:5]}"
    assert np.array_equal(lt, job.LT), f"{name}: log-target differs"
    if grad:
        assert np.array_equal(g, job.G), f"{name}: gradient differs at {np.argwhere(g != job.G)[:5]}"
    s, q, nsaved = eng.chain_sums()
    assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), f"{name}: per-chain sums differ"
    assert nsaved == len(range(case.get("burnin", 0) + 1, case["nsteps"] + 1, case.get("thinning", 1)))
    na, nst = eng.accept_counts()
    assert np.array_equal(na, job.naccept) and nst == case["nsteps"]
    step, acc, prop, tot = eng.tune()
    if case.get("tuner_mode", 0) == L.TUNE_POOLED:
        assert step[0] == job.step[0] and acc[0] == job.accepted[0] and prop[0] == job.proposed[0] and tot[0] == job.totproposed[0]
    else:
        assert np.array_equal(step, job.step, equal_nan=True), f"{name}: tuned step differs"
        assert np.array_equal(acc, job.accepted) and np.array_equal(prop, job.proposed) and np.array_equal(tot, job.totproposed)
    if case.get("tuner", 0) == L.TUNER_DUAL_AVERAGING:
        eb, hb = eng.dual_averaging()
        assert np.array_equal(eb, job.da_epsbar) and np.array_equal(hb, job.da_hbar), f"{name}: dual-averaging state differs"
    ps, pq, pna, pnt, pns = eng.pooled_summaries()          # (device tree-sum against numpy's: 1e-12 relative, as in test_gpu_parity.py — another association)
    assert np.allclose(ps, job.sum.sum(0), rtol=1e-12, atol=1e-9) and np.allclose(pq, job.sumsq.sum(0), rtol=1e-12)
    assert pna == int(job.naccept.sum()) and pnt == case["nsteps"] * case["nchains"] and pns == nsaved
    for ch in (0, case["nchains"] // 2, case["nchains"] - 1):
        assert np.array_equal(eng.chain(ch), job.hist[:, ch, :].T), f"{name}: value history of chain {ch} differs"
        lt_h, g_h = eng.chain_fields(ch, logtarget=True, gradlogtarget=grad)
        assert np.array_equal(lt_h, job.hist_lt[:, ch]), f"{name}: log-target history of chain {ch} differs"
        if grad:
            assert np.array_equal(g_h, job.hist_g[:, ch, :].T), f"{name}: gradient history of chain {ch} differs"


def _rate(job, case):
    rate = float(job.accept.mean())
    assert rate == 1.0 if case["sampler"] == L.SAMPLER_SLICE else 0.05 < rate < 0.95, rate
    return rate


# ---- (a)
@pytest.mark.parametrize("d,kind", S.TWO_ROW_JOBS, ids=[f"d{d}-{k}" for d, k in S.TWO_ROW_JOBS])
def test_two_row_plan_classes(d, kind):
    case = S.staged_case(2, d, kind)
    g, e, wpb, padded = S.plan(d, 2)
    eng, job = _run(case, S.monitor(case))
    assert eng.layout() == (0, g, e), (eng.layout(), (g, e))
    print(f"(G={g}, E={e}, wpb={wpb}, pad={int(padded)}) -> D={d} {kind}: {case['nchains']} chains, acceptance {_rate(job, case):.3f}")
    _assert_same(eng, job, case)
    eng.close()


# ---- (b)
@pytest.mark.parametrize("d,kind", S.THREE_ROW_JOBS, ids=[f"d{d}-{k}" for d, k in S.THREE_ROW_JOBS])
def test_three_row_plan_classes(d, kind):
    """The coupled likelihood + prior closure.  A deliberately separable target in its place would no longer tell a shifted `ts` row from the right one at
    the elements a lane does not own (module docstring); with the coupling term every element of both gradient rows depends on its neighbours."""
    case = S.staged_case(3, d, kind)
    g, e, wpb, padded = S.plan(d, 3)
    eng, job = _run(case, S.monitor(case, lllp=True))
    assert eng.layout() == (0, g, e), (eng.layout(), (g, e))
    print(f"(G={g}, E={e}, wpb={wpb}, pad={int(padded)}) -> D={d} {kind}: {case['nchains']} chains, acceptance {_rate(job, case):.3f}")
    _assert_same(eng, job, case)
    if case["sampler"] not in NOGRAD:
        # the :loglikelihood / :logprior histories against the host build of the two functions at the stored states; ll + lp is the log-target history
        t = case["target"]
        lib = O.compile_user_target(t.source, d)[0]
        dp = C.POINTER(C.c_double)
        for f in (lib.klara_user_loglikelihood, lib.klara_user_logprior):
            f.restype, f.argtypes = C.c_double, [dp, C.c_int, dp, C.c_longlong]
        for ch in (0, case["nchains"] // 2, case["nchains"] - 1):
            v = eng.chain(ch); lt_h, _ = eng.chain_fields(ch); ll, lp = eng.chain_likelihood_prior(ch)
            assert ll.shape == lt_h.shape and np.array_equal(ll + lp, lt_h), f"ll + lp of chain {ch} is not its log-target history"
            for i in range(v.shape[1]):
                xi = np.ascontiguousarray(v[:, i])
                assert ll[i] == lib.klara_user_loglikelihood(xi.ctypes.data_as(dp), d, t.data.ctypes.data_as(dp), t.data.size), (ch, i)
                assert lp[i] == lib.klara_user_logprior(xi.ctypes.data_as(dp), d, t.data.ctypes.data_as(dp), t.data.size), (ch, i)
    eng.close()


# ---- (c)
@pytest.mark.parametrize("rows,d,kind", S.WPB_JOBS, ids=[f"rows{r}-d{d}-{k}" for r, d, k in S.WPB_JOBS])
def test_workgroup_shape_does_not_change_the_bits(rows, d, kind, monkeypatch):
    g, e, _, _ = S.plan(d, rows)
    case = S.staged_case(rows, d, kind, n=4 * (64 // g) + 64 // g + 1)
    out = []
    for wpb in ("2", "4"):
        monkeypatch.setenv("KLARA_CUSTOM_WPB", wpb)
        assert S.plan(d, rows)[:3] == (g, e, int(wpb))
        eng, job = _run(case, S.monitor(case))
        assert eng.layout() == (0, g, e), (wpb, eng.layout())
        _rate(job, case)
        _assert_same(eng, job, case)
        out.append(eng.state() + (eng.accept_mask(),) + tuple(eng.chain_sums()[:2]))
        eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b), "the two workgroup shapes give different bits"


# ---- (d)
def _ad_run(rows, d, kind, chunk):
    case = S.ad_case(rows, d, kind, chunk)
    eng, job = _run(case, S.monitor(case), ad=True)
    assert eng.layout() == (0,) + S.AD_EXPECTED[(rows, d)][:2], eng.layout()
    _rate(job, case)
    _assert_same(eng, job, case)
    out = eng.state() + (eng.accept_mask(),)
    eng.close()
    return out


@pytest.mark.parametrize("rows,d,kind,chunk", [j for j in S.AD_JOBS if j[3] == 0], ids=[f"rows{r}-d{d}-{k}" for r, d, k, c in S.AD_JOBS if c == 0])
def test_staged_autodiff_plan_shapes(rows, d, kind, chunk):
    assert S.plan(d, rows)[:3] == S.AD_EXPECTED[(rows, d)]
    _ad_run(rows, d, kind, chunk)


def test_staged_autodiff_chunk_that_divides_nothing():
    """E = 12 at KLARA_USER_AUTODIFF_CHUNK 5 (sweeps of 5, 5 and 2 directions: the c0 + k < E guard works) against the host build, and — invariant A2 — the
    bits of the library's chunk of 4"""
    (rows, d, kind, chunk), = [j for j in S.AD_JOBS if j[3]]
    assert S.plan(d, rows)[1] == 12 and chunk == 5
    for a, b in zip(_ad_run(rows, d, kind, 0), _ad_run(rows, d, kind, chunk)):
        assert np.array_equal(a, b)


# ---- (e)
@pytest.mark.parametrize("d,kind", S.PAIR_JOBS, ids=[f"d{d}-{k}" for d, k in S.PAIR_JOBS])
def test_pair_closure_dimension_sweep(d, kind):
    case = S.pair_case(d, kind)
    eng, job = _run(case, L.MON_ACCEPT | L.MON_SUMMARIES, spl=2)
    assert eng.layout() == (3, S.pair_lanes(d), 2 * ((d + 2 * S.pair_lanes(d) - 1) // (2 * S.pair_lanes(d)))), eng.layout()
    x, lt, g = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), d
    assert case["sampler"] in NOGRAD or np.array_equal(g, job.G), d
    assert np.array_equal(eng.accept_counts()[0], job.naccept), d
    assert np.array_equal(eng.accept_mask(), job.accept), d
    eng.close()
