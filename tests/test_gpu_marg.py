"""The pooled marginal histograms on the device (klara_marg.hip's k_marg_update behind every launch of a job with klara_desc.marg_nbins > 0,
klara_gather_histogram) against klara_jl_amd.stats.pooled_hist, the literal NumPy form of the index formula: counts are integers and every comparison is
exact.  Through klara_selftest_marginals at the smallest shapes at which the kernel can still go wrong — a chain count that is no multiple of 4 or 64, a
single chain, fewer dimensions than lanes (the lanes of one instruction collide in one table), a width that is no multiple of 64, more than one dimension
block, one bin to 1,024, more than one chain slab, 33 saved steps cut three ways — on histories built on purpose (every edge and its neighbours, the
infinities and NaN, every sample in one slot, bounds that differ per dimension, an offset of 1e6 at width 1e-3), and through small jobs of every launch
path.  tests/test_marg_host.py holds the NumPy forms themselves to values known by construction."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import klara_jl_amd as K
import marg_ref as R
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]
ROOT = Path(__file__).resolve().parent.parent


def check(hist, nbins, lo, hi, what, splits_list):
    want = R.reference(hist, nbins, lo, hi)
    assert int(want.sum()) == hist.size
    for name, splits in splits_list:
        got = R.selftest(hist, splits, nbins, lo, hi)
        diff = int(np.count_nonzero(got != want))
        print(f"marg {what}, splits {name}: {hist.size} samples, slots differing {diff}; outer counts {int(want[:, 0].sum())} / {int(want[:, -1].sum())}")
        assert got.dtype == np.uint64 and diff == 0, (what, name)
    return want


# ---------------------------------------------------------------- through the self test
@pytest.mark.parametrize("nbins", R.BINS)
@pytest.mark.parametrize("D", R.DIMS)
def test_selftest_every_width_and_bin_count(D, nbins):
    """N = 67 chains, 33 saved steps cut as 1 + 31 + 1, 32 + 1 and 0 + 32 + 1 + 0: the same counts for every cut, all equal to the reference"""
    hist = R.make_hist(R.NCOLS, R.N_ODD, D)
    lo, hi = R.bounds(D)
    check(hist, nbins, lo, hi, f"N={R.N_ODD} D={D} nbins={nbins}", list(R.SPLITS33.items()))


@pytest.mark.parametrize("D", [1, 100])
def test_selftest_a_single_chain(D):
    hist = R.make_hist(R.NCOLS, 1, D)
    lo, hi = R.bounds(D)
    check(hist, 64, lo, hi, f"N=1 D={D}", list(R.SPLITS33.items()))


@pytest.mark.parametrize("nbins", R.BINS)
@pytest.mark.parametrize("kind", ["per_dim", "offset"])
def test_selftest_edges_infinities_and_nan(kind, nbins):
    """values exactly on every documented edge and one ulp to either side, at lo, at hi, just below lo, just below hi, +-inf, NaN, +-1e308; bounds that
    differ per dimension, and an offset of 1e6 with width 1e-3.  At the edges the index formula decides, on the device as in NumPy"""
    for D in (3, 66):
        hist, lo, hi = R.edge_hist(R.N_ODD, D, nbins, kind)
        want = check(hist, nbins, lo, hi, f"edges {kind} D={D} nbins={nbins}", [("pieces", R.splits_of(hist.shape[0]))])
        assert np.all(want[:, 0] >= 3) and np.all(want[:, -1] >= 5)             # < lo: nextafter(lo), -inf, -1e308; not < hi: hi, its successor, +inf, NaN, 1e308


@pytest.mark.parametrize("D", [3, 64])
def test_selftest_every_sample_in_one_slot(D):
    """the most contended LDS word: every chain of more than one slab, every saved step, one value — in an inner slot, then in each outer one"""
    N = R.slab(64) + 5
    lo, hi = R.bounds(D)
    for v, slot in ((0.25 * lo + 0.75 * hi, None), (lo - 1.0, 0), (hi + 1.0, 65)):
        hist = np.ascontiguousarray(np.broadcast_to(v, (4, N, D)))
        want = check(hist, 64, lo, hi, f"one slot D={D}", [("4", [4]), ("1+3", [1, 3])])
        assert np.all((want != 0).sum(axis=1) == 1) and np.all(want.max(axis=1) == 4 * N)
        if slot is not None:
            assert np.all(want[:, slot] == 4 * N)


@pytest.mark.parametrize("nbins", [64, 1024])
def test_selftest_more_than_one_chain_slab(nbins):
    """2 slabs and 5 chains at 64 bins (slab 256), 1 slab and 3 chains at 1,024 (slab 1,280): the ragged last slab, the slabs' tables folded into one"""
    N = (2 * R.slab(nbins) + 5) if nbins == 64 else R.slab(nbins) + 3
    assert N > R.slab(nbins)
    hist = R.make_hist(5, N, 17)
    lo, hi = R.bounds(17)
    check(hist, nbins, lo, hi, f"N={N} D=17 nbins={nbins}", [("5", [5]), ("2+0+3", [2, 0, 3])])


def test_selftest_refuses_bad_arguments():
    hist = R.make_hist(4, 3, 2)
    lo, hi = R.bounds(2)
    assert R.selftest(hist, [5], 8, lo, hi, status=True) == L.ERR_INVALID_ARG and R.selftest(hist, [2, -1, 3], 8, lo, hi, status=True) == L.ERR_INVALID_ARG
    assert R.selftest(R.make_hist(33, 2, 2), [33], 8, lo, hi, status=True) == L.ERR_INVALID_ARG
    assert R.selftest(hist, [4], 0, lo, hi, status=True) == L.ERR_INVALID_ARG and R.selftest(hist, [4], 1025, lo, hi, status=True) == L.ERR_INVALID_ARG
    assert R.selftest(hist, [4], 8, hi, lo, status=True) == L.ERR_INVALID_ARG and R.selftest(hist, [4], 8, lo, lo, status=True) == L.ERR_INVALID_ARG
    assert R.selftest(hist, [4], 8, lo, hi, status=True) == L.OK and R.selftest(hist, [0, 4, 0], 8, lo, hi, status=True) == L.OK


# ---------------------------------------------------------------- through the API
NCH, BURNIN, THIN, NSTEPS = 256, 10, 3, 200
MARG = K.Marginals(64, -2.5, 3.0)                # MALA on exp(-x.x): sd 0.71 — both outer slots stay populated by a few samples


def _mala(monitor, marginals=MARG, run=None, spl=0, nsteps=NSTEPS, D=100, nchains=NCH):
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.05, nsteps=nsteps, nchains=nchains, burnin=BURNIN, thinning=THIN,
                   monitor=monitor, seed=20261019, steps_per_launch=spl, marginals=marginals)
    eng.init_state_normal()
    for n in ([nsteps] if run is None else run):
        eng.run(n)
    return eng


def _history(eng):
    """(nsaved, N, D) from the read-back chains"""
    return np.ascontiguousarray(np.stack([eng.chain(c) for c in range(eng.nchains)], axis=0).transpose(2, 0, 1))


def _want(eng):
    m = eng.marginals
    return R.reference(_history(eng), m.nbins, m.lo, m.hi)


def test_job_counts_are_the_histogram_of_the_history():
    """MALA on the diagonal Gaussian, 256 chains x D = 100, 200 steps, burn-in 10, thinning 3.  With the value history and marginals: the counts are
    stats.pooled_hist of the history read back.  Without a history — the monitor's own 32-column ring — and run as 150 + 37 + 13: the same counts; at 7
    transitions per launch: the same.  State and accept counts are those of the job without marginals, bit for bit."""
    full = _mala(L.MON_HISTORY | L.MON_ACCEPT)
    counts, edges, ns, nc = full.pooled_histogram()
    nsaved = (NSTEPS - BURNIN - 1) // THIN + 1
    want = _want(full)
    assert (ns, nc) == (nsaved * NCH, NCH) and counts.shape == (100, 66) and edges.shape == (100, 65)
    print(f"marg job: {ns} samples per dimension, slots differing {int(np.count_nonzero(counts != want))}, outer counts {int(counts[:, 0].sum())} / {int(counts[:, -1].sum())}")
    assert np.array_equal(counts, want) and np.all(counts.sum(axis=1) == ns)
    assert edges[0, 0] == -2.5 and edges[0, -1] == 3.0
    state, acc = full.state(), full.accept_counts()
    q = K.histogram_quantiles(counts, 64, -2.5, 3.0, [0.025, 0.5, 0.975])
    order = np.quantile(_history(full).reshape(-1, 100), [0.025, 0.5, 0.975], axis=0, method="inverted_cdf").T
    assert np.all(np.abs(q - order) <= 5.5 / 64 + 1e-12)                          # (one bin width: tests/test_marg_host.py derives the bound)
    full.close()
    plain = _mala(L.MON_HISTORY | L.MON_ACCEPT, marginals=None)                   # the same job without marginals: the same chains
    for a, b in zip(state, plain.state()):
        assert R.bits_differ(a, b) == 0
    assert np.array_equal(acc[0], plain.accept_counts()[0])
    assert plain._lib.klara_gather_histogram(plain._h, None, None, None, None) == L.ERR_STATE
    plain.close()
    for what, kw in (("ring only, three runs", dict(run=[150, 37, 13])), ("7 per launch", dict(spl=7)), ("one run", dict())):
        eng = _mala(L.MON_ACCEPT, **kw)
        c2, _, ns2, nc2 = eng.pooled_histogram()
        assert (ns2, nc2) == (ns, nc) and np.array_equal(c2, counts), what
        for a, b in zip(state, eng.state()):
            assert R.bits_differ(a, b) == 0, what
        assert np.array_equal(acc[0], eng.accept_counts()[0]), what
        eng.close()


def test_job_gather_mid_run_changes_nothing_and_reset_clears():
    eng = _mala(0, run=[BURNIN])
    counts, _, ns, nc = eng.pooled_histogram()                                    # before the first saved sample: zeros
    assert (ns, nc) == (0, NCH) and not counts.any()
    eng.run(54)
    mid, _, ns, _ = eng.pooled_histogram()                                        # mid-run: only reads
    assert ns == 18 * NCH and np.all(mid.sum(axis=1) == ns)
    eng.pooled_histogram()
    eng.run(NSTEPS - 64)
    end, _, ns_end, _ = eng.pooled_histogram()
    ref = _mala(0)
    want, _, ns_ref, _ = ref.pooled_histogram()
    assert ns_end == ns_ref and np.array_equal(end, want)
    for a, b in zip(eng.state(), ref.state()):
        assert R.bits_differ(a, b) == 0
    x = eng.state()[0]
    eng.reset(x)
    z, _, ns, _ = eng.pooled_histogram()
    assert ns == 0 and not z.any()
    eng.run(64)
    again, _, ns, _ = eng.pooled_histogram()
    full = _mala(L.MON_HISTORY, run=[])
    full.reset(x); full.run(64)
    assert ns == 18 * NCH and np.array_equal(again, _want(full)[:, :])            # (only the first 64 transitions' samples)
    eng.set_state(x)
    z, _, ns, _ = eng.pooled_histogram()
    assert ns == 0 and not z.any()
    eng.close(); ref.close(); full.close()


def _case_engine(name, marginals, **over):
    case = cases.make_case(name)
    eng = K.Engine(**cases.engine_kwargs(case, monitor=L.MON_HISTORY, marginals=marginals, **over))
    if case["x0"] is None:
        eng.init_state_normal()
    else:
        eng.set_state(case["x0"])
    eng.run(case["nsteps"])
    return eng


@pytest.mark.parametrize("name", ["mh_d100", "hmc_d100", "slice_d100_nostepout", "slice_d5", "hmc_dense_d300_split", "mala_swiss"])
def test_job_every_launch_path(name):
    """MH, HMC, the free-running and the lockstep slice sampler, a dense-split layout (a tile of 16 chains on a workgroup) and the row-split logistic
    kernels, each at the smallest size the suite's cases have: the consumer sits behind every launch path, and the chains do not learn of it"""
    m = K.Marginals(32, -3.0, 4.0) if name != "mala_swiss" else K.Marginals(32, -20.0, 25.0)
    eng = _case_engine(name, m)
    counts, _, ns, nc = eng.pooled_histogram()
    want = _want(eng)
    print(f"marg job {name}: {ns} samples per dimension, slots differing {int(np.count_nonzero(counts != want))}")
    assert ns > 0 and np.array_equal(counts, want)
    state = eng.state()
    eng.close()
    plain = _case_engine(name, None)
    for a, b in zip(state, plain.state()):
        assert R.bits_differ(a, b) == 0
    plain.close()


def test_job_d1024():
    eng = _mala(L.MON_HISTORY, marginals=K.Marginals(1024, np.linspace(-3.0, -2.0, 1024), 3.0), nsteps=40, D=1024, nchains=8)
    counts, edges, ns, nc = eng.pooled_histogram()
    assert (ns, nc) == (10 * 8, 8) and counts.shape == (1024, 1026) and np.array_equal(counts, _want(eng))
    eng.close()


def test_job_one_rank_communicator_equals_no_communicator(klib):
    eng = _mala(0)
    counts, _, ns, nc = eng.pooled_histogram()
    uid = (C.c_uint8 * 128)()
    L.check(klib.klara_comm_unique_id(uid), "comm_unique_id")
    comm = C.c_void_p()
    L.check(klib.klara_comm_init(C.byref(comm), 1, 0, uid, 0), "comm_init")
    try:
        c2, _, ns2, nc2 = eng.pooled_histogram(comm)
        p = K.BasicContMuvParameter("p", logtarget=K.GaussDiagTarget.negdot(3))
        job = K.BasicMCJob(K.likelihood_model(p, False), K.MALA(0.3), K.BasicMCRange(nsteps=60, burnin=10), {"p": np.zeros((64, 3))},
                           marginals=K.Marginals(16, -2.0, 2.0), outopts={"destination": "none"})
        K.run(job)
        jc, je = K.pooled_hist(job, comm)
        jq = K.pooled_quantiles(job, [0.5], comm)
    finally:
        L.check(klib.klara_comm_destroy(comm), "comm_destroy")
    assert (ns2, nc2) == (ns, nc) and np.array_equal(c2, counts)
    assert jc.shape == (3, 18) and je.shape == (3, 17) and np.all(jc.sum(axis=1) == 50 * 64) and jq.shape == (3, 1) and np.all(np.abs(jq) < 0.5)
    assert np.array_equal(K.pooled_hist(job)[0], jc)
    job.close(); eng.close()


_CANARY = r'''
import sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import klara_jl_amd as K
from klara_jl_amd import _lib as L
for D, N, nbins in ((100, 257, 64), (130, 70, 1024), (3, 5, 1)):
    e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=64, burnin=10, thinning=3, driftstep=0.05,
                 marginals=K.Marginals(nbins, -2.0, 2.5))
    e.init_state_normal(); e.run(64)
    counts, edges, ns, nc = e.pooled_histogram()
    assert ns == 18 * N and np.all(counts.sum(axis=1) == ns)
    e.close()                                                 # klara_destroy: KLARA_OK only with every canary intact
print("INTACT")
'''


def test_job_between_canaries():
    """every device array of a job with marginals between canaries (KLARA_DEBUG_CANARY=1, a child process as tests/test_gpu_canary.py runs its own):
    klara_destroy returns KLARA_OK, so the kernel wrote outside none of its arrays — at a ragged last slab, at ten dimension blocks, at D < 4"""
    env = dict(os.environ, KLARA_DEBUG_CANARY="1")
    r = subprocess.run([sys.executable, "-c", _CANARY.replace("ROOT", str(ROOT))], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("INTACT"), r.stdout
