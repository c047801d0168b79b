"""The pooled posterior covariance (klara_cov.hip: k_cov_update after every launch of a job with KLARA_MON_COVARIANCE, k_cov_finalize
behind klara_gather_covariance, klara_comm.hip's k_merge_between between ranks) against tests/cov_ref.py: bit for bit against the NumPy restatement of the order of operations on every element, and,
so that the mirror is never the only yardstick, against exact rational arithmetic within the derived bound on a fixed handful of (i, j) pairs that
includes both sides of the tile edges.  The kernels run on synthetic histories through klara_selftest_covariance (the launch functions of the job
path; klara_gather_covariance's own between-rank sequence, merge_ranks, with only the all-reduces swapped for ordered host sums) and in small jobs of every save path through the API.  The synthetic inputs are those
tests/test_cov_host.py checks on the CPU."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import cov_ref as R
import klara_jl_amd as K
import pooled_ref as P
from klara_jl_amd import _lib as L
from test_cov_host import OFFSET_SHAPE, RANK_SHAPE

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]
ROOT = Path(__file__).resolve().parent.parent
SENTINEL = -12345.5


def selftest(hist, splits, bounds=None, status=False):
    klib = L.load()
    ncols, N, D = hist.shape
    spl = np.asarray(splits, dtype=np.int64)
    b = np.asarray([0, N] if bounds is None else bounds, dtype=np.int64)
    out = {"mean": np.full(D, SENTINEL), "m2": np.full((D, D), SENTINEL), "ranks_mean": np.full(D, SENTINEL), "ranks_m2": np.full((D, D), SENTINEL)}
    cnt = np.zeros(2, dtype=np.uint64)
    st = klib.klara_selftest_covariance(0, N, D, ncols, hist.ctypes.data, spl.size, spl.ctypes.data, b.size - 1, b.ctypes.data, out["mean"].ctypes.data,
                                        out["m2"].ctypes.data, out["ranks_mean"].ctypes.data, out["ranks_m2"].ctypes.data, cnt.ctypes.data)
    if status:
        return st
    L.check(st, "klara_selftest_covariance")
    out["counters"] = tuple(int(v) for v in cnt)
    return out


def check_case(hist, what, splits, bounds=None):
    """one selftest run against the mirror (bits, all elements) and against exact (bound, the pairs); prints its figures first"""
    ncols, N, D = hist.shape
    out = selftest(hist, splits, bounds)
    mean, M = R.mirror(hist, splits)
    ex = R.exact(hist)
    E, Em = R.bound(hist)
    bits = {"mean": R.bits_differ(out["mean"], mean), "m2": R.bits_differ(out["m2"], M)}
    rm, rmean = R.errors(out["mean"], out["m2"], ex, E, Em)
    msg = f"cov {what}: values differing from the mirror {bits}; |M - exact| / bound {rm:.3g}, |mean - exact| / bound {rmean:.3g}"
    b = [0, N] if bounds is None else bounds
    gmean, gM, cnt, _ = R.mirror_ranks(hist, b, splits)
    Er, Emr = R.bound_ranks(hist, b)
    qm, qmean = R.errors(out["ranks_mean"], out["ranks_m2"], ex, Er, Emr)
    rbits = {"ranks_mean": R.bits_differ(out["ranks_mean"], gmean), "ranks_m2": R.bits_differ(out["ranks_m2"], gM)}
    print(msg + f"; {len(b) - 1} shard(s): {rbits}, |M - exact| / bound {qm:.3g}, |mean - exact| / bound {qmean:.3g}")
    assert not any(bits.values()) and not any(rbits.values()), (what, bits, rbits)
    assert rm <= 1.0 and rmean <= 1.0 and qm <= 1.0 and qmean <= 1.0, what
    assert out["counters"] == cnt == (ncols * N, N)
    assert R.bits_differ(out["m2"], out["m2"].T) == 0 and R.bits_differ(out["ranks_m2"], out["ranks_m2"].T) == 0
    return out


# ---------------------------------------------------------------- through the selftest
@pytest.mark.parametrize("N", R.CHAINS)
def test_selftest_every_chain_count(N):
    """D = 3, 200 saved steps, N over the slab's edges: fewer chains than a k-step (1, 3), exactly one (4), a ragged second (5), one short of a
    slab, a slab, a slab and one chain, two slabs and a ragged third."""
    check_case(R.make_hist(N, 3, 200), f"N={N}", R.splits_of(200), P.shard_bounds(N, 2) if N > 1 else None)


@pytest.mark.parametrize("D", R.DIMS)
def test_selftest_every_width(D):
    """N = 37, 9 saved steps, D over the tile edges: one partial tile, 15 / 16 / 17, two tiles and one more column, the headline's 100 (28 tiles, 7 per
    wavefront), 128 / 129, and 255 / 256 (136 tiles: three tile groups)."""
    check_case(R.make_hist(37, D, 9), f"D={D}", [9], [0, 1, 37])


def test_selftest_splits_give_the_same_bits():
    hist = R.make_hist(R.N_SPLIT, R.D_SPLIT, 70)
    res = {k: check_case(hist, f"splits {k}", s) for k, s in R.SPLITS70.items()}
    first = res["32+32+6"]
    for k, out in res.items():
        for key in ("mean", "m2", "ranks_mean", "ranks_m2"):
            assert R.bits_differ(out[key], first[key]) == 0, (k, key)


@pytest.mark.parametrize("offset", P.OFFSETS)
def test_selftest_offsets(offset):
    """0, 242, 1e4 and 1e6 sd off the origin: the bits stay the mirror's, and the bound on M — reported — does not grow: z = x - pivot does not carry
    the offset."""
    N, D, nc = OFFSET_SHAPE
    hist = R.make_hist(N, D, nc, offset)
    E, Em = R.bound(hist)
    print(f"cov bound at {offset:g} sd: M {E.max():.3g}, mean {Em.max():.3g}")
    check_case(hist, f"offset={offset:g}sd", R.splits_of(nc), P.shard_bounds(N, 3))


def test_selftest_constant_chains_are_exact():
    hist, v = R.const_hist(R.CH + 6, 5, 9)
    out = selftest(hist, [4, 5], [0, 30, R.CH + 6])
    assert np.all(out["m2"] == 0.0) and np.array_equal(out["mean"], v)
    E, Em = R.bound_ranks(hist, [0, 30, R.CH + 6])          # (the merged mean (n_1 x + n_2 x) / n is rounded: not part of the kernel's promise)
    assert np.all(np.abs(out["ranks_m2"]) <= E) and np.all(np.abs(out["ranks_mean"] - v) <= Em)


@pytest.mark.parametrize("nshards", [2, 3])
def test_selftest_shards(nshards):
    """2 x 64 + 5 chains, D = 17, at 1e4 sd with the halves 3 sd apart: n_r d d' is far from zero, so a wrong weight in the merge changes the result"""
    N, D, nc = RANK_SHAPE
    hist = R.make_hist(N, D, nc, 1e4)
    hist[:, N // 2:] += 3.0 * R.SD
    check_case(hist, f"{nshards} shards", R.splits_of(nc), P.shard_bounds(N, nshards))


def test_selftest_refuses_bad_arguments():
    hist = R.make_hist(3, 3, 4)
    assert selftest(hist, [5], status=True) == L.ERR_INVALID_ARG and selftest(hist, [2, -1, 3], status=True) == L.ERR_INVALID_ARG
    assert selftest(R.make_hist(2, 2, 33), [33], status=True) == L.ERR_INVALID_ARG
    for bounds in ([0, 2], [1, 3], [0, 2, 2, 3], [0, 2, 1, 3], [0, 4]):
        assert selftest(hist, [4], bounds, status=True) == L.ERR_INVALID_ARG, bounds
    klib = L.load()
    spl, b = np.array([4], np.int64), np.array([0, 3], np.int64)
    for N, D, nc, h in ((0, 3, 4, hist), (3, 0, 4, hist), (3, 257, 4, hist), (3, 3, 0, hist), (3, 3, 4, None)):
        st = klib.klara_selftest_covariance(0, N, D, nc, None if h is None else h.ctypes.data, 1, spl.ctypes.data, 1, b.ctypes.data, None, None, None, None, None)
        assert st == L.ERR_INVALID_ARG, (N, D, nc)
    assert selftest(hist, [4], status=True) == L.OK and selftest(hist, [0, 4, 0], status=True) == L.OK


# ---------------------------------------------------------------- through the API
NCH, BURNIN, THIN = 256, 10, 3


def _job_kwargs(name):
    rng = np.random.default_rng(20261019)
    if name == "mala_diag_d100":
        return dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(100), driftstep=0.05, nsteps=64), None
    if name == "hmc_dense_d100":
        return dict(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(cases.compound_symmetric_precision(100)), leapstep=0.1, nleaps=5, nsteps=64), None
    if name == "mala_swiss":
        X, y = cases.swiss_data()
        x0 = np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * rng.standard_normal((NCH, 4))
        return dict(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), driftstep=0.1, nsteps=96), x0
    if name == "hmc_rats":
        t = cases.rats_target()
        x0 = t.least_squares_start()[None, :] + 0.05 * rng.standard_normal((NCH, t.ndims))
        return dict(sampler=L.SAMPLER_HMC, target=t, leapstep=0.02, nleaps=5, nsteps=64), x0
    if name == "mala_closure_d20":
        return dict(sampler=L.SAMPLER_MALA, target=K.CustomTarget(20, cases.SRC_QUARTIC_CHAIN, [0.05, 0.3]), driftstep=0.1, nsteps=64), None
    if name == "slice_free_d100":
        return dict(sampler=L.SAMPLER_SLICE, target=K.GaussDiagTarget.negdot(100), slice_widths=1.5, nsteps=64), None
    raise KeyError(name)


JOBS = ["mala_diag_d100", "hmc_dense_d100", "mala_swiss", "hmc_rats", "mala_closure_d20", "slice_free_d100"]


def _run(name, monitor, spl=0, run=None, **over):
    kw, x0 = _job_kwargs(name)
    kw.update(over)
    eng = K.Engine(nchains=NCH, burnin=BURNIN, thinning=THIN, monitor=monitor, seed=20261019, steps_per_launch=spl, **kw)
    if x0 is None:
        eng.init_state_normal()
    else:
        eng.set_state(x0)
    for n in ([kw["nsteps"]] if run is None else run):
        eng.run(n)
    return eng


def _history(eng):
    """(nsaved, N, D) from the read-back chains"""
    return np.ascontiguousarray(np.stack([eng.chain(c) for c in range(eng.nchains)], axis=0).transpose(2, 0, 1))


@pytest.mark.parametrize("name", JOBS)
def test_job_covariance_every_save_path(name):
    """One small job per save path (256 chains, burn-in 10, thinning 3).  With the full value history and the bit: M against exact from the read-back
    histories within the bound, against the mirror bit for bit.  With the monitor's own 32-column ring only: the same bits; at 7 and at 32
    transitions per launch: the same bits; and the chains are those of the job without the bit, bit for bit."""
    full = _run(name, L.MON_HISTORY | L.MON_COVARIANCE)
    mean, M, ns, nc = full.pooled_covariance()
    hist = _history(full)
    nsaved = hist.shape[0]
    assert (ns, nc) == (nsaved * NCH, NCH) and nsaved == (full.nsteps - BURNIN - 1) // THIN + 1
    wm, wM = R.mirror(hist)
    ex = R.exact(hist)
    E, Em = R.bound(hist)
    rm, rmean = R.errors(mean, M, ex, E, Em)
    bits = (R.bits_differ(mean, wm), R.bits_differ(M, wM))
    print(f"cov job {name}: {nsaved} saved steps, values differing from the mirror {bits}; |M - exact| / bound {rm:.3g}, |mean - exact| / bound {rmean:.3g}")
    assert bits == (0, 0) and rm <= 1.0 and rmean <= 1.0
    assert R.bits_differ(M, M.T) == 0
    lit = K.stats.pooled_cov(np.transpose(hist, (1, 2, 0)))
    assert np.allclose(M / (ns - 1), lit, rtol=1e-9, atol=1e-12 * np.abs(lit).max())          # (the literal NumPy form: to rounding only)
    state = full.state()
    full.close()
    plain = _run(name, L.MON_HISTORY)                                            # the same job without the bit: the same chains
    for a, b in zip(state, plain.state()):
        assert R.bits_differ(a, b) == 0
    assert plain._lib.klara_gather_covariance(plain._h, None, None, None, None, None) == L.ERR_STATE
    plain.close()
    for what, kw in (("ring only", dict()), ("7 per launch", dict(spl=7)), ("32 per launch", dict(spl=32)), ("three runs", dict(run=[20, 1, full.nsteps - 21]))):
        eng = _run(name, L.MON_COVARIANCE, **kw)
        m2, M2, ns2, nc2 = eng.pooled_covariance()
        assert (ns2, nc2) == (ns, nc) and R.bits_differ(m2, mean) == 0 and R.bits_differ(M2, M) == 0, what
        for a, b in zip(state, eng.state()):
            assert R.bits_differ(a, b) == 0, what
        eng.close()


def test_job_reset_clears_and_the_first_samples_are_zeros():
    eng = _run("mala_diag_d100", L.MON_COVARIANCE, run=[BURNIN])
    mean, M, ns, nc = eng.pooled_covariance()                                    # before the first saved sample: zeros, as klara_gather_moments
    assert (ns, nc) == (0, NCH) and np.all(mean == 0.0) and np.all(M == 0.0)
    eng.run(54)
    first = eng.pooled_covariance()
    assert first[2] == 18 * NCH and first[1][0, 0] > 0.0
    x = eng.state()[0]
    eng.reset(x)
    z = eng.pooled_covariance()
    assert z[2] == 0 and np.all(z[0] == 0.0) and np.all(z[1] == 0.0)
    eng.run(64)
    again = eng.pooled_covariance()
    ref = _run("mala_diag_d100", L.MON_HISTORY | L.MON_COVARIANCE)
    ref.reset(x); ref.run(64)
    want = ref.pooled_covariance()
    wm, wM = R.mirror(_history(ref))
    assert R.bits_differ(again[0], want[0]) == 0 and R.bits_differ(again[1], want[1]) == 0 and R.bits_differ(want[1], wM) == 0 and R.bits_differ(want[0], wm) == 0
    eng.set_state(x)
    z = eng.pooled_covariance()
    assert z[2] == 0 and np.all(z[1] == 0.0)
    eng.close(); ref.close()


def test_job_diagonal_is_the_pooled_moments_m2():
    """diag(M) against klara_gather_moments' m2 on the rats model (means up to 242 sd off): within the sum of both bounds"""
    eng = _run("hmc_rats", L.MON_HISTORY | L.MON_SUMMARIES | L.MON_COVARIANCE)
    mean, M, ns, nc = eng.pooled_covariance()
    pm, pm2, pns, _, _, pnc = eng.pooled_moments()
    assert (ns, nc) == (pns, pnc)
    hist = _history(eng)
    E, Em = R.bound(hist)
    s, q, nsaved = eng.chain_sums()
    acc, _ = eng.accept_counts()
    inp = {"sum": s, "sumsq": q, "X": eng.state()[0], "held": np.zeros(NCH, dtype=np.int64), "naccept": acc, "nsaved": nsaved}
    relb, meanb = P.bound(NCH, P.exact(inp))
    d = np.abs(np.diag(M) - pm2)
    # pooled_ref's bound takes the chains' running sums as exact inputs, M does not come from them: the sums were added sample by sample in f64, so a
    # chain's sumsq is off by at most nsaved u sumsq and its sum by nsaved u |sum|, which moves sum^2 / nsaved by 2 nsaved u sum^2 / nsaved
    # <= 2 nsaved u sumsq: 3 nsaved u sumsq per chain, taken as 4 for the higher orders
    slack = 4.0 * nsaved * P.U * q.sum(axis=0)
    print(f"cov diagonal against pooled moments: largest |diag(M) - m2| / (bounds) {(d / (np.diag(E) + relb * pm2 + slack)).max():.3g}")
    assert np.all(d <= np.diag(E) + relb * pm2 + slack) and np.all(np.abs(mean - pm) <= Em + meanb)
    eng.close()


def test_job_one_rank_communicator_equals_no_communicator(klib):
    eng = _run("hmc_dense_d100", L.MON_HISTORY | L.MON_COVARIANCE)
    mean, M, ns, nc = eng.pooled_covariance()
    uid = (C.c_uint8 * 128)()
    L.check(klib.klara_comm_unique_id(uid), "comm_unique_id")
    comm = C.c_void_p()
    L.check(klib.klara_comm_init(C.byref(comm), 1, 0, uid, 0), "comm_init")
    try:
        cmean, cM, cns, cnc = eng.pooled_covariance(comm)
        out = K.gather_engine_covariance_klara(eng, type("Comm", (), {"handle": comm})())
    finally:
        L.check(klib.klara_comm_destroy(comm), "comm_destroy")
    hist = _history(eng)
    wm, wM, cnt, _ = R.mirror_ranks(hist, [0, NCH])                               # one rank's between-rank arithmetic: mean = (n mean_r) / n, M + n d d'
    assert (cns, cnc) == (ns, nc) == cnt
    assert R.bits_differ(cmean, wm) == 0 and R.bits_differ(cM, wM) == 0 and R.bits_differ(cM, cM.T) == 0
    E, Em = R.bound_ranks(hist, [0, NCH])
    E1, Em1 = R.bound(hist)
    assert np.all(np.abs(cM - M) <= E + E1) and np.all(np.abs(cmean - mean) <= Em + Em1)      # both within their bounds of the one exact value
    assert np.array_equal(out["m2"], cM) and np.array_equal(out["cov"], cM / (ns - 1))
    eng.close()


def test_job_wider_than_256_is_unsupported():
    with pytest.raises(K.KlaraError) as e:
        K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(257), nchains=8, nsteps=20, driftstep=0.05, monitor=L.MON_COVARIANCE)
    assert e.value.status == L.ERR_UNSUPPORTED
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(256), nchains=8, nsteps=20, driftstep=0.05, monitor=L.MON_COVARIANCE)
    eng.init_state_normal(); eng.run(20)
    mean, M, ns, nc = eng.pooled_covariance()
    assert (ns, nc) == (160, 8) and M.shape == (256, 256) and np.all(np.diag(M) > 0.0)
    eng.close()
    # through the job API: K.pooled_cov / K.pooled_cor of a BasicMCJob(covariance=True)
    p = K.BasicContMuvParameter("p", logtarget=K.GaussDiagTarget.negdot(3))
    job = K.BasicMCJob(K.likelihood_model(p, False), K.MALA(0.3), K.BasicMCRange(nsteps=60, burnin=10), {"p": np.zeros((64, 3))}, covariance=True,
                       outopts={"destination": "none"})
    K.run(job)
    c, r = K.pooled_cov(job), K.pooled_cor(job)
    assert c.shape == (3, 3) and np.array_equal(c, c.T) and np.allclose(np.diag(r), 1.0, rtol=1e-15) and np.all(np.abs(r) <= 1.0 + 1e-15)
    job.close()


_CANARY = r'''
import sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import klara_jl_amd as K
from klara_jl_amd import _lib as L
for D, N in ((100, 257), (256, 70), (3, 5)):
    e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=64, burnin=10, thinning=3, driftstep=0.05, monitor=L.MON_COVARIANCE)
    e.init_state_normal(); e.run(64)
    mean, M, ns, nc = e.pooled_covariance()
    assert ns == 18 * N and np.all(np.isfinite(M)) and np.all(np.diag(M) > 0.0)
    e.close()                                                 # klara_destroy: KLARA_OK only with every canary intact
print("INTACT")
'''


def test_job_between_canaries():
    """every device array of a job with the bit between canaries (KLARA_DEBUG_CANARY=1, a child process as tests/test_gpu_canary.py runs its own):
    klara_destroy returns KLARA_OK, so no kernel of the monitor wrote outside its arrays — at a ragged last slab, at three tile groups, at D < 16"""
    env = dict(os.environ, KLARA_DEBUG_CANARY="1")
    r = subprocess.run([sys.executable, "-c", _CANARY.replace("ROOT", str(ROOT))], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("INTACT"), r.stdout
