"""The across-chain reductions (klara_monitors.hip: k_pool_stage1 / k_pool_stage2, k_moments_stage1 / k_moments_stage2 with chan_merge; klara_comm.hip:
k_scale / k_merge_between) against tests/pooled_ref.py: bit for bit against the NumPy restatement of their order of operations (mirror, mirror_ranks)
and, so that the mirror is never the only yardstick, against exact rational arithmetic within the derived bound.  The kernels run on synthetic per-chain
sums through klara_selftest_pooled (the launch functions of the job path; klara_gather_moments' own between-rank sequence, merge_ranks, over simulated
ranks with only the all-reduces swapped for ordered host sums, which is what lets mean_r - mean differ from zero on one GPU), and in small jobs through the API.  The inputs are those tests/test_pooled_host.py checks on the CPU."""
import ctypes as C

import numpy as np
import pytest

import klara_jl_amd as K
import pooled_ref as R
from klara_jl_amd import _lib as L
from test_pooled_host import CHAINS, DIMS, N_WIDE, NS_WIDE, case, errors

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

SENTINEL = -12345.5


def selftest(inp, bounds=None, with_sums=True, status=False, N=None, D=None, nsaved=None, **arrays):
    """klara_selftest_pooled on pooled_ref inputs: dict of its outputs (status=True: the status alone).  The sum slots are handed in holding SENTINEL.
    N, D, nsaved and single arrays can be overridden for the argument checks."""
    klib = L.load()
    a = {k: inp[k] for k in ("sum", "sumsq", "X", "held", "naccept")}
    a.update(arrays)
    N = inp["sum"].shape[0] if N is None else N
    D = inp["sum"].shape[1] if D is None else D
    nsaved = inp["nsaved"] if nsaved is None else nsaved
    b = np.asarray([0, N] if bounds is None else bounds, dtype=np.int64)
    out = {k: np.full(D if 1 <= D <= 1024 else 1, SENTINEL) for k in ("sum", "sumsq", "mean", "m2", "ranks_mean", "ranks_m2")}
    acc, cnt = C.c_uint64(0), np.zeros(3, dtype=np.uint64)
    ptr = lambda v: None if v is None else v.ctypes.data
    st = klib.klara_selftest_pooled(0, N, D, nsaved, ptr(a["sum"]), ptr(a["sumsq"]), ptr(a["X"]), ptr(a["held"]), ptr(a["naccept"]), b.size - 1, ptr(b),
                                    int(with_sums), ptr(out["sum"]), ptr(out["sumsq"]), C.addressof(acc), ptr(out["mean"]), ptr(out["m2"]),
                                    ptr(out["ranks_mean"]), ptr(out["ranks_m2"]), ptr(cnt))
    if status:
        return st
    L.check(st, "klara_selftest_pooled")
    out["accept"] = int(acc.value); out["counters"] = tuple(int(v) for v in cnt)
    return out


def check_case(inp, ex, what, bounds=None):
    """one selftest run against the mirror (bits) and against exact (bound); prints its figures first"""
    N = inp["sum"].shape[0]
    bounds = [0, N] if bounds is None else bounds
    out = selftest(inp, bounds)
    ms, mq, macc = R.mirror_summaries(inp)
    mean, m2 = R.mirror(inp)
    rmean, rm2, rcnt = R.mirror_ranks(inp, bounds)
    e, bm2, em, bmean = errors(out["mean"], out["m2"], ex, N)
    re, rbm2, rem, rbmean = errors(out["ranks_mean"], out["ranks_m2"], ex, N, ranks=len(bounds) - 1)
    bits = {k: int(np.sum(a.view(np.uint64) != b.view(np.uint64))) for k, (a, b) in
            {"sum": (out["sum"], ms), "sumsq": (out["sumsq"], mq), "mean": (out["mean"], mean), "m2": (out["m2"], m2),
             "ranks_mean": (out["ranks_mean"], rmean), "ranks_m2": (out["ranks_m2"], rm2)}.items()}
    print(f"pooled {what}: values differing from the mirror {bits}; M2 error {e.max():.3g} (bound {bm2.max():.3g}), mean error {em.max():.3g} "
          f"(bound {bmean.max():.3g}); ranks M2 error {re.max():.3g}, mean error {rem.max():.3g}")
    assert not any(bits.values()), (what, bits)
    assert out["accept"] == macc == ex["accept"] and out["counters"] == rcnt == (ex["accept"], inp["nsaved"] * N, N)
    assert np.all(e <= bm2) and np.all(em <= bmean) and np.all(re <= rbm2) and np.all(rem <= rbmean), what
    cols = ex["cols"]
    depth = 8 * R.merge_depth(N) * R.U              # (plain sums of at most merge_depth additions per path: loose on purpose, the mirror is the sharp check)
    assert np.all(np.abs(out["sum"][cols] - ex["S"]) <= depth * np.abs(ex["S"])) and np.all(np.abs(out["sumsq"][cols] - ex["Q"]) <= depth * ex["Q"])
    return out


@pytest.mark.parametrize("N", CHAINS)
def test_selftest_every_chain_count(N):
    """D = 3, 200 saved steps, N over the grid edges: fewer chains than blocks (1, 2, 3), than threads of stage 2 (255), exactly and just above 256 and
    1,024, just above 2 x 1,024, three trips and a ragged last one (3,077).  Cut into two shards (one: N = 1) for the between-rank arithmetic."""
    inp, ex = case(N, 3, 200, 0.0)
    check_case(inp, ex, f"N={N}", R.splits(N)["2"] if N > 1 else None)


@pytest.mark.parametrize("D", DIMS)
def test_selftest_every_width(D):
    """N = 1,025, D over the edges of the j += 256 loops of k_moments_stage1 (D) and k_pool_stage1 (2 D), up to the library's 1,024; 8 saved steps keep
    the inputs small; exact on at most eight columns, the mirror on all of them."""
    inp, ex = case(N_WIDE, D, NS_WIDE, 0.0)
    check_case(inp, ex, f"D={D}", [0, 1, N_WIDE])


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_selftest_offsets(offset):
    """N = 1,025, D = 3 at 0, 242, 1e4 and 1e6 sd: the bound grows with |mean| / sd (the mean's rounding carried into delta^2), the bits stay the
    mirror's; up to 242 sd the 1e-12 of the rats test."""
    inp, ex = case(1025, 3, 200, offset)
    out = check_case(inp, ex, f"offset={offset:g}sd", R.splits(1025)["3"])
    if offset <= 242.0:
        assert np.all(np.abs(out["m2"] - ex["M2"]) <= 1e-12 * ex["M2"]) and np.all(np.abs(out["ranks_m2"] - ex["M2"]) <= 1e-12 * ex["M2"])


@pytest.mark.parametrize("nsaved", [0, 1, 2, 200])
def test_selftest_saved_steps(nsaved):
    """nsaved = 0: every division is 0 / 0 and only chan_merge's guard keeps NaN out — zeros; 1: at the clamp (q - s^2 is a square's rounding error,
    either sign; the expected value is the mirror's); 2; 200."""
    for N in (3, 1025):
        if nsaved == 1:
            inp = R.clamp_inputs(N, 3, 242.0)
            ex = R.exact(inp)
        else:
            inp, ex = case(N, 3, nsaved, 242.0)
        out = check_case(inp, ex, f"nsaved={nsaved} N={N}", R.splits(N)["3"])
        if nsaved == 0:
            for k in ("mean", "m2", "ranks_mean", "ranks_m2"):
                assert np.all(out[k] == 0.0), k


@pytest.mark.parametrize("name", list(R.splits(2051)))
def test_selftest_ranks(name):
    """2,051 chains over 1, 2, 3 and 5 simulated ranks as shard_chains cuts them, and unequal shards (1 | N - 1, N - 1 | 1, 1 | 1 | N - 2, 1025 | rest),
    at 1e4 sd: n_r (mean_r - mean)^2 is far from zero, so a wrong weight in k_scale or k_merge_between, or a wrong offset, count or counter slot in merge_ranks, changes the result."""
    inp, ex = case(2051, 3, 200, 1e4)
    b = R.splits(2051)[name]
    out = check_case(inp, ex, f"ranks {name}", b)
    if len(b) > 2:
        mean_r = [R.mirror(R.slice_inputs(inp, c0, c1))[0] for c0, c1 in zip(b[:-1], b[1:])]
        between = sum(200.0 * (c1 - c0) * (m - out["ranks_mean"]) ** 2 for m, c0, c1 in zip(mean_r, b[:-1], b[1:]))
        print(f"pooled ranks {name}: between-rank term / (bound x M2) {(between / (R.bound(2051, ex, len(b) - 1)[0] * ex['M2'])).min():.3g}")
        assert np.all(between > 10.0 * R.bound(2051, ex, len(b) - 1)[0] * ex["M2"])           # the between-rank term is well above the bound


def test_selftest_accept_total_and_untouched_sum_slots():
    """The accept total is the exact integer sum of counters near 2^40 (above 2^32 in all); without sums the sum slots come back as they went in."""
    inp, ex = case(1025, 3, 200, 0.0)
    assert ex["accept"] > 2 ** 40 and int(inp["naccept"].max()) > 2 ** 39
    out = selftest(inp, with_sums=False)
    assert out["accept"] == ex["accept"]
    assert np.all(out["sum"] == SENTINEL) and np.all(out["sumsq"] == SENTINEL)
    mean, m2 = R.mirror(inp)
    assert np.array_equal(out["mean"], mean) and np.array_equal(out["m2"], m2)
    out = selftest(inp, with_sums=True)
    assert not np.any(out["sum"] == SENTINEL) and out["accept"] == ex["accept"]


def test_selftest_refuses_bad_arguments():
    inp, _ = case(3, 3, 200, 0.0)
    for bounds in ([0, 2], [1, 3], [0, 2, 2, 3], [0, 2, 1, 3], [0, 4]):
        assert selftest(inp, bounds, status=True) == L.ERR_INVALID_ARG, bounds
    assert selftest(inp, status=True, D=0) == L.ERR_INVALID_ARG and selftest(inp, status=True, D=1025) == L.ERR_INVALID_ARG
    assert selftest(inp, status=True, N=0) == L.ERR_INVALID_ARG and selftest(inp, status=True, nsaved=-1) == L.ERR_INVALID_ARG
    for k in ("sum", "sumsq", "X", "held", "naccept"):
        assert selftest(inp, status=True, **{k: None}) == L.ERR_INVALID_ARG, k
    assert selftest(inp, status=True) == L.OK


# ---------------------------------------------------------------- jobs
JOB_MU, JOB_SIGMA = np.array([0.0, 242.0, -1e4]) * np.array([1.0, 0.5, 2.0]), np.array([1.0, 0.5, 2.0])


def _job(N, nsteps=60, burnin=20, run=None):
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.mvnormal(JOB_MU, JOB_SIGMA), nchains=N, nsteps=nsteps, burnin=burnin, driftstep=0.4,
                   monitor=L.MON_SUMMARIES, seed=20261019, steps_per_launch=7)
    eng.set_state(JOB_MU + JOB_SIGMA * np.random.default_rng(3).standard_normal((N, 3)))
    eng.run(nsteps if run is None else run)
    return eng


def _job_inputs(eng):
    s, q, nsaved = eng.chain_sums()
    acc, _ = eng.accept_counts()
    return {"sum": s, "sumsq": q, "X": eng.state()[0], "held": np.zeros(eng.nchains, dtype=np.int64), "naccept": acc, "nsaved": nsaved}


@pytest.mark.parametrize("N", [1, 3, 300, 1025])
def test_job_pooled_results_are_the_mirror_of_the_chain_sums(N):
    """MALA on a diagonal Gaussian (D = 3, means at 0, 242 and -1e4 sd), 40 saved steps: Engine.pooled_moments() and pooled_summaries() bit for bit
    against the mirror.  The handle's held counts cannot be read through the API, so the mirror is fed chain_sums() — the device's own part + held x,
    the same two operations the pooling kernels apply — with held = 0."""
    eng = _job(N)
    inp = _job_inputs(eng)
    assert inp["nsaved"] == 40
    mean, m2, ns, na, nt, nc = eng.pooled_moments()
    s, q, pna, pnt, pns = eng.pooled_summaries()
    wm, wq = R.mirror(inp)
    ws, wsq, wacc = R.mirror_summaries(inp)
    assert np.array_equal(mean, wm) and np.array_equal(m2, wq) and np.array_equal(s, ws) and np.array_equal(q, wsq)
    assert (ns, na, nt, nc) == (40 * N, wacc, 60 * N, N) and (pna, pnt, pns) == (wacc, 60 * N, 40)
    ex = R.exact(inp)
    e, bm2, em, bmean = errors(mean, m2, ex, N)
    print(f"pooled job N={N}: M2 error {e.max():.3g} (bound {bm2.max():.3g}), mean error {em.max():.3g} (bound {bmean.max():.3g})")
    assert np.all(e <= bm2) and np.all(em <= bmean)
    eng.close()


def test_job_without_a_saved_step():
    """No saved step yet: means and M2 are zeros, the counters are right, nothing is NaN — through the API and through the selftest's rank path on the
    same sums.  (klara_create refuses nsteps == burnin, so the job is read after its `burnin` transitions: the same state of the handle.)"""
    eng = _job(300, run=20)
    inp = _job_inputs(eng)
    assert inp["nsaved"] == 0
    mean, m2, ns, na, nt, nc = eng.pooled_moments()
    assert np.all(mean == 0.0) and np.all(m2 == 0.0)
    assert (ns, na, nt, nc) == (0, int(inp["naccept"].sum()), 20 * 300, 300) and na > 0
    s, q, pna, pnt, pns = eng.pooled_summaries()
    assert np.all(s == 0.0) and np.all(q == 0.0) and (pna, pnt, pns) == (na, nt, 0)
    out = selftest(inp, [0, 100, 300])
    assert np.all(out["ranks_mean"] == 0.0) and np.all(out["ranks_m2"] == 0.0) and out["counters"] == (na, 0, 300)
    eng.close()


def test_job_one_rank_communicator_is_bit_identical(klib):
    """klara_gather_moments through a one-rank RCCL communicator at N = 300: bit for bit the between-rank arithmetic of one rank (mean = (n mean_r) / n,
    M2_r + n (mean_r - mean)^2: mirror_ranks with one shard), and bit for bit the result without a communicator."""
    eng = _job(300)
    inp = _job_inputs(eng)
    mean, m2, ns, na, nt, nc = eng.pooled_moments()
    wm, wq, cnt = R.mirror_ranks(inp, [0, 300])
    uid = (C.c_uint8 * 128)()
    L.check(klib.klara_comm_unique_id(uid), "comm_unique_id")
    comm = C.c_void_p()
    L.check(klib.klara_comm_init(C.byref(comm), 1, 0, uid, 0), "comm_init")
    try:
        cmean, cm2, cns, cna, cnt_, cnc = eng.pooled_moments(comm)
    finally:
        L.check(klib.klara_comm_destroy(comm), "comm_destroy")
    assert (cns, cna, cnt_, cnc) == (ns, na, nt, nc)
    assert np.array_equal(cmean, wm) and np.array_equal(cm2, wq)
    assert np.array_equal(cmean, mean) and np.array_equal(cm2, m2)
    eng.close()
