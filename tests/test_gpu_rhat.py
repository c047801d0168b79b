"""The Gelman–Rubin diagnostic on the device (klara_rhat.hip: k_rhat_stage1 / k_rhat_stage2 over the chains' running sums, k_rhat_halves over the stored
history; klara_comm.hip: the between-rank merge of klara_merge.h with chains where the samples stand) against tests/rhat_ref.py: bit for bit against the
NumPy restatement of the order of operations and, so that the mirror is never the only yardstick, against exact rational arithmetic within the derived
bound.  The kernels run on synthetic inputs through klara_selftest_rhat (the launch functions of the job path; klara_gather_rhat's own between-rank
sequence over simulated ranks with only the all-reduces swapped for ordered host sums) and in a small job through the API.  The inputs are those
tests/test_rhat_host.py checks on the CPU."""
import ctypes as C
import multiprocessing as mp
import os

import numpy as np
import pytest

import klara_jl_amd as K
import pooled_ref as P
import rhat_ref as R
from klara_jl_amd import _lib as L
from test_rhat_host import hist_case, hist_shapes, selftest, sums_case, sums_shapes

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]


@pytest.mark.parametrize("N", R.NS)
def test_sums_path_is_the_mirror_and_within_the_bound_of_exact(N):
    """N: m < 2, the 256-thread tree's edges, nb = min(N, 1024), blocks with unequal chain counts; D = 257 across the 256-thread stride; nsaved 1 (n < 2:
    NaN), 2, 3, 200; offsets 0, 242 and 1e6 sd; chains that never moved among them (pooled_ref.make_inputs); every shard cut of rhat_ref.rank_bounds"""
    worst = 0.0
    for D, ns, off in sums_shapes(N):
        inp, ex = sums_case(N, D, ns, off)
        mir = R.mirror(inp=inp)
        for r, b in R.rank_bounds(N).items():
            what = f"sums N={N} D={D} nsaved={ns} offset={off} ranks={r}"
            out = selftest(inp=inp, bounds=b)
            worst = max(worst, R.check(out["out"], mir, ex, 1, what), R.check(out["ranks"], R.mirror_ranks(b, inp=inp), ex, r, what))
            if ns < 2 or N < 2:
                assert np.all(np.isnan(out["out"]["rhat"])) and np.all(np.isnan(out["ranks"]["rhat"])), what
    print(f"rhat device, sums, N={N}: largest error / bound {worst:.3g}")


@pytest.mark.parametrize("N", R.NS)
def test_split_path_is_the_mirror_and_within_the_bound_of_exact(N):
    """ncols 3 (h = 1: NaN), 4, 5 and 7 (the middle sample dropped), 200; chains that never moved and chains still through their first half among them"""
    worst = 0.0
    for D, nc, off in hist_shapes(N):
        h, ex = hist_case(N, D, nc, off)
        mir = R.mirror(hist=h)
        for r, b in R.rank_bounds(N).items():
            what = f"split N={N} D={D} ncols={nc} offset={off} ranks={r}"
            out = selftest(hist=h, bounds=b)
            worst = max(worst, R.check(out["split"], mir, ex, 1, what), R.check(out["split_ranks"], R.mirror_ranks(b, hist=h), ex, r, what))
            if nc < 4:
                assert np.all(np.isnan(out["split"]["rhat"])) and np.all(np.isnan(out["split_ranks"]["rhat"])), what
    print(f"rhat device, split, N={N}: largest error / bound {worst:.3g}")


def test_still_chains_give_zero_inf_and_nan_exactly():
    """All chains still: wsum exactly 0, R-hat +inf where their states differ, NaN where all stand at one state; both paths, all chains and shards"""
    b = [0, 1, 100, 257]
    for off in R.OFFSETS:
        for same in (False, True):
            inp = R.still_inputs(257, 3, 200, off, same=same)
            h = R.make_hist(257, 3, 200, off, still="same" if same else "all")
            out = selftest(inp=inp, hist=h, bounds=b)
            exs, exh = R.exact(inp=inp), R.exact(hist=h)
            R.check(out["out"], R.mirror(inp=inp), exs, 1, "still sums"); R.check(out["ranks"], R.mirror_ranks(b, inp=inp), exs, 3, "still sums ranks")
            R.check(out["split"], R.mirror(hist=h), exh, 1, "still split"); R.check(out["split_ranks"], R.mirror_ranks(b, hist=h), exh, 3, "still split ranks")
            for k in ("out", "ranks", "split", "split_ranks"):
                assert np.all(out[k]["wsum"] == 0.0)
                assert np.all(np.isnan(out[k]["rhat"])) if same else np.all(out[k]["rhat"] == np.inf), (k, same, out[k]["rhat"])


# ---------------------------------------------------------------- a small job
JOB_MU = np.array([0.0, 242.0 * 1.5, -1e4 * 0.5])
JOB_SIGMA = np.array([1.0, 1.5, 0.5])
NJOB, NSTEPS, BURNIN = 512, 84, 20


def _job(N=NJOB, run=NSTEPS, monitor=L.MON_SUMMARIES | L.MON_HISTORY, offset=0, device=0, **kw):
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.mvnormal(JOB_MU, JOB_SIGMA), nchains=N, nsteps=NSTEPS + 16, burnin=BURNIN, driftstep=0.4,
                   monitor=monitor, seed=20261019, steps_per_launch=7, chain_offset=offset, device=device, **kw)
    eng.set_state((JOB_MU + JOB_SIGMA * np.random.default_rng(3).standard_normal((NJOB, 3)))[offset:offset + N])
    eng.run(run)
    return eng


def _job_inputs(eng):
    s, q, nsaved = eng.chain_sums()
    return {"sum": s, "sumsq": q, "X": eng.state()[0], "held": np.zeros(eng.nchains, dtype=np.int64), "naccept": eng.accept_counts()[0], "nsaved": nsaved}


def _job_hist(eng):
    return np.ascontiguousarray(np.stack([eng.chain(c).T for c in range(eng.nchains)], axis=1))      # (saved steps, chains, D)


def test_job_rhat_is_the_mirror_of_its_sums_and_of_its_history():
    """MALA, D = 3, 512 chains, 64 saved steps, running sums and history: Engine.rhat() is the mirror of chain_sums(), Engine.rhat(split=True) the mirror of
    the histories read back, bit for bit; wsum + nper bsum is pooled_moments()'s M2 within the sum of the two derived bounds; K.stats.rhat agrees."""
    eng = _job()
    inp, h = _job_inputs(eng), _job_hist(eng)
    assert inp["nsaved"] == 64 and h.shape == (64, NJOB, 3)
    got, gots = eng.rhat(), eng.rhat(split=True)
    mir, mirs = R.mirror(inp=inp), R.mirror(hist=h)
    for k in ("rhat", "mean", "wsum", "bsum", "nchains", "nper"):
        assert np.array_equal(got[k], mir[k]), (k, got[k], mir[k])
        assert np.array_equal(gots[k], mirs[k]), (k, gots[k], mirs[k])
    assert (got["nchains"], got["nper"], gots["nchains"], gots["nper"]) == (NJOB, 64, 2 * NJOB, 32)
    assert np.all(got["rhat"] > 0.99) and np.all(gots["rhat"] > 0.98) and np.all(np.isfinite(got["rhat"])) and np.all(np.isfinite(gots["rhat"]))
    v = h.transpose(1, 0, 2)
    assert np.allclose(got["rhat"], K.stats.rhat(v), rtol=1e-6) and np.allclose(gots["rhat"], K.stats.rhat(v, split=True), rtol=1e-6)
    # the decomposition against the total the pooled moments return
    ex = R.exact(inp=inp)
    rel_w, rel_b, _ = R.bound(ex)
    pex = P.exact(inp)
    rel_p, _ = P.bound(NJOB, pex)
    _, m2, ns, _, _, _ = eng.pooled_moments()
    total = got["wsum"] + got["nper"] * got["bsum"]
    tol = rel_w * got["wsum"] + rel_b * got["nper"] * got["bsum"] + rel_p * m2 + 4 * R.U * m2
    print(f"rhat job: |wsum + n bsum - M2| / M2 {np.abs(total - m2) / m2}, tolerance / M2 {tol / m2}")
    assert ns == 64 * NJOB and np.all(np.abs(total - m2) <= tol), (total, m2, tol)
    assert np.array_equal(eng.rhat()["rhat"], got["rhat"]) and np.array_equal(eng.rhat(split=True)["bsum"], gots["bsum"])      # the same bits again
    eng.close()


def test_job_goes_on_as_if_rhat_had_never_been_called():
    a, b = _job(run=50), _job(run=50)
    a.rhat(); a.rhat(split=True)
    a.run(NSTEPS + 16 - 50); b.run(NSTEPS + 16 - 50)
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    sa, sb = a.chain_sums(), b.chain_sums()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]
    assert np.array_equal(a.chain(17), b.chain(17)) and np.array_equal(a.accept_counts()[0], b.accept_counts()[0])
    a.close(); b.close()


def test_job_states_that_are_refused_or_empty(klib):
    """Before the first saved sample: NaN, zeros, KLARA_OK.  Split needs the whole history: a ring, no history at all or fewer than 4 saved steps are
    KLARA_ERR_STATE, as is the unsplit form without running sums."""
    eng = _job(run=BURNIN)
    for split in (False, True):
        out = eng.rhat(split=split)
        assert np.all(np.isnan(out["rhat"])) and all(np.all(out[k] == 0.0) for k in ("mean", "wsum", "bsum")) and (out["nchains"], out["nper"]) == (0, 0)
    eng.run(3)
    assert eng.rhat()["nper"] == 3
    with pytest.raises(L.KlaraError) as e:
        eng.rhat(split=True)
    assert e.value.status == L.ERR_STATE
    eng.run(1)
    assert eng.rhat(split=True)["nper"] == 2
    assert klib.klara_gather_rhat(eng._h, None, 1, None, None, None, None, None, None) == L.OK       # every output may be NULL
    eng.close()
    ring = _job(hist_ring_cols=16)
    assert ring.rhat()["nper"] == 64
    with pytest.raises(L.KlaraError) as e:
        ring.rhat(split=True)
    assert e.value.status == L.ERR_STATE
    ring.close()
    sums_only = _job(monitor=L.MON_SUMMARIES)
    with pytest.raises(L.KlaraError) as e:
        sums_only.rhat(split=True)
    assert e.value.status == L.ERR_STATE
    sums_only.close()
    hist_only = _job(monitor=L.MON_HISTORY)
    with pytest.raises(L.KlaraError) as e:
        hist_only.rhat()
    assert e.value.status == L.ERR_STATE
    assert hist_only.rhat(split=True)["nper"] == 32
    hist_only.close()


def test_job_one_rank_communicator_runs_the_merge(klib):
    """klara_gather_rhat through a one-rank RCCL communicator: bit for bit the between-rank arithmetic of one rank (rhat_ref.mirror_ranks with one shard)
    and what klara_selftest_rhat returns for it, both forms; K.rhat and the distributed wrapper return the same"""
    eng = _job()
    inp, h = _job_inputs(eng), _job_hist(eng)
    uid = (C.c_uint8 * 128)()
    L.check(klib.klara_comm_unique_id(uid), "comm_unique_id")
    comm = C.c_void_p()
    L.check(klib.klara_comm_init(C.byref(comm), 1, 0, uid, 0), "comm_init")
    try:
        got, gots = eng.rhat(comm=comm), eng.rhat(split=True, comm=comm)
    finally:
        L.check(klib.klara_comm_destroy(comm), "comm_destroy")
    st = selftest(inp=inp, hist=h, bounds=[0, NJOB])
    for k in ("rhat", "mean", "wsum", "bsum", "nchains", "nper"):
        assert np.array_equal(got[k], R.mirror_ranks([0, NJOB], inp=inp)[k]) and np.array_equal(got[k], st["ranks"][k]), k
        assert np.array_equal(gots[k], R.mirror_ranks([0, NJOB], hist=h)[k]) and np.array_equal(gots[k], st["split_ranks"][k]), k
    eng.close()


# ---------------------------------------------------------------- several GPUs
def _rank_main(rank, world, uid_q, out_q, uneven):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import klara_jl_amd as K2
    from klara_jl_amd import _lib as L2
    import test_gpu_rhat as T
    lib = L2.load()
    try:
        uid = (C.c_uint8 * 128)()
        if rank == 0:
            L2.check(lib.klara_comm_unique_id(uid), "klara_comm_unique_id")
            for _ in range(world - 1):
                uid_q.put(bytes(uid))
        else:
            uid = (C.c_uint8 * 128).from_buffer_copy(uid_q.get(timeout=120))
        offset, n = K2.shard_chains(T.NJOB, rank, world)
        eng = T._job(N=n, run=T.NSTEPS + (rank if uneven else 0), offset=offset, device=rank)
        comm = C.c_void_p()
        L2.check(lib.klara_comm_init(C.byref(comm), world, rank, uid, rank), "klara_comm_init")
        res = []
        for split in (False, True):
            try:
                res.append(eng.rhat(split=split, comm=comm))
            except L2.KlaraError as exc:
                res.append(exc.status)
        out_q.put((rank, offset, n, res, None if uneven else T._job_inputs(eng), None if uneven else T._job_hist(eng), None))
        L2.check(lib.klara_comm_destroy(comm), "klara_comm_destroy")
        eng.close()
    except Exception as exc:        # the parent must not wait for a rank that died
        out_q.put((rank, 0, 0, None, None, None, repr(exc)))


def _run_ranks(world, uneven):
    ctx = mp.get_context("spawn")
    uid_q, out_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, uid_q, out_q, uneven)) for r in range(world)]
    for p in procs:
        p.start()
    results = [out_q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
    errs = [r[-1] for r in results if r[-1] is not None]
    assert not errs, errs
    return sorted(results, key=lambda r: r[0])


def test_gather_rhat_over_a_communicator_is_the_selftest_with_the_same_bounds():
    """One process per GPU, the job sharded by chain_offset: klara_gather_rhat over the communicator against klara_selftest_rhat on the ranks' own sums and
    histories with the same bounds — bit for bit at world size 2, within the bound at 3 or 4, where the collective's order of summation is not ours."""
    import torch
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("needs at least 2 GPUs on the box")
    world = min(ndev, 4)
    results = _run_ranks(world, False)
    bounds = [0] + [r[1] + r[2] for r in results]
    inp = {k: np.concatenate([r[4][k] for r in results]) for k in ("sum", "sumsq", "X", "held", "naccept")}
    inp["nsaved"] = results[0][4]["nsaved"]
    h = np.ascontiguousarray(np.concatenate([r[5] for r in results], axis=1))
    st = selftest(inp=inp, hist=h, bounds=bounds)
    exs, exh = R.exact(inp=inp), R.exact(hist=h)
    for rank, _, _, res, _, _, _ in results:
        for got, want, ex in ((res[0], st["ranks"], exs), (res[1], st["split_ranks"], exh)):
            assert isinstance(got, dict), (rank, got)
            assert (got["nchains"], got["nper"]) == (want["nchains"], want["nper"])
            if world == 2:
                for k in ("rhat", "mean", "wsum", "bsum"):
                    assert np.array_equal(got[k], want[k]), (rank, k)
            R.check(got, None, ex, world, f"rank {rank} of {world}")


def test_unequal_saved_steps_are_refused_on_every_rank():
    """Rank r has saved r steps more than rank 0: every rank returns KLARA_ERR_STATE, from both forms, and none is left waiting in a reduction"""
    import torch
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("needs at least 2 GPUs on the box")
    for rank, _, _, res, _, _, _ in _run_ranks(min(ndev, 4), True):
        assert res == [L.ERR_STATE, L.ERR_STATE], (rank, res)
