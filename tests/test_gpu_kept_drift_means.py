"""GPU tests (-m gpu) of the table kernels' step-loop residents and kept drift means (klara.jl_amd/csrc/klara_diagt.h KLARA_LC, late_ctx,
diagt_kept_means / `dm` in k_diagt).

The MALA kernels of the D = 100 job that read Box-Muller's remainder terms from an LDS table (13 pairs per lane on 4 lanes, 7 on 8) hold MALA's
0.5 / h and the accept-draw flag in scalar registers and count the save range in the launch's own steps; the 4-lane kernel re-forms a lane's
chain and pair offsets from the lane number in its rare branches and behind the loop.  Both can also keep the mean of the proposal density,
x + (-h) x, over rejected transitions — formed once per chain group after the state is loaded, read in every transition, re-formed from the
accepted proposal in the commit — for as many of a lane's elements as KLARA_Q4_KEPT_MEANS / KLARA_Q8_KEPT_MEANS say: none by default (the means
need the registers of a two-wavefront budget, KLARA_Q4_SCTAB_WF), and these are the jobs a build that keeps them is held to.
A kept mean that goes stale — not refreshed by an accept, refreshed for the wrong chain of a wavefront, not re-formed at a launch boundary — or a
save range, chain or offset that is off by one moves bits, so small jobs are held to the oracle bit for bit: values, log-targets, gradients,
accept masks and counts, running sums — the comparison of tests/test_gpu_headline_latency.py.

D: 100, 99 (the last pair is half a pair), 104 (no padding pair on 4 lanes), 97 — all 13 pairs per lane on 4 lanes and 7 on 8.
chains: 81 and 197 — partial last wavefronts on both kernels.  sparse_moves: 0 the device decides launch by launch, 1 the 4-lane kernels, 2 the 8-lane.
driftstep 0.9: a state is almost never left; 0.3: on about every second transition; 0.02: nearly every transition accepts, the commit runs again
and again within one launch (accepted share above 0.9, asserted per job).
72 transitions are launches of 32, 32 and 8, all on the table kernels: everything kept over a launch is re-formed from the loaded state at each
launch boundary; 71 are 32, 32 and 7: the last launch runs the arithmetic kernel on what the table kernels left.
Every job with one stream and with the default two chain partitions.
The history jobs add a value history monitor, a burn-in and thinning 3: the stores of the committed x use the late-formed offsets, and the table
kernels count the save range in the launch's own steps — burn-in 5 ends inside the first launch, 37 inside the second, 64 together with the second."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

SUMS = L.MON_ACCEPT | L.MON_SUMMARIES
GROUPS = [(d, n, ns) for d in (100, 99, 104, 97) for n in (81, 197) for ns in (1, 0)]
INNER = [(h, sm, steps) for h in (0.9, 0.3, 0.02) for sm in (0, 1, 2) for steps in (72, 71)]


@pytest.mark.parametrize("d,nchains,nstreams", GROUPS, ids=[f"d{d}_n{n}_{'one_stream' if ns else 'partitions'}" for d, n, ns in GROUPS])
def test_table_kernels_bit_for_bit_against_the_oracle(d, nchains, nstreams):
    for h, sparse, nsteps in INNER:
        acc, size = _job_against_the_oracle(d, h, sparse, nchains, nsteps, nstreams)
        print(f"d{d} n{nchains} streams {nstreams} h{h} sparse {sparse} steps {nsteps}: accepted {acc} of {size} ({acc / size:.4f})")
        if h == 0.02:           # the commit runs on nearly every transition
            assert acc > 0.9 * size, f"d{d} n{nchains} h{h} sparse {sparse} steps {nsteps}: accepted {acc} of {size}"
        if h == 0.9:            # both the commit and the reject path ran (81 chains or more: certain)
            assert 0 < acc < size, f"d{d} n{nchains} h{h} sparse {sparse} steps {nsteps}: accepted {acc} of {size}"


@pytest.mark.parametrize("sparse", [0, 1, 2])
@pytest.mark.parametrize("burnin", [5, 37, 64])
def test_table_kernels_history_stores_and_save_range(sparse, burnin):
    acc, size = _job_against_the_oracle(99, 0.3, sparse, 81, 72, 1, monitor=SUMS | L.MON_HISTORY, burnin=burnin, thinning=3)
    assert 0 < acc < size


def _job_against_the_oracle(d, h, sparse, nchains, nsteps, nstreams, monitor=SUMS, burnin=0, thinning=1):
    name = f"mala_d{d}_h{h}_{sparse}_{nchains}_{nsteps}_{nstreams}_{burnin}_{thinning}"
    kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(d), driftstep=h)
    if sparse:
        kw["sparse_moves"] = sparse
    case = dict(burnin=burnin, thinning=thinning, **kw, nchains=nchains, nsteps=nsteps, x0=None, seed=20261020, name=name)
    over = dict(nstreams=nstreams) if nstreams else {}
    eng = K.Engine(**cases.engine_kwargs(case, monitor=monitor, **over))
    layout = eng.layout()
    assert layout[:2] == (3, 8), layout
    hist = bool(monitor & L.MON_HISTORY)
    job = O.OracleJob(**cases.oracle_kwargs(case, layout=layout), want_hist=hist)
    eng.init_state_normal(); assert job.init_state_normal() == 0
    eng.run(nsteps); assert job.run(nsteps) == 0
    cnt = [int(c) for c in eng.launch_modes()[0]]              # launches on the 4-lane kernel alone, the 8-lane kernel alone, the device-decided pair
    assert sum(cnt) == 3 and (sparse != 1 or cnt[0] == 3) and (sparse != 2 or cnt[0] == 0), (name, cnt)    # the forced kernel family ran every launch
    mask = eng.accept_mask()
    assert np.array_equal(mask, job.accept), f"{name}: accept mask differs at {np.argwhere(mask != job.accept)[:5]}"
    x, lt, g = eng.state()
    assert np.array_equal(x.view(np.uint64), job.X.view(np.uint64)), f"{name}: values differ"
    assert np.array_equal(lt.view(np.uint64), job.LT.view(np.uint64)), f"{name}: log-target differs"
    assert np.array_equal(g.view(np.uint64), job.G.view(np.uint64)), f"{name}: gradient differs"
    na, nst = eng.accept_counts()
    assert np.array_equal(na, job.naccept) and nst == nsteps, f"{name}: accept counts differ"
    s, q, nsaved = eng.chain_sums()
    assert nsaved == len(range(burnin + 1, nsteps + 1, thinning))
    assert np.array_equal(s.view(np.uint64), job.sum.view(np.uint64)), f"{name}: running sums differ"
    assert np.array_equal(q.view(np.uint64), job.sumsq.view(np.uint64)), f"{name}: running sums of squares differ"
    if hist:
        for c in range(nchains):
            v = np.ascontiguousarray(eng.chain(c))
            assert v.shape == (d, nsaved), (name, c, v.shape)
            assert np.array_equal(v.view(np.uint64), np.ascontiguousarray(job.hist[:, c, :].T).view(np.uint64)), f"{name}: value history of chain {c} differs"
    eng.close()
    return int(mask.sum()), int(mask.size)
