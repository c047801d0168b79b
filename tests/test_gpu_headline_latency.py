"""GPU tests (-m gpu) of the table kernels' early-issued reads (klara.jl_amd/csrc/klara_diagt.h pair_issue / pair_finish, detmath.h
kd_normal_pair_issue / kd_normal_pair_finish).

The two MALA kernels of the D = 100 job that read Box-Muller's remainder terms from an LDS table (13 pairs per lane on 4 lanes, 7 on 8) now start
the three table reads of pair p + 1 before they work on pair p, read the launch constants (the Philox key, the save rule's bounds) once before the
step loop instead of at every use, and start their partial sums from the first term instead of adding it to zero.  None of that may move a bit:
small jobs on every path of those kernels against the oracle, which draws a pair in one piece and sums from zero — values, log-targets, gradients,
accept masks and counts and the running sums bit for bit (the comparison of tests/test_gpu_sincos_table.py).

D: 100, 99 (the last pair is half a pair), 104 (no padding pair on 4 lanes: the accept draw forms its own block), 97 — all 13 pairs per lane.
chains: 1, 81, 97, 197 — 1, 6, 7 and 13 wavefronts of the 4-lane kernel: a partial last wavefront, and workgroups whose last wavefronts have no
chains and must still fill their share of the table and reach the barrier, whatever the workgroup size.
sparse_moves: 0 the device decides launch by launch, 1 the 4-lane kernels, 2 the 8-lane kernels.  driftstep 0.9 / 0.3: at 0.3 the commit / fold
path runs on about half the transitions.  40 transitions are launches of 32 and 8, both on the table kernels; 39 are 32 and 7: the second launch
runs the arithmetic kernel (a pair in one piece, 256 threads) on the state and the sums the first one left.  Every job with one stream and with
the default two chain partitions."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

SUMS = L.MON_ACCEPT | L.MON_SUMMARIES
GROUPS = [(d, n, ns) for d in (100, 99, 104, 97) for n in (1, 81, 97, 197) for ns in (1, 0)]
INNER = [(h, sm, steps) for h in (0.9, 0.3) for sm in (0, 1, 2) for steps in (40, 39)]


@pytest.mark.parametrize("d,nchains,nstreams", GROUPS, ids=[f"d{d}_n{n}_{'one_stream' if ns else 'partitions'}" for d, n, ns in GROUPS])
def test_early_issue_kernels_bit_for_bit_against_the_oracle(d, nchains, nstreams):
    moved = {}
    for h, sparse, nsteps in INNER:
        moved[(h, sparse, nsteps)] = _job_against_the_oracle(d, h, sparse, nchains, nsteps, nstreams)
    # both the commit and the reject path ran in every job with enough chains for that to be certain (a lone chain at driftstep 0.9 accepts
    # a few per cent of 40 proposals: it may well accept none, and is compared all the same)
    if nchains >= 81:
        for key, (acc, size) in moved.items():
            assert 0 < acc < size, f"d{d} n{nchains} {key}: accepted {acc} of {size}"


def _job_against_the_oracle(d, h, sparse, nchains, nsteps, nstreams):
    name = f"mala_d{d}_h{h}_{sparse}_{nchains}_{nsteps}_{nstreams}"
    kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(d), driftstep=h)
    if sparse:
        kw["sparse_moves"] = sparse
    case = dict(burnin=0, **kw, nchains=nchains, nsteps=nsteps, x0=None, seed=20261019, name=name)
    over = dict(nstreams=nstreams) if nstreams else {}
    eng = K.Engine(**cases.engine_kwargs(case, monitor=SUMS, **over))
    layout = eng.layout()
    assert layout[:2] == (3, 8), layout
    job = O.OracleJob(**cases.oracle_kwargs(case, layout=layout))
    eng.init_state_normal(); assert job.init_state_normal() == 0
    eng.run(nsteps); assert job.run(nsteps) == 0
    cnt = [int(c) for c in eng.launch_modes()[0]]              # launches on the 4-lane kernel alone, the 8-lane kernel alone, the device-decided pair
    assert sum(cnt) == 2 and (sparse != 1 or cnt[0] == 2) and (sparse != 2 or cnt[0] == 0), (name, cnt)    # the forced kernel family ran both launches
    mask = eng.accept_mask()
    assert np.array_equal(mask, job.accept), f"{name}: accept mask differs at {np.argwhere(mask != job.accept)[:5]}"
    x, lt, g = eng.state()
    assert np.array_equal(x.view(np.uint64), job.X.view(np.uint64)), f"{name}: values differ"
    assert np.array_equal(lt.view(np.uint64), job.LT.view(np.uint64)), f"{name}: log-target differs"
    assert np.array_equal(g.view(np.uint64), job.G.view(np.uint64)), f"{name}: gradient differs"
    na, nst = eng.accept_counts()
    assert np.array_equal(na, job.naccept) and nst == nsteps, f"{name}: accept counts differ"
    s, q, nsaved = eng.chain_sums()
    assert nsaved == nsteps
    assert np.array_equal(s.view(np.uint64), job.sum.view(np.uint64)), f"{name}: running sums differ"
    assert np.array_equal(q.view(np.uint64), job.sumsq.view(np.uint64)), f"{name}: running sums of squares differ"
    eng.close()
    return int(mask.sum()), int(mask.size)
