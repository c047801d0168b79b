"""GPU tests (-m gpu) of the remainder table of Box-Muller's 20-bit angle (klara.jl_amd/csrc/detmath.h kd_sincos2pi_tab20, klara_diagt.h SCTAB).

The untuned monitored MALA kernels of the D = 100 job on the unit diagonal (13 pairs per lane on 4 lanes, 7 on 8) read sin y and cos y - 1 of the angle's remainder from a
4,096-entry LDS table that every workgroup fills first, instead of forming them per pair; no bit of any result may move
(tests/test_sincos_table_host.py has the arithmetic).  Here: all 2^20 angles through the table on the device against the arithmetic form on the
device and on the host, and small jobs on every path of those kernels against the oracle, which keeps the arithmetic form — values, log-targets,
gradients, accept masks and counts and the running sums bit for bit."""
import numpy as np
import pytest

import cases
import oracle_ffi as O
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

NSTEPS = 40                                   # a launch of 32 transitions and one of 8 (the shortest that takes the table): it is filled twice
SUMS = L.MON_ACCEPT | L.MON_SUMMARIES


def _math(klib, op, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    L.check(klib.klara_selftest_math(0, op, x.size, x.ctypes.data, x.ctypes.data, out.ctypes.data), "selftest_math")
    return out.view(np.uint64)


def test_table_form_on_the_device_at_every_angle(klib):
    """ops 13 / 14 (sin / cos of angle index k through the table, filled in that kernel) against ops 15 / 16 (the arithmetic form of the same
    20-bit angle), ops 2 / 3 (kd_sincos2pi at u = (k + 1/2) 2^-20, which forms the same bits: tests/test_sincos_table_host.py) and the host."""
    k = np.arange(1 << 20, dtype=np.float64)
    u = (k + 0.5) * 2.0 ** -20
    for tab, bits20, dbl in ((13, 15, 2), (14, 16, 3)):
        got = _math(klib, tab, k)
        host = O.math_op(dbl, u, u).view(np.uint64)
        for name, ref in (("device, 20-bit arithmetic form", _math(klib, bits20, k)), ("device, kd_sincos2pi", _math(klib, dbl, u)), ("host", host)):
            bad = np.flatnonzero(got != ref)
            assert bad.size == 0, f"op {tab} against {name}: {bad.size} of {k.size} angles differ, the first at k = {bad[:5]}"


# D: 100 (13 pairs per lane on 4 lanes, 7 on 8), 99 (the last pair is half a pair), 104 (no padding pair on 4 lanes: the accept draw forms its
# own block) — the kernels that take the table (klara_diagt.h diagt_sctab) — and 17 (the smallest layout: its kernels keep the arithmetic, the
# other side of that switch).  driftstep 0.9 / 0.3: at 0.3 the commit / fold path runs on about half the transitions.
# sparse_moves: 0 the device decides launch by launch, 1 the 4-lane kernels, 2 the 8-lane kernels.
# chains: 50 (a partial last wavefront: 16 / 8 chains per wavefront), 197 (13 wavefronts of the 4-lane form: more than one workgroup, the last partial).
JOBS = [(d, h, sm, n) for d in (100, 99, 104, 17) for h in (0.9, 0.3) for sm in (0, 1, 2) for n in (50, 197)]


@pytest.mark.parametrize("d,h,sparse,nchains", JOBS, ids=[f"d{d}_h{h}_lanes{('auto', 'q4', 'q8')[sm]}_n{n}" for d, h, sm, n in JOBS])
def test_table_kernels_bit_for_bit_against_the_oracle(d, h, sparse, nchains):
    _job_against_the_oracle(d, h, sparse, nchains, NSTEPS)


# 36 transitions are a launch of 32 on the table kernel and one of 4 on its arithmetic twin (klara_launch.h diagt_go: fewer than
# KLARA_SCTAB_MIN_STEPS = 8 transitions do not pay for the fill); 39 = 32 + 7 is the longest launch that keeps the arithmetic (40 = 32 + 8, above,
# the shortest that takes the table).  One job carries its state and sums from the one kernel into the other.
SPLITS = [(nsteps, sm) for nsteps in (36, 39) for sm in (0, 1, 2)]


@pytest.mark.parametrize("nsteps,sparse", SPLITS, ids=[f"steps{ns}_lanes{('auto', 'q4', 'q8')[sm]}" for ns, sm in SPLITS])
def test_short_launch_switches_to_the_arithmetic_kernel_mid_job(nsteps, sparse):
    _job_against_the_oracle(100, 0.3, sparse, 197, nsteps)


def _job_against_the_oracle(d, h, sparse, nchains, NSTEPS):
    name = f"mala_d{d}_h{h}_{sparse}_{nchains}_{NSTEPS}"
    kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(d), driftstep=h)
    if sparse:
        kw["sparse_moves"] = sparse
    case = dict(burnin=0, **kw, nchains=nchains, nsteps=NSTEPS, x0=None, seed=20261017, name=name)
    eng = K.Engine(**cases.engine_kwargs(case, monitor=SUMS))
    layout = eng.layout()
    assert layout[:2] == (3, 8), layout
    job = O.OracleJob(**cases.oracle_kwargs(case, layout=layout))
    eng.init_state_normal(); assert job.init_state_normal() == 0
    eng.run(NSTEPS); assert job.run(NSTEPS) == 0
    cnt = [int(c) for c in eng.launch_modes()[0]]              # launches on the 4-lane kernel alone, the 8-lane kernel alone, the device-decided pair
    assert sum(cnt) == 2 and (sparse != 1 or cnt[0] == 2) and (sparse != 2 or cnt[0] == 0), (name, cnt)    # the forced kernel family ran both launches
    mask = eng.accept_mask()
    assert np.array_equal(mask, job.accept), f"{name}: accept mask differs at {np.argwhere(mask != job.accept)[:5]}"
    assert 0 < int(mask.sum()) < mask.size, f"{name}: accepted {int(mask.sum())} of {mask.size}"      # both the commit and the reject path ran
    x, lt, g = eng.state()
    assert np.array_equal(x.view(np.uint64), job.X.view(np.uint64)), f"{name}: values differ"
    assert np.array_equal(lt.view(np.uint64), job.LT.view(np.uint64)), f"{name}: log-target differs"
    assert np.array_equal(g.view(np.uint64), job.G.view(np.uint64)), f"{name}: gradient differs"
    na, nst = eng.accept_counts()
    assert np.array_equal(na, job.naccept) and nst == NSTEPS, f"{name}: accept counts differ"
    s, q, nsaved = eng.chain_sums()
    assert nsaved == NSTEPS
    assert np.array_equal(s.view(np.uint64), job.sum.view(np.uint64)), f"{name}: running sums differ"
    assert np.array_equal(q.view(np.uint64), job.sumsq.view(np.uint64)), f"{name}: running sums of squares differ"
    eng.close()
