"""The AMWG kernels over the random jobs of amwg_cases.random_case: bit for bit against the CPU reference (tests/amwg_ref.py) at D in 1 .. 16 on the logistic
target (E = 2 .. 16, both sides of the 64-row edge of the row split) and D in 1 .. 32 on user-defined closures (plain, half-space, likelihood + prior),
chain counts around one wavefront and one workgroup, every monitor word, launch lengths 1 / 7 / the default, split runs, shard offsets, periods 2 .. 9 and
three target rates.  It follows tests/test_gpu_am_random.py."""
import numpy as np
import pytest

import amwg_cases as WC
import klara_jl_amd as K
import matrix_sampler_random as MR
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu


def _run_pair(case, monitor, steps_per_launch, chain_offset, runs):
    eng = K.Engine(**WC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset))
    eng.set_state(case["x0"])
    job = WC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, want_hist=bool(monitor & L.MON_HISTORY))
    assert job.set_state(case["x0"]) == 0
    for k in runs:
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_same(eng, job, monitor):
    """as far as the monitor word keeps it: without a monitor the state and the sampler's own state alone"""
    x, lt, _ = eng.state()
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    ls, acc, nacc = eng.amwg_state()
    assert np.array_equal(ls, job.logsigma), "log proposal scales differ from the reference"
    assert np.array_equal(acc, job.accepted) and np.array_equal(nacc, job.naccept_coord), "per-coordinate counts differ from the reference"
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
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, _ = eng.chain_fields(c, logtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"


@pytest.mark.parametrize("seed", range(WC.RANDOM_NSEEDS))
def test_random_configurations(gpu_required, seed):
    case = WC.random_case(seed)
    r = case.run
    eng, job = _run_pair(case, r["monitor"], r["steps_per_launch"], r["chain_offset"], r["runs"])
    d = case["target"].ndims
    rows = MR.nrows(case)
    if rows is not None:
        e = 2 if d <= 2 else 4 if d <= 4 else 8 if d <= 8 else 16
        assert eng.layout() == ((2, 4) if rows >= 64 else (0, 1)) + (e,), (eng.layout(), rows)          # kind 2: RS = 4 lanes share a chain's rows
    else:
        assert eng.layout() == (0, 1, max(2, 1 << (d - 1).bit_length())), eng.layout()
    _assert_same(eng, job, r["monitor"])
    eng.close()
