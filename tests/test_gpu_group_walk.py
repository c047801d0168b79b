"""A persistent wavefront of the group-layout transition kernel that walks over several chain groups, for every sampler the kernel serves: MH, MALA,
HMC, the slice sampler, SMMALA, RAM, AM and AMWG on the swiss logistic regression (D = 4), bit for bit against the CPU oracle (oracle_ffi.OracleJob; its
subclasses for the samplers that carry a matrix per chain; for AMWG tests/amwg_ref.py, which evaluates through an OracleJob).

The plan gives a wavefront more than one group only from 16,384 groups upwards, so at test sizes the per-group set-up and tear-down of the kernel's
persistent loop — the reload or the hand-over of the prefetched group, the sampler's per-chain state taken up and put back — runs only under the
KLARA_GROUPS_PER_WAVE override.  With 8 groups per wavefront and 517 chains every chains-per-wavefront value of the layouts leaves more groups than
wavefronts and a short last group (64: 9 groups on 4 wavefronts; 32: 17 on 4; 16: 33 on 8; 8: 65 on 12): some wavefront walks three groups or more,
one of them partial.  The test asserts that from the engine's layout.

12 transitions, burn-in 2, thinning 2; monitored (sums, history, accept mask: MODE 1) and unmonitored (MODE 3), each fused and with one transition per
launch (MODE 7 when unmonitored: the prefetching path).  The reference of a sampler is computed once and shared."""
import functools

import numpy as np
import pytest

import am_cases as AC
import amwg_cases as WC
import cases
import klara_jl_amd as K
import oracle_ffi as O
import ram_cases as RC
import smmala_cases as SC
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

NCHAINS, GROUPS_PER_WAVE = 517, 8
HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT
SAMPLERS = ["mh", "mala", "hmc", "slice", "smmala", "ram", "am", "amwg"]
CARRIES_GRADIENT = ("mala", "hmc", "smmala")


def make(name):
    X, y = cases.swiss_data()
    x0 = SC.SWISS_X0[None, :] + 0.05 * np.random.default_rng(17).standard_normal((NCHAINS, 4))
    kw = {"mh": dict(sampler=L.SAMPLER_MH, mh_sigma=np.full(4, 0.3)),
          "mala": dict(sampler=L.SAMPLER_MALA, driftstep=0.25),
          "hmc": dict(sampler=L.SAMPLER_HMC, leapstep=0.4, nleaps=3),
          "slice": dict(sampler=L.SAMPLER_SLICE, slice_widths=np.full(4, 1.0)),
          "smmala": dict(sampler=L.SAMPLER_SMMALA, driftstep=0.006),
          "ram": dict(sampler=L.SAMPLER_RAM, ram_targetrate=0.234, ram_gamma=0.7, ram_S0=np.eye(4)),
          "am": dict(am_C0=np.eye(4), **AC.am(4, 4, minorscale=0.04)),            # t0 = 4: the covariance adapts within the 12 transitions
          "amwg": dict(amwg_logsigma0=np.log(np.full(4, 0.5)), **WC.amwg(period=5))}[name]   # two tuning events
    return dict(target=K.LogisticTarget(X, y, 100.0), nchains=NCHAINS, nsteps=12, burnin=2, thinning=2, x0=x0, name=name, **kw)


def layout_of(case):
    t = case["target"]
    return O.default_layout(t.kind, t.ndims, int(t.X.shape[0]), sampler=L.SAMPLER_MH)


def ref_job(name, case):
    family = {"smmala": SC, "ram": RC, "am": AC, "amwg": WC}.get(name)
    if family is not None:
        return family.ref_job(case, layout=layout_of(case), want_hist=True)
    return O.OracleJob(**cases.oracle_kwargs(case, layout=layout_of(case)), want_hist=True)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the CPU reference of sampler `name` after all 12 transitions, history on; shared by the four launch shapes, never modified"""
    case = make(name)
    job = ref_job(name, case)
    assert job.set_state(case["x0"]) == 0 and job.run(case["nsteps"]) == 0
    return job


def assert_walks_several_groups(eng):
    """the precondition: more chain groups than the launch has wavefronts (workgroups of 256 threads: 4 per block of the grid), the last one short"""
    kind, g, e = eng.layout()
    assert kind in (0, 2), (kind, g, e)
    cpw = 64 // g                                   # chains per wavefront: G lanes per chain (kind 0) or per row-split group (kind 2)
    groups = -(-NCHAINS // cpw)
    grid = -(-(-(-groups // GROUPS_PER_WAVE)) // 4)
    assert groups > 4 * grid, f"layout {(kind, g, e)}: {groups} groups on {4 * grid} wavefronts — no wavefront takes a second group"
    assert -(-groups // (4 * grid)) >= 3 and NCHAINS % cpw != 0, (groups, grid, cpw)


def assert_sampler_state(name, eng, job, monitor):
    if name == "ram":
        S, skipped = eng.ram_factor()
        assert np.array_equal(S, job.S), "RAM factors differ from the oracle"
        assert skipped == job.skipped
    elif name == "am":
        Cm, m, m2, fallbacks = eng.am_state()
        assert np.array_equal(Cm, job.C), "AM covariances differ from the oracle"
        assert np.array_equal(m, job.lastmean) and np.array_equal(m2, job.secondlastmean), "AM running means differ from the oracle"
        assert fallbacks == job.fallbacks
    elif name == "amwg":
        ls, acc, nacc = eng.amwg_state()
        assert np.array_equal(ls, job.logsigma), "AMWG log proposal scales differ from the reference"
        assert np.array_equal(acc, job.accepted) and np.array_equal(nacc, job.naccept_coord), "AMWG counts differ from the reference"
        if monitor & L.MON_ACCEPT:
            assert np.array_equal(eng.amwg_accept_mask(), job.masks), "AMWG coordinate masks differ from the reference"


@pytest.mark.parametrize("steps_per_launch", [0, 1])
@pytest.mark.parametrize("monitor", [HIST, 0])
@pytest.mark.parametrize("name", SAMPLERS)
def test_wavefront_walks_several_chain_groups(gpu_required, monkeypatch, name, monitor, steps_per_launch):
    monkeypatch.setenv("KLARA_GROUPS_PER_WAVE", str(GROUPS_PER_WAVE))
    case = make(name)
    job = reference(name)
    eng = K.Engine(**cases.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch))
    try:
        assert eng.layout() == layout_of(case), (eng.layout(), layout_of(case))
        assert_walks_several_groups(eng)
        eng.set_state(case["x0"])
        eng.run(case["nsteps"])
        x, lt, g = eng.state()
        assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the oracle"
        if name in CARRIES_GRADIENT:
            assert np.array_equal(g, job.G), "gradient differs from the oracle"
        a, n = eng.accept_counts()
        assert np.array_equal(a, job.naccept) and n == job.t == case["nsteps"]
        assert_sampler_state(name, eng, job, monitor)
        if monitor:
            assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the oracle"
            s, q, nsaved = eng.chain_sums()
            assert nsaved == job.hist_cols == 5
            assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the oracle"
            for c in (0, 63, 64, 256, 511, 512, NCHAINS - 1):          # first and last chains of groups, the short last group
                v = eng.chain(c)
                assert v.shape[1] == job.hist_cols and np.array_equal(v, job.hist[:, c, :].T), f"value history of chain {c} differs"
                lt_h, _ = eng.chain_fields(c, logtarget=True)
                assert np.array_equal(lt_h, job.hist_lt[:, c]), f"log-target history of chain {c} differs"
        if name not in ("slice", "amwg"):              # (those two always move) a sampler that never or always accepts would hide a lost group
            assert 0.0 < job.accept.mean() < 1.0
    finally:
        eng.close()
