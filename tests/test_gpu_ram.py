"""The RAM kernels on the GPU: bit for bit against the CPU reference (oracle/klara_oracle.c ko_ram) — the factors included —, launch-length and sharding
invariance, klara_reset, the factor round trip, refusals, and a check that needs no reference: the factor learns the target's covariance shape
at the target acceptance rate."""
from pathlib import Path

import numpy as np
import pytest

import klara_jl_amd as K
import ram_cases as RC
from klara_jl_amd import _lib as L

pytestmark = pytest.mark.gpu

HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT


def _run_pair(case, monitor=HIST, steps_per_launch=0, chain_offset=0, nchains=None, runs=None):
    n = case["nchains"] if nchains is None else nchains
    x0 = case["x0"][chain_offset:chain_offset + n]
    eng = K.Engine(**RC.engine_kwargs(case, monitor=monitor, steps_per_launch=steps_per_launch, chain_offset=chain_offset, nchains=n))
    job = RC.ref_job(case, layout=eng.layout(), chain_offset=chain_offset, nchains=n, want_hist=bool(monitor & L.MON_HISTORY))
    eng.set_state(x0)
    assert job.set_state(x0) == 0
    for k in (runs or [case["nsteps"]]):
        eng.run(k)
        assert job.run(k) == 0
    return eng, job


def _assert_same(eng, job, hist=True):
    x, lt, _ = eng.state()
    assert np.array_equal(eng.accept_mask(), job.accept), "accept mask differs from the reference"
    assert np.array_equal(x, job.X) and np.array_equal(lt, job.LT), "state differs from the reference"
    S, skipped = eng.ram_factor()
    assert np.array_equal(S, job.S), "factors differ from the reference"
    assert skipped == job.skipped == 0
    s, q, _ = eng.chain_sums()
    assert np.array_equal(s, job.sum) and np.array_equal(q, job.sumsq), "running sums differ from the reference"
    _, a, p, t = eng.tune()
    assert np.array_equal(a, job.accepted) and np.array_equal(p, job.proposed) and np.array_equal(t, job.totproposed), "tuner counters differ"
    if hist:
        for c in (0, job.N // 2, job.N - 1):
            v = eng.chain(c)
            assert np.array_equal(v, job.hist[:v.shape[1], c, :].T), f"value history of chain {c} differs"
            lt_h, _ = eng.chain_fields(c, logtarget=True)
            assert np.array_equal(lt_h, job.hist_lt[:lt_h.size, c]), f"log-target history of chain {c} differs"


@pytest.mark.parametrize("name", RC.ALL)
def test_bit_exact_against_the_reference(gpu_required, name):
    case = RC.make(name)
    eng, job = _run_pair(case)
    _assert_same(eng, job)
    assert 0.0 < job.accept.mean() < 1.0
    if name == "logit_d8_verbose":
        assert job.proposed.max() > 0 and job.totproposed.min() > case["period"], "the verbose tuner counted nothing"
    eng.close()


@pytest.mark.parametrize("monitor", [0, L.MON_ACCEPT, HIST])
@pytest.mark.parametrize("name", ["swiss_example", "logit_d3"])
def test_launch_length_does_not_change_the_bits(gpu_required, name, monitor):
    """steps_per_launch 1 / 7 / 32: the factors travel through memory between launches (monitor 0 of these plain jobs: MODE 3 and the
    one-transition kernel, MODE 7)"""
    case = RC.make(name)
    out = []
    for spl in (1, 7, 32):
        eng = K.Engine(**RC.engine_kwargs(case, monitor=monitor, steps_per_launch=spl))
        eng.set_state(case["x0"])
        eng.run(case["nsteps"])
        x, lt, _ = eng.state()
        S, skipped = eng.ram_factor()
        out.append((x, lt, S, np.int64(skipped)) + ((eng.accept_mask(),) if monitor & L.MON_ACCEPT else ()))
        eng.close()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)
    job = RC.ref_job(case)
    assert job.set_state(case["x0"]) == 0 and job.run(case["nsteps"]) == 0
    assert np.array_equal(out[0][0], job.X) and np.array_equal(out[0][2], job.S)


def test_split_runs_and_reset(gpu_required):
    case = RC.make("swiss_example")
    eng, job = _run_pair(case, runs=[13, 1, 26])
    _assert_same(eng, job)
    S0 = np.broadcast_to(np.eye(4), (case["nchains"], 4, 4))
    # reset(job): the next Philox key; S = S0 and the count restart (RAM.jl:201-211)
    eng.reset(); assert job.reset() == 0
    S, skipped = eng.ram_factor()
    assert np.array_equal(S, S0) and skipped == 0
    eng.run(17); assert job.run(17) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.state()[1], job.LT)
    assert np.array_equal(eng.accept_mask(), job.accept) and np.array_equal(eng.ram_factor()[0], job.S)
    x1 = RC.SWISS_X0[None, :] + np.zeros((case["nchains"], 4))
    eng.reset(x1); assert job.reset(x1) == 0
    assert np.array_equal(eng.ram_factor()[0], S0)
    eng.run(9); assert job.run(9) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.accept_mask(), job.accept) and np.array_equal(eng.ram_factor()[0], job.S)
    eng.close()


def test_chain_offset_sharding(gpu_required):
    """two shards with chain_offset draw and adapt what one job of all chains does"""
    case = RC.make("logit_d8")
    whole = K.Engine(**RC.engine_kwargs(case))
    whole.set_state(case["x0"]); whole.run(case["nsteps"])
    xw, Sw = whole.state()[0], whole.ram_factor()[0]
    whole.close()
    xs, Ss = [], []
    for off, n in ((0, 20), (20, case["nchains"] - 20)):
        e = K.Engine(**RC.engine_kwargs(case, chain_offset=off, nchains=n))
        e.set_state(case["x0"][off:off + n]); e.run(case["nsteps"])
        xs.append(e.state()[0]); Ss.append(e.ram_factor()[0]); e.close()
    assert np.array_equal(np.concatenate(xs), xw) and np.array_equal(np.concatenate(Ss), Sw)
    eng, job = _run_pair(case, chain_offset=20, nchains=case["nchains"] - 20)
    _assert_same(eng, job)
    eng.close()


def test_factor_round_trip_and_warm_start(gpu_required):
    case = RC.make("gauss_d3")
    n = case["nchains"]
    rng = np.random.default_rng(77)
    F = np.tril(0.2 * rng.standard_normal((n, 3, 3)))
    F[:, [0, 1, 2], [0, 1, 2]] = 0.4 + rng.random((n, 3))
    eng = K.Engine(**RC.engine_kwargs(case))
    job = RC.ref_job(case, layout=eng.layout())
    eng.set_state(case["x0"]); assert job.set_state(case["x0"]) == 0
    eng.set_ram_factor(F); job.set_factor(F)
    assert np.array_equal(eng.ram_factor()[0], F)
    eng.run(15); assert job.run(15) == 0
    assert np.array_equal(eng.state()[0], job.X) and np.array_equal(eng.accept_mask(), job.accept) and np.array_equal(eng.ram_factor()[0], job.S)
    eng.close()


def test_refusals(gpu_required):
    case = RC.make("logit_d3")
    eng = K.Engine(**RC.engine_kwargs(case))
    with pytest.raises(K.KlaraError) as ei:                       # before set_state
        eng.set_ram_factor(np.eye(3))
    assert ei.value.status == L.ERR_STATE
    x0 = case["x0"].copy(); x0[5, 1] = np.nan
    with pytest.raises(K.KlaraError) as ei:
        eng.set_state(x0)
    assert ei.value.status == L.ERR_NONFINITE_INIT
    eng.set_state(case["x0"])                                     # ... and the job goes on from valid values
    eng.run(3)
    for bad in (0.0, -1.0, np.nan, np.inf):
        F = np.broadcast_to(0.3 * np.eye(3), (case["nchains"], 3, 3)).copy()
        F[7, 2, 2] = bad
        with pytest.raises(K.KlaraError) as ei:
            eng.set_ram_factor(F)
        assert ei.value.status == L.ERR_INVALID_ARG
    eng.close()
    kw = RC.engine_kwargs(case)
    kw.update(sampler=L.SAMPLER_MH, mh_sigma=np.ones(3), ram_S0=None, ram_targetrate=0.0, ram_gamma=0.0)
    mh = K.Engine(**kw)
    mh.set_state(case["x0"])
    with pytest.raises(K.KlaraError) as ei:
        mh.ram_factor()
    assert ei.value.status == L.ERR_INVALID_ARG
    with pytest.raises(K.KlaraError) as ei:
        mh.set_ram_factor(np.eye(3))
    assert ei.value.status == L.ERR_INVALID_ARG
    mh.close()


@pytest.mark.parametrize("fname", ["ram_swiss", "ram_gauss_d3"])
def test_goldens(gpu_required, fname):
    """tests/golden/make_golden_ram.py: the committed reference vectors, bit for bit"""
    g = np.load(Path(__file__).resolve().parent / "golden" / f"{fname}.npz")
    case = RC.make({"ram_swiss": "swiss_example", "ram_gauss_d3": "gauss_d3"}[fname])
    eng = K.Engine(**RC.engine_kwargs(case))
    eng.set_state(g["x0"]); eng.run(case["nsteps"])
    x, lt, _ = eng.state()
    S, skipped = eng.ram_factor()
    assert np.array_equal(eng.accept_mask(), g["accept"])
    assert np.array_equal(x, g["X"]) and np.array_equal(lt, g["LT"]) and np.array_equal(S, g["S"]) and skipped == int(g["skipped"])
    eng.close()


@pytest.mark.parametrize("d, max_shape_error", [(2, 0.05), (3, 0.20)])
def test_factor_learns_the_covariance_shape_at_the_target_rate(gpu_required, d, max_shape_error):
    """no reference needed: on N(0, P^-1) with condition number 50, 4,096 chains started in equilibrium with RAM(ones(d)), targetrate 0.234,
    gamma 0.7.  After 2,000 transitions the acceptance over the last 1,000 is within 0.02 of 0.234 (the reference algorithm, restated in NumPy with
    two seeds: 0.2428 / 0.2432 at d = 2, 0.2443 / 0.2444 at d = 3; standard error 2e-4, the finite-time bias above the target is the algorithm's
    own), and the median over the chains of || C / tr C - Sigma / tr Sigma ||_F / || Sigma / tr Sigma ||_F with C = S S', Sigma = P^-1 is at most
    0.05 (d = 2; measured 0.023 / 0.024) or 0.20 (d = 3; 0.119 / 0.120) — at the start S0 = I it is 0.69 / 0.75, so a kernel that never
    updates S cannot pass."""
    n, steps = 4096, 2000
    P = RC.conditioned_precision(d, 50.0, seed=d)
    Sigma = np.linalg.inv(P)
    x0 = np.random.default_rng(100 + d).standard_normal((n, d)) @ np.linalg.cholesky(Sigma).T
    eng = K.Engine(sampler=L.SAMPLER_RAM, target=RC.quad_target(0.5, P, P), nchains=n, nsteps=steps, ram_S0=np.ones(d), ram_targetrate=0.234,
                   ram_gamma=0.7, seed=9000 + d)
    eng.set_state(x0)
    eng.run(steps // 2)
    a1, n1 = eng.accept_counts()
    eng.run(steps // 2)
    a2, n2 = eng.accept_counts()
    S, skipped = eng.ram_factor()
    eng.close()
    assert n1 == steps // 2 and n2 == steps
    rate = float((a2.astype(np.int64) - a1.astype(np.int64)).mean()) / (steps // 2)
    Cm = S @ np.transpose(S, (0, 2, 1))
    Cn = Cm / np.trace(Cm, axis1=1, axis2=2)[:, None, None]
    Sn = Sigma / np.trace(Sigma)
    err = np.linalg.norm(Cn - Sn, axis=(1, 2)) / np.linalg.norm(Sn)
    start = np.linalg.norm(np.eye(d) / d - Sn) / np.linalg.norm(Sn)
    print(f"d = {d}: acceptance over the last {steps // 2} transitions {rate:.4f}, median shape error {np.median(err):.4f} (start {start:.2f}), skipped {skipped}")
    assert abs(rate - 0.234) <= 0.02, rate
    assert np.median(err) <= max_shape_error, np.median(err)
    assert start > 0.6
    assert skipped == 0
