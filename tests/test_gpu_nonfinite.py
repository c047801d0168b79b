"""The transition kernels on proposals that are not finite (-m gpu): the jobs of tests/nonfinite_cases.py through the C ABI.

Every parity test elsewhere runs well-scaled jobs; here half of the chains of every job regularly propose a point whose log-target, ratio or Hamiltonian is -inf
or NaN (tests/test_nonfinite_host.py counts how often, on the CPU, and is the proof that every job ends within its trip counts).  The contract (DESIGN.md
section 2, "Proposals that are not finite"): a ratio of -inf or NaN rejects; after a rejection nothing of the proposal survives in X, lt, G, the history
columns, sum / sumsq, the batch means or the tuner's counters; a committed state is finite; a chain never influences another chain.

Each job runs with MON_ACCEPT | MON_SUMMARIES | MON_HISTORY (and MON_HIST_GRAD where the sampler holds a gradient: klara_create refuses it for MH), once in one
launch and once with three transitions per launch (the D = 100 jobs also with one), two of them with bm_batchlen = 4:

  (a) against the shipped oracle on the layout the device reports (which must be the job's): accept masks, X, lt, G, sum, sumsq, accept counts, tuner counters
      and steps, every history column (and the batch means) bit-equal on uint64 views.  Where the ORACLE's value is a NaN the device's must be one too (x86 and
      gfx950 differ in a NaN's sign and payload); that may happen in sumsq and in the batch means of a HOT chain (squares of 1e154 are infinite, and a
      difference of two infinities is a NaN) and never in X, lt, G, the history, the tuner's state or an ordinary chain's row.
  (b) without an oracle: every value of the final state and of every saved column is finite.
  (c) isolation: the same job again with the hot chains' start rows replaced by ordinary rows.  Every ordinary chain's masks, state, sums, counters and history
      are bit-identical between the two runs: the chains share a wavefront or a tile of the matrix cores and nothing else, so a difference is one chain's value
      in a neighbour's arithmetic (a padding zero times an infinity, a shared tile row, a reduction that crosses chains).

Sensitivity, on a scratch copy (profiles/nonfinite_proposals.txt): HMC's `1.0 < e ? 1.0 : e` written as fmin(1.0, e), a MALA commit written as
x + acc (xp - x), and the proposal instead of the kept state added to `sum` on rejection each turn tests of this file red.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
import nonfinite_cases as NF  # noqa: E402
import oracle_ffi as O  # noqa: E402
import test_nonfinite_host as H  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

NAN_ALLOWED = ("sumsq", "bm")          # where the oracle's own value may be a NaN, and then in a hot chain's row only: the squares of 1e154 are +inf there


def _needg(job):
    return job["kw"]["sampler"] != L.SAMPLER_MH


def device_run(job, x0, spl):
    """the job through the C ABI -> the arrays H.oracle_run returns (plus layout, and bm where the job streams batch means)"""
    n, ns, d = job["n"], job["nsteps"], job["kw"]["target"].ndims
    mon = NF.MONITOR if _needg(job) else NF.MONITOR & ~L.MON_HIST_GRAD
    eng = K.Engine(nchains=n, nsteps=ns, seed=NF.SEED, monitor=mon, steps_per_launch=spl, bm_batchlen=job["bm"], **job["kw"])
    try:
        out = dict(layout=tuple(eng.layout()))
        eng.set_state(x0)
        eng.run(ns)
        out["accept"] = eng.accept_mask()
        out["X"], out["LT"], out["G"] = eng.state()
        out["sum"], out["sumsq"], nsaved = eng.chain_sums()
        out["naccept"], nst = eng.accept_counts()
        out["step"], out["accepted"], out["proposed"], out["totproposed"] = eng.tune()
        cols = ns - job["kw"].get("burnin", 0)
        assert nsaved == cols and nst == ns
        out["hist"] = np.stack([eng.chain(c).T for c in range(n)], axis=1)                                  # (cols, n, d)
        if _needg(job):
            out["hist_g"] = np.stack([eng.chain_fields(c, logtarget=False, gradlogtarget=True)[1].T for c in range(n)], axis=1)
        if job["bm"]:
            out["bm"], out["nb"] = eng.chain_bm()
        if job["kw"].get("tuner") == L.TUNER_DUAL_AVERAGING:
            out["da_epsbar"], out["da_hbar"] = eng.dual_averaging()
    finally:
        eng.close()
    return out


_refs = {}


def oracle_reference(name, which):
    """the shipped oracle's run of the job from x0 (which = "x0") or from the ordinary rows (which = "cool"): computed once, shared by both launch splittings"""
    if (name, which) not in _refs:
        job = NF.jobs()[name]
        ref = H.oracle_run(job, job[which])
        if job["bm"]:
            oj = O.OracleJob(**cases.oracle_kwargs(H.oracle_case(job), layout=job["layout"]))
            assert oj.set_state(job[which]) == 0
            with np.errstate(all="ignore"):
                ref["bm"], ref["nb"] = oj.run_with_batch_means(job["nsteps"], job["bm"])
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[(name, which)] = ref
    return _refs[(name, which)]


def _same_bits(dev, ref, key, name, rows=None, hot=None):
    """bit-equal on uint64 views; where the reference is a NaN (NAN_ALLOWED only) the device's value must be a NaN"""
    a, b = np.ascontiguousarray(dev[key]), np.ascontiguousarray(ref[key])
    assert a.shape == b.shape, (name, key, a.shape, b.shape)
    if rows is not None:                                   # the chain axis: the last but one of the histories, the last of the masks, else the first
        ax = {"accept": 1, "hist": 1, "hist_g": 1}.get(key, 0)
        a, b = np.ascontiguousarray(np.take(a, rows, axis=ax)), np.ascontiguousarray(np.take(b, rows, axis=ax))
    if a.dtype.kind != "f":
        assert np.array_equal(a, b.astype(a.dtype)), (name, key, np.argwhere(a != b.astype(a.dtype))[:5])
        return
    nan = np.isnan(b)
    assert not nan.any() or (key in NAN_ALLOWED and hot is not None and not nan[~hot].any()), (name, key, "the reference holds a NaN where none may be")
    assert np.isnan(a[nan]).all(), (name, key, "a NaN of the oracle is a number on the device")
    ua, ub = a.view(np.uint64), b.view(np.uint64)
    diff = (ua != ub) & ~nan
    assert not diff.any(), (name, key, int(diff.sum()), np.argwhere(diff)[:5], a[diff][:3], b[diff][:3])


@pytest.mark.parametrize("name,spl", [(nm, spl) for nm, jb in NF.jobs().items() for spl in jb["spl"]])
def test_kernels_hold_the_contract_on_non_finite_proposals(name, spl):
    job = NF.jobs()[name]
    dev = device_run(job, job["x0"], spl)
    assert dev["layout"][0] == job["kind"] and dev["layout"] == job["layout"], (name, "the job did not run on the kernel family it is here for", dev["layout"], job["layout"])
    keys = ["accept", "X", "LT", "sum", "sumsq", "naccept", "step", "accepted", "proposed", "totproposed", "hist"] + (["G", "hist_g"] if _needg(job) else [])
    keys += ["da_epsbar", "da_hbar"] if "da_epsbar" in dev else []
    # ---- (a) the shipped oracle, bit for bit
    ref = oracle_reference(name, "x0")
    assert 0 < int(ref["accept"].sum()) < ref["accept"].size
    for k in keys:
        _same_bits(dev, ref, k, name, hot=job["hot"])
    if job["bm"]:
        assert dev["nb"] == ref["nb"] == (job["nsteps"] - job["kw"].get("burnin", 0)) // job["bm"] >= 2
        _same_bits(dev, ref, "bm", name, hot=job["hot"])
    assert np.isfinite(dev["step"]).all(), (name, "a step that is not finite: a dead chain")
    # ---- (b) a committed state is finite, whatever any oracle says
    for k in ("X", "LT", "hist") + (("G", "hist_g") if _needg(job) else ()):
        assert np.isfinite(dev[k]).all(), (name, k, "a non-finite value was committed", np.argwhere(~np.isfinite(dev[k]))[:5])
    # ---- (c) isolation: the ordinary chains do not notice what their neighbours are
    cool = device_run(job, job["cool"], spl)
    rows = np.flatnonzero(~job["hot"])
    assert np.array_equal(job["x0"][rows], job["cool"][rows])
    for k in keys + (["bm"] if job["bm"] else []):
        _same_bits(dev, cool, k, name, rows=rows)
    # (and the second run is a job like any other: the oracle again, which also shows that the hot rows' replacements are ordinary)
    refc = oracle_reference(name, "cool")
    for k in keys:
        _same_bits(cool, refc, k, name)
