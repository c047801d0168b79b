"""The random jobs of tests/matrix_sampler_random.py without a GPU: every committed seed runs on the CPU oracle (oracle/klara_oracle.c:
ko_smmala, ko_ram), the oracle agrees with the NumPy restatements (tests/smmala_mirror.py, tests/ram_mirror.py) on the first
4 chains of every seed, the seeds reach every kernel instantiation and every edge they are there for (the ledger), and the jobs both accept and reject.
profiles/matrix_sampler_sweep.txt records the ledger and the acceptance fractions printed here."""
import functools
from collections import Counter

import numpy as np
import pytest

import matrix_sampler_random as MR
import smmala_mirror as SM
from test_ram_host import S_RTOL, _srel
from test_smmala_host import _ref_vs_mirror as _smmala_ref_vs_mirror

SEEDS = [(f, s) for f in MR.FAMILIES for s in range(MR.NSEEDS[f])]
IDS = [f"{f}-{s}" for f, s in SEEDS]
NMIRROR = 4


@functools.lru_cache(maxsize=None)
def _case(family, seed):
    return MR.random_case(seed, family)


@functools.lru_cache(maxsize=None)
def _reference(family, seed):
    """the whole job on its C reference, once: (status of set_state, status of run, all finite, accepted fraction)"""
    case = _case(family, seed)
    job = MR.MODULES[family].ref_job(case)
    st0 = job.set_state(case["x0"])
    st = job.run(case["nsteps"]) if st0 == 0 else -1
    finite = bool(np.all(np.isfinite(job.X)) and np.all(np.isfinite(job.LT)) and (family == "ram" or np.all(np.isfinite(job.G))))
    if family == "ram":
        finite = finite and bool(np.all(np.isfinite(job.S))) and job.skipped == 0
    return st0, st, finite, float(job.accept.mean())


@pytest.mark.parametrize("family,seed", SEEDS, ids=IDS)
def test_reference_runs_every_seed(family, seed):
    st0, st, finite, _ = _reference(family, seed)
    assert st0 == 0 and st == 0, (st0, st)
    assert finite, "the reference left a non-finite state (RAM: or skipped a factor update)"


def _mirror_rows(case, chains, nsteps):
    if MR.is_pooled(case):
        return SM.run_pooled(chains, nsteps, tuner="rate", targetrate=case["targetrate"], period=case["period"], burnin=case.get("burnin", 0))
    for c in chains:
        c.run(nsteps)
    return np.array([c.accepts for c in chains], dtype=np.uint8).T


@pytest.mark.parametrize("family,seed", SEEDS, ids=IDS)
def test_reference_matches_restatement(family, seed):
    """the first 4 chains, compared as tests/test_smmala_host.py, tests/test_softabs_host.py and tests/test_ram_host.py compare their named cases: accept masks equal,
    X / LT to 1e-10, the gradient to 1e-10 + 1e-9 (SMMALA), the step to 1e-12, RAM's factors to S_RTOL.  No seed is excluded for a near-tie; the restatement does
    not model the erf score, so those SMMALA / softabs seeds are left to test_reference_runs_every_seed."""
    case = _case(family, seed)
    if MR.has_erf_score(case):
        return
    n, nsteps, mod = min(NMIRROR, case["nchains"]), case["nsteps"], MR.MODULES[family]
    if family == "smmala":
        _smmala_ref_vs_mirror(case, nchains=n, nsteps=nsteps, pooled=MR.is_pooled(case))
        return
    job = mod.ref_job(case, nchains=n)
    assert job.set_state(case["x0"][:n]) == 0 and job.run(nsteps) == 0
    chains = mod.mirror_chains(case, nchains=n)
    rows = _mirror_rows(case, chains, nsteps)
    assert np.array_equal(job.accept, rows), "accept masks differ between the C reference and the NumPy restatement"
    np.testing.assert_allclose(job.X, np.array([c.x for c in chains]), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.LT, [c.lt for c in chains], rtol=1e-10, atol=1e-10)
    if family == "softabs":
        steps = job.step if not MR.is_pooled(case) else np.full(n, job.step[0])
        np.testing.assert_allclose(steps, [c.step for c in chains], rtol=1e-12)
    else:
        rel = _srel(job.S, np.array([c.S for c in chains]))
        assert rel <= S_RTOL, f"factor differs from the literal restatement by {rel:.3e} (relative)"
        assert job.skipped == 0


def _ledger(family):
    cs = [_case(family, s) for s in range(MR.NSEEDS[family])]
    inst = [MR.instantiation(c) for c in cs]
    return dict(cases=cs,
                em=Counter((e, m) for _, e, m in inst),
                d_kind=Counter((c["target"].ndims, "logit" if c.run["kind"] == "logit" else "custom") for c in cs),
                source=Counter(c.run["kind"] for c in cs),
                tuner=Counter(MR.tuner_kind(c) for c in cs),
                rowsplit=Counter("rows>=64" if MR.nrows(c) >= 64 else "rows<64" for c in cs if MR.nrows(c) is not None),
                rows=Counter(MR.nrows(c) for c in cs if MR.nrows(c) is not None),
                chains=Counter(c["nchains"] for c in cs))


def test_ledger():
    """what the committed seeds reach: all 12 (E, MODE) pairs of SMMALA and of RAM, E = 2 / 4 / 8 with softabs, every D in 1 .. 8 with both target kinds
    (softabs: both sources, from D = 2 — SRC_MIXED divides by D - 1), every tuner, both row-split states, the 63 / 64 / 65 row edge, and chain counts 1, 64, 65
    and 257"""
    chains, rows = Counter(), Counter()
    for family in MR.FAMILIES:
        led = _ledger(family)
        chains += led["chains"]; rows += led["rows"]
        print(f"\n{family}: seeds {MR.BASE[family]} + 0 .. {MR.NSEEDS[family] - 1}")
        print("  cases per D:", {d: sum(v for (dd, _), v in led["d_kind"].items() if dd == d) for d in range(1, 9)})
        print("  cases per source:", dict(sorted(led["source"].items())), " per tuner:", dict(sorted(led["tuner"].items())))
        print("  cases per (E, MODE):", {k: led["em"][k] for k in sorted(led["em"])})
        print("  row split:", dict(led["rowsplit"]), " rows:", dict(sorted(led["rows"].items())))
        print("  chains:", dict(sorted(led["chains"].items())))
        assert all(led["tuner"][t] > 0 for t in (("vanilla", "verbose") if family == "ram" else ("vanilla", "verbose", "rate", "rate_erf", "pooled"))), sorted(led["tuner"])
        if family == "softabs":
            assert {e for e, _ in led["em"]} == {2, 4, 8}
            kinds = Counter((c["target"].ndims, c.run["kind"]) for c in led["cases"])
            assert all(kinds[(d, "doublewell")] > 0 for d in range(1, 9)) and all(kinds[(d, "mixed")] > 0 for d in range(2, 9)), sorted(kinds)
        else:
            assert all(led["em"][(e, m)] > 0 for e in (2, 4, 8) for m in (0, 1, 3, 7)), sorted(led["em"])
            assert all(led["d_kind"][(d, k)] > 0 for d in range(1, 9) for k in ("logit", "custom")), sorted(led["d_kind"])
            assert led["rowsplit"]["rows<64"] > 0 and led["rowsplit"]["rows>=64"] > 0
    assert all(chains[n] > 0 for n in (1, 64, 65, 257)), sorted(chains)
    assert all(rows[n] > 0 for n in (1, 63, 64, 65)), sorted(rows)


@pytest.mark.parametrize("family", MR.FAMILIES)
def test_the_sweep_is_not_vacuous(family):
    """a condition on the inputs, asserted on the reference alone: at least 90 % of the family's jobs both accept and reject"""
    frac = np.array([_reference(family, s)[3] for s in range(MR.NSEEDS[family])])
    inside = int(np.sum((frac > 0.0) & (frac < 1.0)))
    print(f"\n{family}: acceptance fraction min {frac.min():.3f}, median {np.median(frac):.3f}, max {frac.max():.3f}; {inside} of {frac.size} strictly between 0 and 1")
    assert inside >= 0.9 * frac.size
