"""The jobs of tests/nonfinite_cases.py on the CPU: three restatements agree on them, and the inputs do what they are there for.

For every job the shipped oracle, the literal-mode oracle and the NumPy mirror replay ALL chains (the jobs are at most 200 chains x 24 transitions; the oracle
replays them in blocks of 16 chains, as tests/test_gpu_literal.py does, which also shows that a block does not depend on its neighbours).  Asserted:

  * every accept decision identical between the three;
  * final X, lt and G within 1e-12 (literal) and 1e-9 (mirror) by the measure of tests/test_gpu_literal.py, taken chain by chain (a hot chain's 1e154 must
    not set the scale for its neighbour);
  * borderline transitions: where the mirror's |lt'|, or a sum that enters the decision, lies within 1e-9 relative of DBL_MAX the summation order decides between
    a finite value and an infinity; the chain leaves the mirror comparison from there on, and at most 1 % of a job's chain-transitions may leave it that way;
  * every committed state (final and every saved column) of the oracle is finite, and the largest leapfrog trip count is the job's own (no capped quotient);
  * the coverage conditions below, counted by the mirror's hook (numpy_mirror.Chain.seen), never from the code under test.

Coverage, per job: at least 25 % of the chains never see a non-finite value and accept 20 - 90 % of their transitions (the hierarchical job: 10 %); at least 25 %
of the chains see a non-finite proposal; at least 10 % of the chain-transitions are non-finite, one of them with a NaN where the arithmetic can form one
(nonfinite_cases: `why_no_nan`); at least 5 chains have both an accepted transition and a non-finite proposal (`why_no_both`: where a hot chain's decision
is a function of its state alone).  The headline MALA job at D = 100, whose ratio cannot overflow, is held to its own conditions (`screen_only`).  Literal mode
is not replayed for the logistic jobs (`why_no_literal`); the gradient is compared with literal mode at 1e-12 (the hierarchical target: 1e-10) and with the mirror at 1e-9.

This file is the proof that every job ends within its trip-count bound: the kernels' loops are the oracle's.  A job that fails here is not run on a device.
`python tests/test_nonfinite_host.py [job ...]` prints the figures of profiles/nonfinite_proposals.txt.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import cases  # noqa: E402
import nonfinite_cases as NF  # noqa: E402
import numpy_mirror as M  # noqa: E402
import oracle_ffi as O  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

BLOCK = 16
LITERAL_RTOL, MIRROR_RTOL = 1e-12, 1e-9       # tests/test_gpu_literal.py
EDGE_REL, LEFT_OUT_CAP = 1e-9, 0.01


def oracle_case(job, n=None):
    return dict(job["kw"], nchains=job["n"] if n is None else n, nsteps=job["nsteps"], burnin=job["kw"].get("burnin", 0), name="nonfinite", x0=None, seed=NF.SEED)


def oracle_run(job, x0, literal=False, block=None):
    """the whole job by the oracle on the job's layout (block: in blocks of that many chains) -> dict of arrays"""
    lib = O.load()
    n, ns, d = job["n"], job["nsteps"], job["kw"]["target"].ndims
    cols = ns - job["kw"].get("burnin", 0)                                 # (thinning 1 throughout)
    out = dict(accept=np.zeros((ns, n), np.uint8), X=np.zeros((n, d)), LT=np.zeros(n), G=np.zeros((n, d)), hist=np.zeros((cols, n, d)), hist_g=np.zeros((cols, n, d)),
               sum=np.zeros((n, d)), sumsq=np.zeros((n, d)), step=np.zeros(n), accepted=np.zeros(n, np.int64), proposed=np.zeros(n, np.int64),
               totproposed=np.zeros(n, np.int64), naccept=np.zeros(n, np.uint64), da_epsbar=np.zeros(n), da_hbar=np.zeros(n))
    step = n if block is None else block
    lib.ko_set_literal(1 if literal else 0)
    try:
        for off in range(0, n, step):
            m = min(step, n - off)
            oj = O.OracleJob(**cases.oracle_kwargs(oracle_case(job, m), layout=job["layout"], chain_offset=off), want_hist=True)
            assert oj.set_state(x0[off:off + m]) == 0, "a start state is not finite"
            assert oj.run(ns) == 0
            sl = slice(off, off + m)
            out["accept"][:, sl] = oj.accept
            out["hist"][:, sl], out["hist_g"][:, sl] = oj.hist, oj.hist_g
            for k, v in (("X", oj.X), ("LT", oj.LT), ("G", oj.G), ("sum", oj.sum), ("sumsq", oj.sumsq), ("step", oj.step), ("accepted", oj.accepted),
                         ("proposed", oj.proposed), ("totproposed", oj.totproposed), ("naccept", oj.naccept), ("da_epsbar", oj.da_epsbar), ("da_hbar", oj.da_hbar)):
                out[k][sl] = v
    finally:
        lib.ko_set_literal(0)
    return out


def mirror_run(job):
    smp, (ltf, gradf), ckw = job["mirror"]
    chains = []
    with np.errstate(all="ignore"):
        for k in range(job["n"]):
            c = M.Chain(smp, ltf, gradf, job["x0"][k], NF.SEED, k, nsteps=job["nsteps"], burnin=job["kw"].get("burnin", 0), **ckw)
            c.run(job["nsteps"])
            chains.append(c)
    return chains


def _bad(e):
    return bool(e["lt"] or e["grad"] or e["ratio"] or e["a"])


def coverage(job, chains):
    """the figures of the coverage table, from the mirror's hook"""
    n, ns = job["n"], job["nsteps"]
    bad = np.array([[_bad(e) for e in c.seen] for c in chains])               # (n, ns)
    acc = np.array([c.accepts for c in chains], bool)
    rate = acc.mean(axis=1)
    plain = (~bad.any(axis=1)) & (rate >= 0.2) & (rate <= 0.9)
    cause = {k: int(sum(bool(e[k]) for c in chains for e in c.seen)) for k in ("lt", "grad", "ratio", "a")}
    hot = job["hot"]
    return dict(chains=n, transitions=ns, plain_chains=int(plain.sum()), chains_with_nonfinite=int(bad.any(axis=1).sum()), nonfinite=int(bad.sum()),
                nonfinite_share=float(bad.mean()), with_nan=int(sum(e["nan"] for c in chains for e in c.seen)), by_cause=cause,
                both=int((bad.any(axis=1) & acc.any(axis=1)).sum()), accept_ordinary=float(acc[~hot].mean()), accept_hot=float(acc[hot].mean()),
                max_nleaps=int(max(getattr(c, "max_nleaps", 0) for c in chains)))


def _dev(a, b):
    """tests/test_gpu_literal.py's measure max |a - b| / (|b| + mean |b|), for one chain's values"""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    return float(np.max(np.abs(a - b) / (np.abs(b) + np.abs(b).mean() + 5e-324)))


def check_job(name):
    job = NF.jobs()[name]
    n, ns = job["n"], job["nsteps"]
    assert n <= 200 and ns <= 24
    assert job["hot"][1::2].all() and not job["hot"][0::2].any()          # hot and ordinary chains alternate: both kinds in every wavefront and 16-chain tile
    needg = job["kw"]["sampler"] != L.SAMPLER_MH
    ship = oracle_run(job, job["x0"], block=BLOCK)
    whole = oracle_run(job, job["x0"])
    for k in ship:                                                         # a block of 16 replays alone: no chain depends on a neighbour
        assert np.array_equal(ship[k], whole[k], equal_nan=True), (name, k, "the oracle's chains are not independent")
    lit = oracle_run(job, job["x0"], literal=True, block=BLOCK) if not job["why_no_literal"] else ship
    chains = mirror_run(job)
    cov = coverage(job, chains)
    # ---- a committed state is always finite; the oracle's tuner state too (no NaN step: no capped trip count)
    for k in ("X", "LT", "hist") + (("G", "hist_g") if needg else ()):
        assert np.isfinite(ship[k]).all(), (name, k, "the oracle committed a non-finite value")
    assert np.isfinite(ship["step"]).all() and cov["max_nleaps"] <= 256, (name, "a step is not finite, or a trajectory is longer than 256 steps")
    # ---- literal mode: every decision, final state
    assert np.array_equal(ship["accept"], lit["accept"]), (name, "shipped and literal oracle decide differently", np.argwhere(ship["accept"] != lit["accept"])[:5])
    worst_lit = 0.0
    for c in range(n):
        devs = [_dev(lit["X"][c], ship["X"][c]), _dev(lit["LT"][c], ship["LT"][c])]
        assert max(devs) <= job["rtol"], (name, c, devs)
        if needg:
            gd = _dev(lit["G"][c], ship["G"][c])
            assert gd <= job["gtol"], (name, c, gd)
        worst_lit = max(worst_lit, *devs)
    # ---- the mirror: every decision up to a chain's first borderline transition, final state of the chains that never had one
    left, worst_mir = 0, 0.0
    for c, ch in enumerate(chains):
        edge = [i for i, e in enumerate(ch.seen) if np.isfinite(e["edge"]) and abs(e["edge"] / NF.DBL_MAX - 1.0) <= EDGE_REL]
        upto = edge[0] if edge else ns
        left += ns - upto
        assert np.array_equal(ship["accept"][:upto, c].astype(bool), np.array(ch.accepts[:upto], bool)), (name, c, "oracle and mirror decide differently")
        if upto == ns:
            devs = [_dev(ch.x, ship["X"][c]), _dev(ch.lt, ship["LT"][c])] + ([_dev(ch.g, ship["G"][c])] if needg else [])
            assert max(devs[:2]) <= MIRROR_RTOL and (not needg or devs[2] <= max(MIRROR_RTOL, job["gtol"])), (name, c, devs)
            worst_mir = max(worst_mir, *devs)
    cov.update(left_out=left, left_out_share=left / (n * ns), dev_vs_literal=worst_lit, dev_vs_mirror=worst_mir, acceptance=float(ship["accept"].mean()))
    assert cov["left_out_share"] <= LEFT_OUT_CAP, (name, cov)
    # ---- the coverage conditions
    print({"job": name, **cov})
    if job["screen_only"]:
        # jobs whose arithmetic cannot form a non-finite value (nonfinite_cases.SCREEN_ONLY, GRADIENT_ONLY), which the hook confirms.  Their inputs put huge
        # values beside ordinary chains that move: every hot chain starts beyond 1e152, and some ordinary chain accepts and some ordinary proposal is rejected
        assert cov["nonfinite"] == 0 and cov["with_nan"] == 0, (name, cov)
        assert (np.abs(job["x0"][job["hot"]]).max(axis=1) > 1e152).all() and (np.abs(job["x0"][~job["hot"]]).max(axis=1) < 1e152).all(), name
        ordinary = ship["accept"][:, ~job["hot"]]
        assert 0 < ordinary.sum() < ordinary.size, (name, "the ordinary chains do not both accept and reject")
        if name == "pair_negdot_d100_mala":          # sum x^2 on both sides of the screen's gate 2^1000, and a run with one transition per launch
            q = np.sum(job["x0"][2::4] ** 2, axis=1)
            assert (q < 2.0 ** 1000).sum() >= 5 and (q > 2.0 ** 1000).sum() >= 5 and 1 in job["spl"], (name, q)
        return cov
    assert cov["plain_chains"] >= job["min_plain"] * n, (name, "too few ordinary chains that move", cov)
    assert cov["chains_with_nonfinite"] >= 0.25 * n, (name, "too few chains see a non-finite proposal", cov)
    assert cov["nonfinite_share"] >= 0.10, (name, "too few non-finite chain-transitions", cov)
    # (where a reason says that the arithmetic cannot form a NaN, or that no hot chain can both accept and overflow, the reason is checked: the count is 0)
    assert cov["with_nan"] == 0 if job["why_no_nan"] else cov["with_nan"] >= 1, (name, "NaN among the non-finite proposals", cov)
    assert cov["both"] == 0 if job["why_no_both"] else cov["both"] >= 5, (name, "chains that both accept and see a non-finite proposal", cov)
    return cov


@pytest.mark.parametrize("name", list(NF.jobs()))
def test_oracle_literal_and_mirror_agree_on_non_finite_proposals(name):
    check_job(name)


if __name__ == "__main__":
    import json
    for nm in (sys.argv[1:] or list(NF.jobs())):
        try:
            print(json.dumps({"job": nm, **check_job(nm)}))
        except AssertionError as e:
            print("FAILED", nm, str(e)[:1500])
