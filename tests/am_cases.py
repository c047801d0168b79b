"""AM jobs shared by tests/test_am_host.py, tests/test_gpu_am.py and tests/test_gpu_am_random.py.

A case is a dict of Engine keyword arguments plus "x0" (cases.engine_kwargs turns it into an Engine's); `ref_job(case)` builds the matching
CPU reference (tests/am_ref.py) and `mirror_chains(case)` the literal NumPy restatement (tests/am_mirror.py).  `random_case(seed)` draws a job the
way tests/matrix_sampler_random.py does for the other samplers that carry a per-chain matrix (its tables and helpers are imported, the file is
not edited); how the job is run hangs on the dict as the attribute `run`."""
import numpy as np

import cases
import klara_jl_amd as K
import matrix_sampler_random as MR
import ram_cases as RC
import smmala_cases as SC
from klara_jl_amd import _lib as L

SWISS_X0 = SC.SWISS_X0                             # v0[:p] of the swiss examples (doc/examples/swiss/RAM.jl)
engine_kwargs = cases.engine_kwargs
quad_target, conditioned_precision = SC.quad_target, SC.conditioned_precision      # (SRC_QUAD_TENSOR: AM ignores its gradient and tensor)
target_function = RC.target_function
HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT

# logistic D = 1, 2, 3, 4, 5, 8 — E = 2, 4, 8 with (1, 3, 5) and without (2, 4, 8) padding — on layout kind 0 (40 rows) and kind 2 (the row split, >= 64 rows)
LOGIT = [f"logit_d{d}_k{k}" for d in (1, 2, 3, 4, 5, 8) for k in (0, 2)]
# every case whose covariance factors from t0 on (the literal restatement runs them too); "t0_2_d3" is the one that falls back
ALL = ["swiss_example"] + LOGIT + ["logit_d8_verbose", "quad_d3", "quad_d8", "likprior_d5", "quad_d3_c0", "quad_d3_chalf"]
FALLBACK = "t0_2_d3"


def am(d, t0, c=0.05, corescale=None, minorscale=0.01):
    """AM's fields; corescale 2.38^2 / d (Haario et al.'s scaling), a stabilising component small enough that both accepts and rejects occur"""
    return dict(sampler=L.SAMPLER_AM, am_corescale=2.38 ** 2 / d if corescale is None else corescale, am_minorscale=minorscale, am_c=c, am_t0=t0)


def make(name):
    if name == "swiss_example":               # AM(ones(4)) on the swiss regression, lambda = 100; 96 chains: 6 wavefronts of the row split
        X, y = cases.swiss_data()
        n = 96
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(3).standard_normal((n, 4))
        c = dict(target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=40, burnin=10, am_C0=np.eye(4), x0=x0, **am(4, 10, minorscale=0.04))
    elif name in LOGIT:
        d, kind = int(name[7]), int(name[-1])
        nrow = {0: 40, 2: 131}[kind]
        X, y = cases.synthetic_logit(nrow, d, seed=11 + d)
        n = 100 if kind == 0 else 131        # one wavefront and 36 lanes of the next (kind 0: 64 chains per wavefront); 8 wavefronts and 3 chains (kind 2: 16)
        x0 = 0.3 * np.random.default_rng(d).standard_normal((n, d))
        C0 = 0.09 * np.eye(d)
        if d == 3:                           # a full symmetric C0
            C0 = np.array([[0.09, 0.02, -0.01], [0.02, 0.06, 0.015], [-0.01, 0.015, 0.08]])
        c = dict(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=32, burnin=0, am_C0=C0, x0=x0, **am(d, 5 if d % 2 else 10, minorscale=0.02))
    elif name == "logit_d8_verbose":           # VanillaMCTuner(verbose=true): proposals and accepted proposals counted
        X, y = cases.synthetic_logit(70, 8, seed=19)
        n = 99
        x0 = 0.3 * np.random.default_rng(8).standard_normal((n, 8))
        c = dict(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=30, burnin=10, am_C0=0.09 * np.eye(8), verbose=True, period=6, x0=x0, **am(8, 5, minorscale=0.02))
    elif name in ("quad_d3", "quad_d8", "quad_d3_c0", "quad_d3_chalf"):
        d = int(name[6])
        P = conditioned_precision(d, 50.0, seed=d)
        n = 100
        x0 = np.random.default_rng(10 + d).standard_normal((n, d)) * 0.5
        cw = {"quad_d3_c0": 0.0, "quad_d3_chalf": 0.5}.get(name, 0.05)
        c = dict(target=quad_target(0.5, P, P), nchains=n, nsteps=36, burnin=8, am_C0=np.full(d, 0.5), x0=x0, **am(d, 10 if d == 3 else 5, c=cw, minorscale=0.05))
    elif name == "likprior_d5":                # the likelihood + prior closure form (no gradient closures: AM evaluates none)
        rng = np.random.default_rng(55)
        t = K.CustomTarget.likelihood_prior(5, cases.SRC_NN_LL, cases.SRC_NN_LP,
                                            data=np.concatenate([rng.standard_normal(5) * 2, np.linspace(0.5, 2.0, 5), np.linspace(-1, 1, 5), np.linspace(1.0, 5.0, 5)]))
        n = 97
        x0 = rng.standard_normal((n, 5))
        c = dict(target=t, nchains=n, nsteps=30, burnin=5, am_C0=np.full(5, 0.8), x0=x0, **am(5, 5, c=0.1, minorscale=0.25))
    elif name == FALLBACK:                     # t0 = 2: k - 1 = 0 wipes C0 and the first adaptive C is (x1 - x2)(x1 - x2)' / 2, of rank <= 1
        P = conditioned_precision(3, 10.0, seed=3)
        n = 100
        x0 = np.random.default_rng(23).standard_normal((n, 3)) * 0.5
        c = dict(target=quad_target(0.5, P, P), nchains=n, nsteps=40, burnin=0, am_C0=np.eye(3), x0=x0, **am(3, 2, minorscale=0.25))
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import am_ref
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    return am_ref.AmRefJob(layout=layout, want_hist=want_hist, **kw)


def mirror_chains(case, nchains=None, first=0):
    import am_mirror as AMM
    n = case["nchains"] if nchains is None else nchains
    lt = target_function(case["target"])
    C0 = np.asarray(case["am_C0"], dtype=float)
    C0 = np.diag(C0) if C0.ndim == 1 else C0
    return [AMM.AmChain(lt, case["x0"][i], case.get("seed", 20260927), i, C0, case["am_corescale"], case["am_minorscale"], case["am_c"], case["am_t0"])
            for i in range(first, first + n)]


# ---------------------------------------------------------------- random jobs (tests/test_gpu_am_random.py)
RANDOM_BASE, RANDOM_NSEEDS = 2600, 36        # rng = default_rng(RANDOM_BASE + seed): a range the other families' seeds (matrix_sampler_random.BASE) do not reach


def random_case(seed):
    """D, target kind (hence E and the row split), rows, chains, kernel MODE, monitor set, launch length, split run, shard offset as
    matrix_sampler_random.random_case draws them; t0 in 2 .. 12 (and at least three transitions before the end), c in {0, 0.05, 0.5}, the two scales and C0 (diagonal or full) drawn here"""
    rng = np.random.default_rng(RANDOM_BASE + seed)
    d = int(rng.integers(1, 9))
    n = int(rng.choice(MR.CHAINS))
    mode = int(rng.choice([0, 1, 3, 7], p=[0.4, 0.2, 0.2, 0.2]))
    monitor = 0 if mode in (3, 7) else int(rng.choice([L.MON_ACCEPT, L.MON_ACCEPT | L.MON_SUMMARIES, HIST] + ([0] if mode == 0 else [])))
    spl = 1 if mode == 7 else int(rng.choice([0, 7] + ([1] if mode in (0, 1) else [])))
    burnin = int(rng.choice([0, 3, 20])); thinning = int(rng.choice([1, 1, 2, 5]))
    nsteps = burnin + int(rng.integers(6, 41))
    c = MR.Case(nchains=n, nsteps=nsteps, burnin=burnin, thinning=thinning, seed=int(rng.integers(1, 2 ** 40)))
    t0 = min(int(rng.integers(2, 13)), nsteps - 3)                 # (at least three adaptive transitions; nsteps >= 6)
    c.update(am(d, t0, c=float(rng.choice([0.0, 0.05, 0.5])), corescale=float(rng.uniform(0.3, 3.0)), minorscale=float(rng.choice([0.01, 0.1, 1.0]))))
    C0 = rng.uniform(0.05, 0.6, d)
    if bool(rng.integers(0, 2)):                 # a full symmetric positive definite C0
        A = np.diag(np.sqrt(C0)) + np.tril(0.1 * rng.standard_normal((d, d)), -1)
        C0 = A @ A.T
    c["am_C0"] = C0
    if bool(rng.integers(0, 2)):
        kind = "logit"
        c.update(target=MR._logit(rng, seed, d), x0=0.3 * rng.standard_normal((n, d)))
    else:
        kind = str(rng.choice(["quad", "halfspace", "likprior"]))
        if kind == "quad":
            P = conditioned_precision(d, float(rng.choice([1.0, 50.0, 1e4])), seed=int(rng.integers(1, 1 << 30)))
            c.update(target=quad_target(0.5, P, P), x0=0.5 * rng.standard_normal((n, d)))
        elif kind == "halfspace":            # started inside the support; proposals leave it (log-target -inf)
            c.update(target=K.CustomTarget(d, RC.SRC_HALFSPACE), x0=np.abs(rng.standard_normal((n, d))) * 0.3 + 0.05)
        else:                                # likelihood + prior form, no gradient closures
            data = np.concatenate([rng.standard_normal(d) * 2, rng.uniform(0.5, 2.0, d), rng.uniform(-1.0, 1.0, d), rng.uniform(1.0, 5.0, d)])
            c.update(target=K.CustomTarget.likelihood_prior(d, cases.SRC_NN_LL, cases.SRC_NN_LP, data=data), x0=rng.standard_normal((n, d)))
    if mode == 0:
        c.update(verbose=True, period=int(rng.integers(3, 12)))
    c["name"] = f"random_am_{seed}_{kind}_d{d}"
    c.run = dict(monitor=monitor, steps_per_launch=spl, runs=MR._split(rng, nsteps), chain_offset=int(rng.choice([0, 1, 64, 1000])), kind=kind, mode=mode)
    return c
