"""AMWG jobs shared by tests/test_amwg_host.py, tests/test_gpu_amwg.py and tests/test_gpu_amwg_random.py.

A case is a dict of Engine keyword arguments plus "x0" (cases.engine_kwargs turns it into an Engine's); `ref_job(case)` builds the matching CPU
reference (tests/amwg_ref.py), `reference(name)` runs it once and keeps it for every test that compares against it, and `mirror_chains(case)` builds the
independent NumPy restatement (tests/amwg_mirror.py).  `random_case(seed)` draws a job in the manner of tests/matrix_sampler_random.py (its tables and
helpers are imported, the file is not edited); how the job is run hangs on the dict as the attribute `run`.

Sizes: chain counts 1, 70 and 200 (a short last group; several groups), 40 - 60 transitions with period 5 (eight or more tuning events), burn-in and
thinning above 1.  The reference costs one Python-level evaluation per chain, coordinate and transition, so the wide closures run on 70 chains."""
import functools

import numpy as np

import cases
import klara_jl_amd as K
import matrix_sampler_random as MR
import ram_cases as RC
import smmala_cases as SC
from klara_jl_amd import _lib as L

engine_kwargs = cases.engine_kwargs
conditioned_precision = SC.conditioned_precision
SWISS_X0 = SC.SWISS_X0
HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT

# a quadratic log-target without a gradient closure (AMWG evaluates none): data = [a, P (D x D)]; lt = -a x'Px
SRC_QUAD = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) {
        double r = 0.0;
        for (int j = 0; j < KLARA_D; ++j) r = kd_fma(data[1 + i * KLARA_D + j], x[j], r);
        s = kd_fma(x[i], r, s);
    }
    return -data[0] * s;
}
"""
# the same as a pair closure's marker would read: refused (tests/test_amwg_host.py)
SRC_PAIR = cases.SRC_PAIR_NEGDOT

CLOSURE_DIMS = (1, 5, 16, 17, 32)        # E = 2, 8, 16, 32, 32; 17 is odd and the first size whose uniform slots pass 16
LOGIT = ["swiss_d4", "logit_d3", "logit_d8", "logit_d11"]
CLOSURES = [f"{form}_d{d}" for d in CLOSURE_DIMS for form in ("quad", "likprior")]
ALL = LOGIT + CLOSURES
WALK = "quad_d5_n300"                    # quad_d5 on 300 chains: five groups of 64 (the last one short) for the four wavefronts of one workgroup


def amwg(targetrate=0.44, period=5):
    return dict(sampler=L.SAMPLER_AMWG, tuner=L.TUNER_ROBERTS_ROSENTHAL, targetrate=targetrate, period=period)


def quad_target(a, P):
    P = np.asarray(P, float)
    return K.CustomTarget(P.shape[0], SRC_QUAD, data=np.concatenate([[float(a)], P.ravel()]))


def likprior_target(d, rng):
    """the Normal-Normal model of cases.SRC_NN_LL / SRC_NN_LP in likelihood + prior form, no gradient closures"""
    data = np.concatenate([rng.standard_normal(d) * 2, rng.uniform(0.5, 2.0, d), rng.uniform(-1.0, 1.0, d), rng.uniform(1.0, 5.0, d)])
    return K.CustomTarget.likelihood_prior(d, cases.SRC_NN_LL, cases.SRC_NN_LP, data=data)


def make(name):
    if name == "swiss_d4":                     # MuvAMWG(fill(0.5, 4)) on the swiss regression (doc/examples/swiss/AMWG.jl), 200 rows: the row split, 13 wavefronts
        X, y = cases.swiss_data()
        n = 200
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(3).standard_normal((n, 4))
        c = dict(target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=45, burnin=5, thinning=2, amwg_logsigma0=np.log(np.full(4, 0.5)), x0=x0, **amwg())
    elif name in ("logit_d3", "logit_d8", "logit_d11"):
        d = int(name[7:])
        # d = 3: a padding element at E = 4, 40 rows: layout kind 0, one chain per lane; d = 8: E = 8 on the row split; d = 11: E = 16 with five padding elements
        nrow, n = {3: (40, 200), 8: (131, 70), 11: (70, 70)}[d]
        X, y = cases.synthetic_logit(nrow, d, seed=31 + d)
        x0 = 0.3 * np.random.default_rng(d).standard_normal((n, d))
        ls0 = np.log(np.linspace(0.2, 0.9, d))
        c = dict(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=40, burnin=4, thinning=3, amwg_logsigma0=ls0, x0=x0, **amwg())
    elif name in CLOSURES or name == WALK:
        form, d = name.split("_n")[0].split("_d")
        d = int(d)
        n = 300 if name == WALK else 1 if (form, d) == ("quad", 1) else 200 if d <= 5 else 70
        rng = np.random.default_rng(100 + d)
        if form == "quad":
            t = quad_target(0.5, conditioned_precision(d, 50.0, seed=d))
            x0 = 0.5 * rng.standard_normal((n, d))
        else:
            t = likprior_target(d, rng)
            x0 = rng.standard_normal((n, d))
        c = dict(target=t, nchains=n, nsteps=40 if d > 5 else 60, burnin=3, thinning=2, amwg_logsigma0=np.log(np.linspace(0.3, 1.5, d)), x0=x0,
                 **amwg(targetrate=0.44 if form == "quad" else 0.3))
    elif name == "quad_d3_p7":                 # period 7: run(7); run(13) puts a tuning event on the launch boundary
        rng = np.random.default_rng(7)
        n = 70
        c = dict(target=quad_target(0.5, conditioned_precision(3, 20.0, seed=3)), nchains=n, nsteps=20, burnin=2, thinning=2,
                 amwg_logsigma0=np.log(np.array([0.4, 1.0, 2.0])), x0=0.5 * rng.standard_normal((n, 3)), **amwg(period=7))
    elif name == "mirror_d3":                  # the job tests/test_amwg_host.py holds to the NumPy restatement: D = 3, 60 transitions, period 5
        rng = np.random.default_rng(11)
        n = 6
        c = dict(target=quad_target(0.5, conditioned_precision(3, 20.0, seed=4)), nchains=n, nsteps=60, burnin=0, thinning=1,
                 amwg_logsigma0=np.log(np.array([0.4, 1.0, 2.0])), x0=0.5 * rng.standard_normal((n, 3)), **amwg())
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import amwg_ref
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    return amwg_ref.AmwgRefJob(layout=layout, want_hist=want_hist, **kw)


def default_layout(case):
    """(kind, G, E) of an AMWG job as klara_plan.h plans it (tests/oracle_ffi.py default_layout states the same rules for MH)"""
    import oracle_ffi as O
    t = case["target"]
    return O.default_layout(t.kind, t.ndims, int(t.X.shape[0]) if isinstance(t, K.LogisticTarget) else 0, sampler=L.SAMPLER_MH)


@functools.lru_cache(maxsize=None)
def reference(name, runs=None):
    """the reference of case `name`, run once over all its transitions (in the launches `runs`) with the history on; shared, never modified"""
    case = make(name)
    job = ref_job(case, layout=default_layout(case), want_hist=True)
    assert job.set_state(case["x0"]) == 0
    for k in (runs or (case["nsteps"],)):
        assert job.run(k) == 0
    return job


def target_function(t):
    """the log-target of a case's target as a NumPy function (for tests/amwg_mirror.py)"""
    if isinstance(t, K.CustomTarget) and t.source == SRC_QUAD:
        d = t.ndims
        a, P = t.data[0], t.data[1:1 + d * d].reshape(d, d)
        return lambda x: -a * float(x @ P @ x)
    return RC.target_function(t)


def mirror_chains(case, nchains=None, first=0):
    import amwg_mirror as WM
    n = case["nchains"] if nchains is None else nchains
    lt = target_function(case["target"])
    return [WM.AmwgChain(lt, case["x0"][i], case.get("seed", 20260927), i, case["amwg_logsigma0"], case["targetrate"], case["period"])
            for i in range(first, first + n)]


# ---------------------------------------------------------------- random jobs (tests/test_gpu_amwg_random.py)
RANDOM_BASE, RANDOM_NSEEDS = 5200, 20        # rng = default_rng(RANDOM_BASE + seed): a range the other families' seeds do not reach


def random_case(seed):
    """D, target kind (hence E and the row split), rows, chains, monitor set, launch length, split run and shard offset drawn as
    matrix_sampler_random.random_case draws them; period in 2 .. 9, target rate in {0.2, 0.44, 0.7}, the start scales drawn here.  The reference costs
    chains x D x transitions evaluations in Python: the product is kept below 40,000."""
    rng = np.random.default_rng(RANDOM_BASE + seed)
    logit = bool(rng.integers(0, 2))
    d = int(rng.integers(1, 17)) if logit else int(rng.choice([1, 2, 3, 5, 8, 9, 16, 17, 24, 31, 32]))
    n = int(rng.choice(MR.CHAINS))
    monitor = int(rng.choice([0, L.MON_ACCEPT, L.MON_ACCEPT | L.MON_SUMMARIES, HIST]))
    spl = int(rng.choice([0, 1, 7]))
    burnin = int(rng.choice([0, 3, 20])); thinning = int(rng.choice([1, 1, 2, 5]))
    nsteps = burnin + int(rng.integers(6, 41))
    while n * d * nsteps > 40000 and nsteps > burnin + 6:
        nsteps -= 1
    while n * d * nsteps > 40000:
        n = max(1, n // 2)
    c = MR.Case(nchains=n, nsteps=nsteps, burnin=burnin, thinning=thinning, seed=int(rng.integers(1, 2 ** 40)))
    c.update(amwg(targetrate=float(rng.choice([0.2, 0.44, 0.7])), period=int(rng.integers(2, 10))))
    c["amwg_logsigma0"] = np.log(rng.uniform(0.1, 2.0, d))
    if logit:
        kind = "logit"
        c.update(target=MR._logit(rng, seed, d), x0=0.3 * rng.standard_normal((n, d)))
    else:
        kind = str(rng.choice(["quad", "halfspace", "likprior"]))
        if kind == "quad":
            c.update(target=quad_target(0.5, conditioned_precision(d, float(rng.choice([1.0, 50.0, 1e4])), seed=int(rng.integers(1, 1 << 30)))),
                     x0=0.5 * rng.standard_normal((n, d)))
        elif kind == "halfspace":            # started inside the support; proposals of coordinate 0 leave it (log-target -inf: a rejection)
            c.update(target=K.CustomTarget(d, RC.SRC_HALFSPACE), x0=np.abs(rng.standard_normal((n, d))) * 0.3 + 0.05)
        else:
            c.update(target=likprior_target(d, rng), x0=rng.standard_normal((n, d)))
    c["name"] = f"random_amwg_{seed}_{kind}_d{d}"
    c.run = dict(monitor=monitor, steps_per_launch=spl, runs=MR._split(rng, nsteps), chain_offset=int(rng.choice([0, 1, 64, 1000])), kind=kind)
    return c
