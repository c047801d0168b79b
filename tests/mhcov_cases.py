"""MH(Σ) jobs shared by tests/test_mhcov_host.py and tests/test_gpu_mhcov.py.

A case is a dict of Engine keyword arguments plus "x0" (cases.engine_kwargs turns it into an Engine's); `ref_job(case)` builds the matching CPU
reference (tests/mhcov_ref.py), `reference(name, chain_offset)` runs it once on the case's 130 chains and keeps it for every test that compares against it
— chains are independent and chain c draws from stream offset + c, so a 70-chain job is the first 70 chains of the same reference — and
`mirror_chains(case)` builds the independent NumPy restatement (tests/mhcov_mirror.py).

Sizes: 130 chains (two full wavefronts and a partial one at a chain per lane; 70: one and a partial one), 40 transitions, burn-in 5, thinning 2.  Factors
are a positive diagonal plus 0.1 tril(randn), as tests/ram_cases.py builds RAM's, times 0.6 / sqrt(D) so that the chains of every D both accept and
reject."""
import functools

import numpy as np

import amwg_cases as WC
import cases
import klara_jl_amd as K
import ram_cases as RC
import smmala_cases as SC
from klara_jl_amd import _lib as L

engine_kwargs = cases.engine_kwargs
conditioned_precision = SC.conditioned_precision
SWISS_X0 = SC.SWISS_X0
SRC_QUAD = WC.SRC_QUAD                      # lt = -a x'Px without a gradient closure (MH evaluates none); data = [a, P]
quad_target = WC.quad_target
likprior_target = WC.likprior_target
HIST = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT
SEED = 20260927

CLOSURE_DIMS = (2, 3, 5, 8, 9, 16, 17, 32)   # E = 2, 4, 8, 8, 16, 16, 32, 32: every E with D < E and with D = E
CLOSURES = [f"quad_d{d}" for d in CLOSURE_DIMS]
LOGIT = ["swiss_d4", "logit_d11"]
ALL = CLOSURES + LOGIT
NCHAINS, NSTEPS, BURNIN, THINNING = 130, 40, 5, 2


def full_factor(d, seed, scale=None):
    """a positive diagonal plus 0.1 tril(randn) below it, times `scale` (0.6 / sqrt(D) by default)"""
    rng = np.random.default_rng(seed)
    f = np.diag(rng.uniform(0.5, 1.5, d)) + 0.1 * np.tril(rng.standard_normal((d, d)), -1)
    return (0.6 / np.sqrt(d) if scale is None else scale) * f


def mhcov(factor):
    return dict(sampler=L.SAMPLER_MH_COV, mh_factor=np.asarray(factor, dtype=np.float64))


def make(name, nchains=NCHAINS):
    n = nchains
    common = dict(nchains=n, nsteps=NSTEPS, burnin=BURNIN, thinning=THINNING)
    if name == "swiss_d4":                     # the swiss regression, 200 rows: layout kind 2 (the rows split over four lanes), E = 4
        X, y = cases.swiss_data()
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(3).standard_normal((n, 4))
        c = dict(target=K.LogisticTarget(X, y, 100.0), x0=x0, **mhcov(full_factor(4, 41, scale=0.25)), **common)
    elif name in ("logit_d11", "logit_d9"):    # 70 rows / 40 rows: E = 16 with padding elements; 40 rows: layout kind 0, a chain per lane
        d = int(name[7:])
        X, y = cases.synthetic_logit({11: 70, 9: 40}[d], d, seed=31 + d)
        x0 = 0.3 * np.random.default_rng(d).standard_normal((n, d))
        c = dict(target=K.LogisticTarget(X, y, 25.0), x0=x0, **mhcov(full_factor(d, 50 + d, scale=0.15)), **common)
    elif name.startswith("quad_d"):
        d = int(name[6:])
        rng = np.random.default_rng(100 + d)
        c = dict(target=quad_target(0.5, conditioned_precision(d, 50.0, seed=d)), x0=0.5 * rng.standard_normal((n, d)), **mhcov(full_factor(d, 200 + d)), **common)
    elif name.startswith("likprior_d"):
        d = int(name[10:])
        rng = np.random.default_rng(300 + d)
        c = dict(target=likprior_target(d, rng), x0=rng.standard_normal((n, d)), **mhcov(full_factor(d, 400 + d, scale=1.2 / np.sqrt(d))), **common)
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def as_mh(case, sigma):
    """the MH(σ::Vector) job of the same target, start and range"""
    c = {k: v for k, v in case.items() if k != "mh_factor"}
    c.update(sampler=L.SAMPLER_MH, mh_sigma=np.asarray(sigma, dtype=np.float64))
    return c


def with_factor(case, factor):
    c = dict(case)
    c.update(mhcov(factor))
    return c


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import mhcov_ref
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    return mhcov_ref.MhCovRefJob(layout=layout, want_hist=want_hist, **kw)


def default_layout(case):
    """(kind, G, E) of an MH(Σ) job as klara_plan.h plans it: MH's (tests/oracle_ffi.py default_layout)"""
    import oracle_ffi as O
    t = case["target"]
    return O.default_layout(t.kind, t.ndims, int(t.X.shape[0]) if isinstance(t, K.LogisticTarget) else 0, sampler=L.SAMPLER_MH)


@functools.lru_cache(maxsize=None)
def reference(name, chain_offset=0):
    """the reference of case `name` at `chain_offset`, all NCHAINS chains run once over all transitions with the history on; shared, never modified"""
    case = make(name)
    job = ref_job(case, layout=default_layout(case), chain_offset=chain_offset, want_hist=True)
    assert job.set_state(case["x0"]) == 0
    assert job.run(case["nsteps"]) == 0
    return job


def target_function(t):
    """the log-target of a case's target as a NumPy function (for tests/mhcov_mirror.py)"""
    return WC.target_function(t)


def mirror_chains(case, nchains=None, chain_offset=0):
    import mhcov_mirror as CM
    n = case["nchains"] if nchains is None else nchains
    lt = target_function(case["target"])
    return [CM.MhCovChain(lt, case["x0"][i], case.get("seed", SEED), chain_offset + i, case["mh_factor"]) for i in range(n)]


def correlated_gaussian(d, rho):
    """(target, Σ): N(0, Σ) with unit variances and every correlation rho, as the closure smmala_cases.SRC_QUAD_TENSOR (a = 1/2, P = Σ^-1; its tensor is
    not read by MH)"""
    S = np.full((d, d), float(rho)) + (1.0 - float(rho)) * np.eye(d)
    P = np.linalg.inv(S)
    P = 0.5 * (P + P.T)
    return SC.quad_target(0.5, P, P), S
