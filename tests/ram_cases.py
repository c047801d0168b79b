"""RAM jobs shared by tests/test_ram_host.py, tests/test_gpu_ram.py and tests/golden/make_golden_ram.py.

A case is a dict of Engine keyword arguments plus "x0" (cases.engine_kwargs turns it into an Engine's); `ref_job(case)` builds the matching
CPU reference (tests/ram_ref.py) and `mirror_chains(case)` the literal NumPy restatement (tests/ram_mirror.py)."""
import numpy as np

import cases
import klara_jl_amd as K
import smmala_cases as SC
from klara_jl_amd import _lib as L

SWISS_X0 = SC.SWISS_X0                             # v0[:p] of doc/examples/swiss/RAM.jl
engine_kwargs = cases.engine_kwargs
quad_target, conditioned_precision = SC.quad_target, SC.conditioned_precision      # (SRC_QUAD_TENSOR: RAM ignores its tensor)

# a target with bounded support: the standard normal restricted to x[0] >= 0 (a proposal outside has log-target -inf)
SRC_HALFSPACE = r"""
#ifndef INFINITY
#define INFINITY __builtin_inf()
#endif
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    if (x[0] < 0.0) return -INFINITY;
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + x[i] * x[i];
    return -0.5 * s;
}
"""

ALL = ["swiss_example", "logit_d1", "logit_d3", "logit_d8", "logit_d3_unsplit", "logit_d4_thin_4099", "gauss_d2", "gauss_d3", "gauss_d6",
       "likprior_d5", "halfspace_d2", "logit_d8_verbose"]


def make(name):
    ram = dict(sampler=L.SAMPLER_RAM, ram_targetrate=0.234, ram_gamma=0.7)
    if name == "swiss_example":               # RAM(ones(4)), lambda = 100 (doc/examples/swiss/RAM.jl)
        X, y = cases.swiss_data()
        n = 70
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(3).standard_normal((n, 4))
        c = dict(target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=40, burnin=10, ram_S0=np.eye(4), x0=x0, **ram)
    elif name in ("logit_d1", "logit_d3", "logit_d8", "logit_d3_unsplit"):
        d, nrow = {"logit_d1": (1, 90), "logit_d3": (3, 131), "logit_d8": (8, 200), "logit_d3_unsplit": (3, 40)}[name]
        X, y = cases.synthetic_logit(nrow, d, seed=11 + d)
        n = 37
        x0 = 0.3 * np.random.default_rng(d).standard_normal((n, d))
        c = dict(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=30, burnin=0, ram_S0=0.3 * np.eye(d), x0=x0, **ram)
    elif name == "logit_d4_thin_4099":         # burn-in and thinning, 4,099 chains (a ragged last wavefront, more than one group per wavefront)
        X, y = cases.synthetic_logit(200, 4, seed=23)
        n = 4099
        x0 = 0.3 * np.random.default_rng(4).standard_normal((n, 4))
        c = dict(target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=23, burnin=7, thinning=3, ram_S0=0.3 * np.eye(4), x0=x0, **ram)
    elif name in ("gauss_d2", "gauss_d3", "gauss_d6"):
        d = int(name[-1])
        P = conditioned_precision(d, 50.0, seed=d)
        n = 45
        x0 = np.random.default_rng(10 + d).standard_normal((n, d)) * 0.5
        S0 = np.array([[0.9, 0.0, 0.0], [0.3, 0.6, 0.0], [-0.2, 0.25, 0.8]]) if d == 3 else 0.7 * np.eye(d)
        c = dict(target=quad_target(0.5, P, P), nchains=n, nsteps=30, burnin=8, ram_S0=S0, x0=x0, **ram)
    elif name == "likprior_d5":                # the likelihood + prior closure form (no gradient closures: RAM evaluates none)
        rng = np.random.default_rng(55)
        t = K.CustomTarget.likelihood_prior(5, cases.SRC_NN_LL, cases.SRC_NN_LP,
                                            data=np.concatenate([rng.standard_normal(5) * 2, np.linspace(0.5, 2.0, 5), np.linspace(-1, 1, 5), np.linspace(1.0, 5.0, 5)]))
        n = 41
        x0 = rng.standard_normal((n, 5))
        c = dict(target=t, nchains=n, nsteps=30, burnin=5, ram_S0=np.full(5, 0.8), x0=x0, ram_targetrate=0.3, ram_gamma=0.6, sampler=L.SAMPLER_RAM)
    elif name == "halfspace_d2":               # started inside the support; proposals leave it
        n = 39
        x0 = np.abs(np.random.default_rng(21).standard_normal((n, 2))) * 0.3 + 0.05
        c = dict(target=K.CustomTarget(2, SRC_HALFSPACE), nchains=n, nsteps=30, burnin=0, ram_S0=np.eye(2), x0=x0, **ram)
    elif name == "logit_d8_verbose":           # VanillaMCTuner(verbose=true): proposals and accepted proposals counted
        X, y = cases.synthetic_logit(70, 8, seed=19)
        n = 40
        x0 = 0.3 * np.random.default_rng(8).standard_normal((n, 8))
        c = dict(target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=25, burnin=10, ram_S0=0.3 * np.eye(8), verbose=True, period=6, x0=x0, **ram)
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import ram_ref
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    return ram_ref.RamRefJob(layout=layout, want_hist=want_hist, **kw)


def target_function(t):
    """the log-target of a case's target as a NumPy function (for tests/ram_mirror.py)"""
    import numpy_mirror as M
    if isinstance(t, K.LogisticTarget):
        return M.logistic_target(t.X, t.y, t.lam)[0]
    d = t.ndims
    if t.source == SRC_HALFSPACE:
        return lambda x: -np.inf if x[0] < 0 else -0.5 * float(x @ x)
    if t.has_parts:                                           # cases.SRC_NN_LL / SRC_NN_LP: data = (x, s, mu0, s0)
        xd, s, m0, s0 = t.data.reshape(4, d)
        c = d * 1.8378770664093453
        return lambda mu: -0.5 * (float(((xd - mu) ** 2 / s).sum()) + c + float(np.log(s).sum())) - 0.5 * (float(((mu - m0) ** 2 / s0).sum()) + c + float(np.log(s0).sum()))
    a, P = t.data[0], t.data[1:1 + d * d].reshape(d, d)       # SRC_QUAD_TENSOR: data = [a, P, T]
    return lambda x: -a * float(x @ P @ x)


def mirror_chains(case, nchains=None):
    import ram_mirror as RM
    n = case["nchains"] if nchains is None else nchains
    lt = target_function(case["target"])
    S0 = np.asarray(case["ram_S0"], dtype=float)
    S0 = np.diag(S0) if S0.ndim == 1 else S0
    return [RM.RamChain(lt, case["x0"][i], case.get("seed", 20260927), i, S0, case["ram_targetrate"], case["ram_gamma"]) for i in range(n)]
