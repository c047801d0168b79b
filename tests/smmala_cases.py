"""SMMALA jobs shared by tests/test_smmala_host.py, tests/test_gpu_smmala.py and tests/golden/make_golden_smmala.py.

A case is a dict of Engine keyword arguments plus "x0" (cases.engine_kwargs turns it into an Engine's); `ref_job(case)` builds the matching
CPU reference (tests/smmala_ref.py) and `mirror_chains(case)` the NumPy restatement (tests/smmala_mirror.py)."""
import numpy as np

import cases
import klara_jl_amd as K
from klara_jl_amd import _lib as L

SWISS_X0 = np.array([5.1, -0.9, 8.2, -4.5])        # v0[:p] of doc/examples/swiss/SMMALA/analytical.jl
engine_kwargs = cases.engine_kwargs

# A user-defined quadratic target with a constant metric: data = [a, P (D x D), T (D x D)]; lt = -a x'Px, grad = -2a Px, tensor = T.
# The BivariateNormal example (doc/examples/BivariateNormal/SMMALA/analytical.jl) is a = 1, P = C, T = softabs(-2C, 1000) formed on the host;
# a Gaussian N(0, P^-1) with its precision as the metric is a = 1/2, T = P.
SRC_QUAD_TENSOR = r"""
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
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    for (int i = 0; i < KLARA_D; ++i) {
        double r = 0.0;
        for (int j = 0; j < KLARA_D; ++j) r = kd_fma(data[1 + i * KLARA_D + j], x[j], r);
        g[i] = (-2.0 * data[0]) * r;
    }
}
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G)
{
    for (int k = 0; k < KLARA_D * KLARA_D; ++k) G[k] = data[1 + KLARA_D * KLARA_D + k];
}
"""


def softabs(H, a=1000.0):
    """softabs(hessian, a) of src/stats/metrics.jl:1-4: Q diag(lambda ./ tanh(a lambda)) Q'"""
    lam, Q = np.linalg.eigh(H)
    return (Q * (lam / np.tanh(a * lam))) @ Q.T


def quad_target(a, P, T):
    P, T = np.asarray(P, float), np.asarray(T, float)
    d = P.shape[0]
    return K.CustomTarget(d, SRC_QUAD_TENSOR, data=np.concatenate([[float(a)], P.ravel(), T.ravel()]))


def conditioned_precision(d, cond, seed):
    """a random SPD matrix with eigenvalues log-spaced over [1, cond]"""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    P = (Q * np.logspace(0.0, np.log10(cond), d)) @ Q.T
    return 0.5 * (P + P.T)


def _logit(d, n, seed):
    X, y = cases.synthetic_logit(n, d, seed=seed)
    return X, y


def make(name):
    if name == "swiss_example":               # SMMALA(0.02), AcceptanceRateMCTuner(0.5), lambda = 100 (swiss/SMMALA/analytical.jl:33-42)
        X, y = cases.swiss_data()
        n = 70
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(3).standard_normal((n, 4))
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=40, burnin=10, driftstep=0.02,
                 tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5, period=5, x0=x0)
    elif name in ("logit_d1", "logit_d3", "logit_d8", "logit_d3_unsplit"):
        d, nrow = {"logit_d1": (1, 90), "logit_d3": (3, 131), "logit_d8": (8, 200), "logit_d3_unsplit": (3, 40)}[name]
        X, y = _logit(d, nrow, seed=11 + d)
        n = 37
        x0 = 0.3 * np.random.default_rng(d).standard_normal((n, d))
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=30, burnin=0, driftstep=0.8, x0=x0)
    elif name == "logit_d4_thin_4099":         # burn-in and thinning, 4,099 chains (a ragged last wavefront)
        X, y = _logit(4, 200, seed=23)
        n = 4099
        x0 = 0.3 * np.random.default_rng(4).standard_normal((n, 4))
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=23, burnin=7, thinning=3, driftstep=0.5, x0=x0)
    elif name == "swiss_pooled":
        X, y = cases.swiss_data()
        n = 70
        x0 = SWISS_X0[None, :] + 0.05 * np.random.default_rng(5).standard_normal((n, 4))
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=30, burnin=12, driftstep=0.3,
                 tuner=L.TUNER_ACCEPT_RATE, tuner_mode=L.TUNE_POOLED, targetrate=0.5, period=4, x0=x0)
    elif name == "bivariate_example":         # doc/examples/BivariateNormal/SMMALA/analytical.jl: SMMALA(1.25, softabs), VanillaMCTuner
        Cm = np.linalg.inv(np.array([[1.0, 0.8], [0.8, 1.0]]))
        n = 50
        x0 = np.array([1.25, 3.11])[None, :] + 0.1 * np.random.default_rng(6).standard_normal((n, 2))
        c = dict(sampler=L.SAMPLER_SMMALA, target=quad_target(1.0, Cm, softabs(-2.0 * Cm, 1000.0)), nchains=n, nsteps=40, burnin=10,
                 driftstep=1.25, x0=x0)
    elif name in ("custom_gauss_d3", "custom_gauss_d3_rate", "custom_gauss_d6_pooled"):
        d = 6 if name.endswith("pooled") else 3
        P = conditioned_precision(d, 50.0, seed=d)
        n = 45
        x0 = np.random.default_rng(10 + d).standard_normal((n, d)) * 0.5
        c = dict(sampler=L.SAMPLER_SMMALA, target=quad_target(0.5, P, P), nchains=n, nsteps=30, burnin=8, driftstep=1.1, x0=x0)
        if name == "custom_gauss_d3_rate":
            c.update(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.6, period=5)
        if name == "custom_gauss_d6_pooled":
            c.update(tuner=L.TUNER_ACCEPT_RATE, tuner_mode=L.TUNE_POOLED, targetrate=0.6, period=4)
    elif name == "logit_d8_verbose":           # VanillaMCTuner(verbose=true): proposals counted, the step kept
        X, y = _logit(8, 70, seed=19)
        n = 40
        x0 = 0.3 * np.random.default_rng(8).standard_normal((n, 8))
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 25.0), nchains=n, nsteps=25, burnin=10, driftstep=0.6,
                 verbose=True, period=6, x0=x0)
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import smmala_ref
    kw = cases.oracle_kwargs(case, layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    return smmala_ref.SmmalaRefJob(layout=layout, want_hist=want_hist, **kw)


def mirror_chains(case, nchains=None):
    import smmala_mirror as SM
    t = case["target"]
    n = case["nchains"] if nchains is None else nchains
    if isinstance(t, K.CustomTarget):                         # SRC_QUAD_TENSOR: data = [a, P, T]
        d = t.ndims
        a, P, T = t.data[0], t.data[1:1 + d * d].reshape(d, d), t.data[1 + d * d:].reshape(d, d)
        lt, grad, tensor = (lambda x: -a * float(x @ P @ x)), (lambda x: -2.0 * a * (P @ x)), (lambda x: T)
    else:
        lt, grad = SM.M.logistic_target(t.X, t.y, t.lam)
        tensor = SM.logistic_tensor(t.X, t.lam)
    tuner = "rate" if case.get("tuner", 0) == L.TUNER_ACCEPT_RATE else "vanilla"
    return [SM.SmmalaChain(lt, grad, tensor, case["x0"][i], case.get("seed", 20260927), i, driftstep=case["driftstep"], tuner=tuner,
                           verbose=case.get("verbose", False), targetrate=case.get("targetrate"), period=case.get("period", 100),
                           nsteps=case["nsteps"], burnin=case.get("burnin", 0), thinning=case.get("thinning", 1)) for i in range(n)]
