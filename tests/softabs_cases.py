"""SMMALA jobs with the softabs transform of the metric (klara_desc.smmala_softabs), shared by tests/test_softabs_host.py,
tests/test_gpu_softabs.py and tests/golden/make_golden_softabs.py.

A case is a dict of Engine keyword arguments plus "x0", as in tests/smmala_cases.py; `ref_job(case)` builds the CPU reference
(tests/softabs_ref.py) and `mirror_chains(case)` the independent NumPy restatement (tests/smmala_mirror.SmmalaChain with
tensor = lambda x: stats.softabs(T(x), a) — LAPACK's eigh and libm's tanh, no code shared with klara_softabs.h)."""
import numpy as np

import autodiff_cases as AC
import cases
import klara_jl_amd as K
import smmala_cases as SC
from klara_jl_amd import _lib as L
from klara_jl_amd import stats

NAMES = ["bivariate_device", "banana_ad2", "doublewell_d3", "doublewell_d5", "doublewell_d8", "d1", "diag_metric_d4", "mixed_4099"]

# sum_i -(x_i^2 - 1)^2 - k/2 sum_i (x_{i+1} - x_i)^2, data = [k], written generically: the metric is minus its Hessian by nested duals
# (KLARA_USER_AUTODIFF 2), tridiagonal with the diagonal 12 x_i^2 - 4 + k deg(i) — negative eigenvalues near the origin
AD_DOUBLEWELL = r"""
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    const double k = data[0];
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const T w = x[i] * x[i] - 1.0; s = s + w * w; }
    T t = 0.0;
    for (int i = 0; i + 1 < KLARA_D; ++i) { const T d = x[i + 1] - x[i]; t = t + d * d; }
    return -s - (0.5 * k) * t;
}
"""

# N(0, I) with a diagonal tensor that has one zero entry: the rotation-free path of the Jacobi sweep and f(0) = 1 / a
SRC_DIAG_METRIC = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + x[i] * x[i];
    return -0.5 * s;
}
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    for (int i = 0; i < KLARA_D; ++i) g[i] = -x[i];
}
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G)
{
    for (int k = 0; k < KLARA_D * KLARA_D; ++k) G[k] = 0.0;
    G[0 * KLARA_D + 0] = 1.0 + x[0] * x[0];
    G[1 * KLARA_D + 1] = 0.0;
    G[2 * KLARA_D + 2] = -2.0;
    G[3 * KLARA_D + 3] = 0.5 + x[3] * x[3];
}
"""

# N(0, I) with the tensor R diag(s_k) R', data = R (D x D row-major, orthogonal), s_k = (-1)^k exp(k c(x) / (D - 1)), c(x) = ln(1e6) min(|x_0| / 3, 1):
# |x_0| = 0 gives a matrix of condition 1, |x_0| >= 3 a spread of 1e6, so the lanes of one wavefront stop after different numbers of sweeps
SRC_MIXED = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + x[i] * x[i];
    return -0.5 * s;
}
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    for (int i = 0; i < KLARA_D; ++i) g[i] = -x[i];
}
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G)
{
    double u = (x[0] < 0.0 ? -x[0] : x[0]) / 3.0;
    if (u > 1.0) u = 1.0;
    const double c = 13.815510557964274 * u;
    double s[KLARA_D];
    for (int k = 0; k < KLARA_D; ++k) { const double e = kd_exp(c * (double)k / (double)(KLARA_D - 1)); s[k] = (k & 1) ? -e : e; }
    for (int i = 0; i < KLARA_D; ++i)
        for (int j = 0; j < KLARA_D; ++j) {
            double t = 0.0;
            for (int k = 0; k < KLARA_D; ++k) t = t + (data[i * KLARA_D + k] * s[k]) * data[j * KLARA_D + k];
            G[i * KLARA_D + j] = t;
        }
}
"""


def _doublewell(d, k):
    lt = lambda x: float(-np.sum((x * x - 1.0) ** 2) - 0.5 * k * np.sum(np.diff(x) ** 2))

    def grad(x):
        g = -4.0 * x * (x * x - 1.0)
        if d > 1:
            dx = np.diff(x)
            g[:-1] += k * dx
            g[1:] -= k * dx
        return g

    def tensor(x):
        deg = np.full(d, 2.0); deg[0] = deg[-1] = 1.0
        if d == 1:
            deg[:] = 0.0
        G = np.diag(12.0 * x * x - 4.0 + k * deg)
        for i in range(d - 1):
            G[i, i + 1] = G[i + 1, i] = -k
        return G

    return lt, grad, tensor


def _banana():
    lt = lambda x: float(-(1.0 - x[0]) ** 2 / 20.0 - (x[1] - x[0] * x[0]) ** 2)
    grad = lambda x: np.array([(1.0 - x[0]) / 10.0 + 4.0 * (x[1] - x[0] * x[0]) * x[0], -2.0 * (x[1] - x[0] * x[0])])
    tensor = lambda x: np.array([[0.1 + 12.0 * x[0] * x[0] - 4.0 * x[1], -4.0 * x[0]], [-4.0 * x[0], 2.0]])
    return lt, grad, tensor


def _mixed_tensor(R):
    d = R.shape[0]

    def tensor(x):
        c = np.log(1e6) * min(abs(x[0]) / 3.0, 1.0)
        s = np.exp(c * np.arange(d) / (d - 1.0)) * np.where(np.arange(d) % 2 == 1, -1.0, 1.0)
        return (R * s) @ R.T

    return tensor


def make(name):
    """Seeds and start states are chosen on the CPU so that no accept decision of the first 8 chains is a near-tie between the C reference and the
    NumPy restatement (tests/test_softabs_host.py compares their masks)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "bivariate_device":            # doc/examples/BivariateNormal/SMMALA/analytical.jl: SMMALA(1.25, H -> softabs(H, 1000.)); the tensor is the raw -2C
        b = SC.make("bivariate_example")
        Cm = np.linalg.inv(np.array([[1.0, 0.8], [0.8, 1.0]]))
        c = {k: v for k, v in b.items() if k != "name"}
        c.update(target=SC.quad_target(1.0, Cm, -2.0 * Cm), smmala_softabs=1000.0)
        c["mirror"] = ((lambda x: -float(x @ Cm @ x)), (lambda x: -2.0 * (Cm @ x)), (lambda x: -2.0 * Cm))
    elif name == "banana_ad2":                # half of the start states lie where minus the Hessian is indefinite (x1 > x0^2 + 0.025)
        n = 64
        c = dict(sampler=L.SAMPLER_SMMALA, target=AC.target(AC.AD_BANANA, 2, order=2), nchains=n, nsteps=30, burnin=5, driftstep=0.7,
                 smmala_softabs=1.0, x0=0.7 * rng.standard_normal((n, 2)), mirror=_banana())
    elif name in ("doublewell_d3", "doublewell_d5", "doublewell_d8", "d1"):
        d = 1 if name == "d1" else int(name[-1])
        n, k = 37, 0.6
        c = dict(sampler=L.SAMPLER_SMMALA, target=AC.target(AD_DOUBLEWELL, d, np.array([k]), order=2), nchains=n, nsteps=30, burnin=8,
                 driftstep=0.5 if d == 8 else 0.9, smmala_softabs=2.0, x0=0.25 * rng.standard_normal((n, d)), mirror=_doublewell(d, k))
        if name == "doublewell_d3":
            c.update(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.6, period=5)
        elif name == "doublewell_d5":
            c.update(tuner=L.TUNER_ACCEPT_RATE, tuner_mode=L.TUNE_POOLED, targetrate=0.6, period=4)
        elif name == "doublewell_d8":
            c.update(verbose=True, period=6)
    elif name == "diag_metric_d4":
        n = 37
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.CustomTarget(4, SRC_DIAG_METRIC), nchains=n, nsteps=30, driftstep=0.8, smmala_softabs=2.0,
                 x0=0.8 * rng.standard_normal((n, 4)),
                 mirror=((lambda x: -0.5 * float(x @ x)), (lambda x: -x), (lambda x: np.diag([1.0 + x[0] * x[0], 0.0, -2.0, 0.5 + x[3] * x[3]]))),
                 # the reference's softabs is 0 / 0 at the zero eigenvalue; the device takes the limit 1 / a, and so does the mirror
                 # of this one case (the matrix is diagonal: no decomposition to restate)
                 mirror_softabs=lambda H, a: np.diag([1.0 / a if v == 0.0 else v / np.tanh(a * v) for v in np.diag(H)]))
    elif name == "mixed_4099":
        n, d = 4099, 6
        R, _ = np.linalg.qr(np.random.default_rng(61).standard_normal((d, d)))
        x0 = 0.5 * rng.standard_normal((n, d))
        x0[:, 0] = rng.uniform(0.0, 3.3, n) * rng.choice([-1.0, 1.0], n)          # neighbouring lanes: condition 1 to spread 1e6
        x0[::7, 0] = 0.0
        c = dict(sampler=L.SAMPLER_SMMALA, target=K.CustomTarget(d, SRC_MIXED, data=np.ascontiguousarray(R).ravel()), nchains=n, nsteps=23,
                 burnin=7, thinning=3, driftstep=0.9, smmala_softabs=1.0, x0=x0,
                 mirror=((lambda x: -0.5 * float(x @ x)), (lambda x: -x), _mixed_tensor(R)))
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def engine_case(case):
    """the case without what only the host side reads"""
    return {k: v for k, v in case.items() if k not in ("mirror", "mirror_softabs")}


def engine_kwargs(case, **kw):
    return cases.engine_kwargs(engine_case(case), **kw)


def ref_job(case, layout=None, chain_offset=0, nchains=None, want_hist=False):
    import softabs_ref as SR
    kw = cases.oracle_kwargs(engine_case(case), layout=layout, chain_offset=chain_offset, nchains=nchains)
    kw.pop("layout")
    a = kw.pop("smmala_softabs")
    cls = SR.AdSoftabsRefJob if case["target"].autodiff_order == 2 else SR.SoftabsRefJob
    return cls(smmala_softabs=a, layout=layout, want_hist=want_hist, **kw)


def mirror_chains(case, nchains=None):
    import smmala_mirror as SM
    n = case["nchains"] if nchains is None else nchains
    lt, grad, T = case["mirror"]
    a = case["smmala_softabs"]
    sa = case.get("mirror_softabs", stats.softabs)
    tensor = lambda x: sa(T(x), a)
    tuner = "rate" if case.get("tuner", 0) == L.TUNER_ACCEPT_RATE else "vanilla"
    return [SM.SmmalaChain(lt, grad, tensor, case["x0"][i], case.get("seed", 20260927), i, driftstep=case["driftstep"], tuner=tuner,
                           verbose=case.get("verbose", False), targetrate=case.get("targetrate"), period=case.get("period", 100),
                           nsteps=case["nsteps"], burnin=case.get("burnin", 0), thinning=case.get("thinning", 1)) for i in range(n)]
