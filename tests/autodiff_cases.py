"""Forward-mode autodiff sources (KLARA_USER_AUTODIFF, klara.jl_amd/csrc/klara_autodiff.h) shared by tests/test_autodiff_host.py and
tests/test_gpu_autodiff.py, with the analytic gradients and Hessians (numpy.longdouble) the host build is held against.

A source here is the text BEHIND the `#define KLARA_USER_AUTODIFF n` line: `K.CustomTarget.autodiff` prepends the defines."""
import numpy as np

import cases
import klara_jl_amd as K
from klara_jl_amd import _lib as L

LD = np.longdouble
EPS = np.finfo(np.float64).eps

# the largest |host - truth| / (eps * sum |terms|) the host build shows on the 50 points of tests/test_autodiff_host.py test_host_build_against_the_truth (measured with g++ on x86-64;
# by A1 / A2 the device computes the same bits, so these are the device's errors too).  The test's cap is 4 x these.
MEASURED = {"negdot_d2": 0.0, "negdot_d3": 0.0, "negdot_d9": 0.0, "negdot_d32": 0.0, "negdot_d33": 0.0, "negdot_d100": 0.0, "negdot_d520": 0.0,
            "banana": 1.394, "logit_swiss": 2.313, "logit_d9": 0.726, "quartic_d33": 1.055, "quartic_d100": 1.058, "nn_d5": 0.850, "erf_d3": 2.575,
            "gauss_d3": 0.787,
            # tests/test_closure_sweep_host.py: the coupled likelihood + prior closure of tests/closure_sweep.py at D = 105, hand-written gll + glp and its autodiff form
            "quartic_parts_hand_d105": 1.102, "quartic_parts_d105": 1.079}
MEASURED_ORDER2 = {"logit_swiss": 5.333, "gauss_d3": 0.0}

AD_NEGDOT = r"""
/* cases.SRC_NEGDOT without its gradient: plogtarget(z) = -dot(z, z) */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + x[i] * x[i];
    return 0.0 - s;
}
"""

AD_BANANA = r"""
/* cases.SRC_BANANA's log-target: lt = -(1 - x0)^2 / 20 - (x1 - x0^2)^2 */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    const T a = 1.0 - x[0], b = x[1] - x[0] * x[0];
    return -(a * a) / 20.0 - b * b;
}
"""

AD_LOGIT = r"""
/* the text of cases.SRC_LOGIT's log-target (doc/examples/swiss/MALA/forwarddiff.jl); data = [X (n x D row-major), y (n), lambda] */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& p, int D, const double* data, long long ndata)
{
    const int n = (int)((ndata - 1) / (KLARA_D + 1));
    const double* X = data; const double* y = data + (long long)n * KLARA_D; const double lambda = data[ndata - 1];
    T dotxy = 0.0, slog = 0.0;
    for (int r = 0; r < n; ++r) {
        T xp = 0.0;
        for (int e = 0; e < KLARA_D; ++e) xp = kd_fma(X[r * KLARA_D + e], p[e], xp);
        dotxy = dotxy + xp * y[r];
        T sp, lg;
        kd_softplus_logistic_rows(xp, &sp, &lg);
        slog = slog + sp;
    }
    T dotpp = 0.0;
    for (int e = 0; e < KLARA_D; ++e) dotpp = dotpp + p[e] * p[e];
    return (dotxy - slog) + -0.5 * (dotpp / lambda + (double)KLARA_D * kd_log(2.0 * 3.141592653589793 * lambda));
}
"""

AD_QUARTIC_CHAIN = r"""
/* cases.SRC_QUARTIC_CHAIN's log-target: lt = -sum_i (x_i^2 / 2 + c x_i^4) - k/2 sum_i (x_{i+1} - x_i)^2, data = [c, k] */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    const double c = data[0], k = data[1];
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const T q = x[i] * x[i]; s = s + (0.5 * q + c * (q * q)); }
    T t = 0.0;
    for (int i = 0; i + 1 < KLARA_D; ++i) { const T d = x[i + 1] - x[i]; t = t + d * d; }
    return -s - (0.5 * k) * t;
}
"""

AD_NN_LL = r"""
/* cases.SRC_NN_LL: x | mu ~ N(mu, diag(s)); data = (x[D], s[D], mu0[D], s0[D]) */
template <class T, class V>
KLARA_USER_FN T klara_user_loglikelihood_ad(const V& mu, int D, const double* data, long long ndata)
{
    const double* x = data; const double* s = data + KLARA_D;
    T q = 0.0; double ld = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const T d = x[i] - mu[i]; q = q + d * d / s[i]; ld = ld + kd_log(s[i]); }
    return -0.5 * (q + (double)KLARA_D * 1.8378770664093453 + ld);
}
"""
AD_NN_LP = r"""
template <class T, class V>
KLARA_USER_FN T klara_user_logprior_ad(const V& mu, int D, const double* data, long long ndata)
{
    const double* m0 = data + 2 * KLARA_D; const double* s0 = data + 3 * KLARA_D;
    T q = 0.0; double ld = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const T d = mu[i] - m0[i]; q = q + d * d / s0[i]; ld = ld + kd_log(s0[i]); }
    return -0.5 * (q + (double)KLARA_D * 1.8378770664093453 + ld);
}
"""

AD_ERF = r"""
/* lt = sum_i log((1 + erf(x_i)) / 2): kd_erf, kd_log and a division by a dual */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) s = s + kd_log(1.0 / (2.0 / (1.0 + kd_erf(x[i]))));
    return s;
}
"""

AD_GAUSS = r"""
/* lt = -a x'Px (smmala_cases.SRC_QUAD_TENSOR's log-target), data = [a, P (D x D)]: the metric of order 2 is 2a P */
template <class T, class V>
KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata)
{
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) {
        T r = 0.0;
        for (int j = 0; j < KLARA_D; ++j) r = kd_fma(data[1 + i * KLARA_D + j], x[j], r);
        s = kd_fma(x[i], r, s);
    }
    return -data[0] * s;
}
"""

AD_PAIR = r"""
#define KLARA_USER_PAIR_TARGET 1
KLARA_USER_FN double klara_user_pair(double x0, double x1, int pair, int D, const double* data, long long ndata, double* g0, double* g1)
{
    *g0 = -2.0 * x0; *g1 = -2.0 * x1;
    return -(x0 * x0) - x1 * x1;
}
"""

AD_NO_FUNCTION = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata) { return -x[0] * x[0]; }
"""


def marked(text, order=1, chunksize=0, parts=False):
    """the source as the library takes it (what K.CustomTarget.autodiff prepends)"""
    head = f"#define KLARA_USER_AUTODIFF {int(order)}\n"
    if chunksize:
        head += f"#define KLARA_USER_AUTODIFF_CHUNK {int(chunksize)}\n"
    if parts:
        head += "#define KLARA_USER_LIKELIHOOD_PRIOR 1\n"
    return head + text


# ---- analytic derivatives in numpy.longdouble: (gradient, sum of the absolute terms of each element's sum[, Hessian, sum of absolute terms])
def _logit_parts(X, y, lam, p):
    X, y, p = X.astype(LD), y.astype(LD), p.astype(LD)
    xp = X @ p
    lg = 1 / (1 + np.exp(-xp))
    return X, y, p, lg


def truth_negdot(p, data=None):
    p = p.astype(LD)
    return -2 * p, np.abs(2 * p)


def truth_banana(p, data=None):
    x0, x1 = p.astype(LD)
    a, b = 1 - x0, x1 - x0 * x0
    g = np.array([a / 10 + 4 * b * x0, -2 * b])
    mag = np.array([abs(a) / 10 + 4 * abs(b * x0), 2 * abs(x1) + 2 * x0 * x0])
    return g, mag


def truth_logit(p, data):
    d = p.size
    n = (data.size - 1) // (d + 1)
    X, y, p, lg = _logit_parts(data[:n * d].reshape(n, d), data[n * d:n * d + n], data[-1], p)
    lam = LD(data[-1])
    g = X.T @ (y - lg) - p / lam
    mag = np.abs(X).T @ (np.abs(y) + lg) + np.abs(p) / lam
    return g, mag


def truth_logit_neg_hessian(p, data):
    d = p.size
    n = (data.size - 1) // (d + 1)
    X, y, p, lg = _logit_parts(data[:n * d].reshape(n, d), data[n * d:n * d + n], data[-1], p)
    w = lg * (1 - lg)
    H = (X * w[:, None]).T @ X + np.eye(d, dtype=LD) / LD(data[-1])
    mag = (np.abs(X) * w[:, None]).T @ np.abs(X) + np.eye(d, dtype=LD) / LD(data[-1])
    return H, mag


def truth_quartic(p, data):
    x = p.astype(LD)
    c, k = LD(data[0]), LD(data[1])
    g = -(x + 4 * c * x ** 3)
    mag = np.abs(x) + 4 * c * np.abs(x) ** 3
    dn = np.zeros_like(x); dn[:-1] = x[1:] - x[:-1]
    up = np.zeros_like(x); up[1:] = x[1:] - x[:-1]
    g = g + k * dn - k * up
    an = np.zeros_like(x); an[:-1] = np.abs(x[1:]) + np.abs(x[:-1])
    au = np.zeros_like(x); au[1:] = np.abs(x[1:]) + np.abs(x[:-1])
    return g, mag + k * (an + au)


def truth_nn(p, data):
    d = p.size
    mu = p.astype(LD)
    x, s, m0, s0 = (data[i * d:(i + 1) * d].astype(LD) for i in range(4))
    g = (x - mu) / s - (mu - m0) / s0
    mag = (np.abs(x) + np.abs(mu)) / s + (np.abs(mu) + np.abs(m0)) / s0
    return g, mag


def truth_erf(p, data=None):
    from math import erf, erfc
    x = p.astype(LD)
    onep = np.array([LD(erfc(-float(v))) for v in x])      # 1 + erf(x) without the cancellation (the bound is relative: double precision is enough here)
    e = np.array([LD(erf(float(v))) for v in x])
    g = (2 / np.sqrt(LD(np.pi))) * np.exp(-x * x) / onep
    return g, np.abs(g) * (1 + np.abs(e)) / onep           # (the terms of the sum 1 + erf(x) that the slope is divided by)


def truth_gauss(p, data):
    d = p.size
    a, P = LD(data[0]), data[1:1 + d * d].reshape(d, d).astype(LD)
    x = p.astype(LD)
    g = -a * (P @ x + P.T @ x)
    mag = a * (np.abs(P) @ np.abs(x) + np.abs(P.T) @ np.abs(x))
    return g, mag


def truth_gauss_neg_hessian(p, data):
    d = p.size
    a, P = LD(data[0]), data[1:1 + d * d].reshape(d, d).astype(LD)
    return a * (P + P.T), a * (np.abs(P) + np.abs(P.T))


def swiss_block():
    X, y = cases.swiss_data()
    return np.concatenate([X.ravel(), y, [100.0]])


def logit_block(n=60, d=9, lam=25.0):
    X, y = cases.synthetic_logit(n, d, seed=5)
    return np.concatenate([X.ravel(), y, [lam]])


def nn_block(d=5):
    rng = np.random.default_rng(7)
    return np.concatenate([rng.standard_normal(d), rng.uniform(0.5, 2.0, d), rng.standard_normal(d), rng.uniform(0.5, 3.0, d)])


def gauss_block(d=3):
    import smmala_cases as SC
    return np.concatenate([[0.5], SC.conditioned_precision(d, 50.0, seed=d).ravel()])


# (name, text, D, data, parts form, truth) — every source of the issue's table at every dimension it lists
def host_sources():
    out = [(f"negdot_d{d}", AD_NEGDOT, d, None, False, truth_negdot) for d in (2, 3, 9, 32, 33, 100, 520)]
    out += [("banana", AD_BANANA, 2, None, False, truth_banana),
            ("logit_swiss", AD_LOGIT, 4, swiss_block(), False, truth_logit),
            ("logit_d9", AD_LOGIT, 9, logit_block(), False, truth_logit),
            ("quartic_d33", AD_QUARTIC_CHAIN, 33, np.array([0.1, 0.5]), False, truth_quartic),
            ("quartic_d100", AD_QUARTIC_CHAIN, 100, np.array([0.1, 0.5]), False, truth_quartic),
            ("nn_d5", AD_NN_LL + AD_NN_LP, 5, nn_block(5), True, truth_nn),
            ("erf_d3", AD_ERF, 3, None, False, truth_erf),
            ("gauss_d3", AD_GAUSS, 3, gauss_block(3), False, truth_gauss)]
    return out


# order 2: (name, text, D, data, truth of minus the Hessian)
def host_sources_order2():
    return [("logit_swiss", AD_LOGIT, 4, swiss_block(), truth_logit_neg_hessian),
            ("gauss_d3", AD_GAUSS, 3, gauss_block(3), truth_gauss_neg_hessian)]


# ---- GPU jobs: Engine keyword arguments + "x0", as tests/smmala_cases.py sizes them
def target(text, d, data=None, order=1, chunksize=0, parts=False):
    return K.CustomTarget(d, marked(text, order, chunksize, parts), data)


def make(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("mala_negdot_d"):
        d = int(name[len("mala_negdot_d"):])
        n, steps = (8, 6) if d == 520 else (37, 30)
        c = dict(sampler=L.SAMPLER_MALA, target=target(AD_NEGDOT, d), nchains=n, nsteps=steps, driftstep=0.9 / d ** (1.0 / 3.0),
                 x0=0.7 * rng.standard_normal((n, d)))
    elif name == "mala_banana":
        n = 41
        c = dict(sampler=L.SAMPLER_MALA, target=target(AD_BANANA, 2), nchains=n, nsteps=30, driftstep=0.4, x0=0.5 * rng.standard_normal((n, 2)))
    elif name in ("mala_logit_swiss_rate", "mala_logit_swiss_pooled"):
        import smmala_cases as SC
        n = 70
        c = dict(sampler=L.SAMPLER_MALA, target=target(AD_LOGIT, 4, swiss_block()), nchains=n, nsteps=40, burnin=10, driftstep=0.1,
                 tuner=L.TUNER_ACCEPT_RATE, targetrate=0.574, period=5, x0=SC.SWISS_X0[None, :] + 0.05 * rng.standard_normal((n, 4)))
        if name.endswith("pooled"):
            c.update(tuner_mode=L.TUNE_POOLED)
    elif name in ("hmc_quartic_d33", "hmc_quartic_d100"):
        d = int(name[len("hmc_quartic_d"):])
        n = 37
        c = dict(sampler=L.SAMPLER_HMC, target=target(AD_QUARTIC_CHAIN, d, np.array([0.1, 0.5])), nchains=n, nsteps=20, leapstep=0.12, nleaps=5,
                 x0=0.5 * rng.standard_normal((n, d)))
    elif name == "hmc_erf":
        n = 45
        c = dict(sampler=L.SAMPLER_HMC, target=target(AD_ERF, 3), nchains=n, nsteps=30, leapstep=0.9, nleaps=5, x0=0.5 + 0.5 * rng.standard_normal((n, 3)))
    elif name == "hmc_logit_d9_da":
        n = 40
        c = dict(sampler=L.SAMPLER_HMC, target=target(AD_LOGIT, 9, logit_block()), nchains=n, nsteps=30, burnin=15, leapstep=0.1, nleaps=5,
                 tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.65, da_nadapt=15, x0=0.3 * rng.standard_normal((n, 9)))
    elif name == "mala_nn_parts":
        n, d = 37, 5
        c = dict(sampler=L.SAMPLER_MALA, target=target(AD_NN_LL + AD_NN_LP, d, nn_block(d), parts=True), nchains=n, nsteps=30, driftstep=0.9,
                 x0=rng.standard_normal((n, d)))
    elif name in ("mh_banana", "slice_banana"):
        n = 37
        c = dict(target=target(AD_BANANA, 2), nchains=n, nsteps=30, x0=0.5 * rng.standard_normal((n, 2)))
        c.update(dict(sampler=L.SAMPLER_MH, mh_sigma=np.array([0.8, 0.8])) if name == "mh_banana" else
                 dict(sampler=L.SAMPLER_SLICE, slice_widths=np.array([1.0, 1.0])))
    elif name == "smmala_logit_swiss":        # doc/examples/swiss/SMMALA/forwarddiff.jl: SMMALA(0.02), AcceptanceRateMCTuner(0.5)
        import smmala_cases as SC
        n = 70
        c = dict(sampler=L.SAMPLER_SMMALA, target=target(AD_LOGIT, 4, swiss_block(), order=2), nchains=n, nsteps=40, burnin=10, driftstep=0.02,
                 tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5, period=5, x0=SC.SWISS_X0[None, :] + 0.05 * rng.standard_normal((n, 4)))
    elif name == "smmala_gauss_d3":
        n = 45
        c = dict(sampler=L.SAMPLER_SMMALA, target=target(AD_GAUSS, 3, gauss_block(3), order=2), nchains=n, nsteps=30, burnin=8, driftstep=1.1,
                 x0=0.5 * rng.standard_normal((n, 3)))
    else:
        raise KeyError(name)
    c["name"] = name
    return c
