"""Thin object wrapper over the C ABI (one Engine = one klara_handle = N chains on one GPU).

Host buffers are NumPy arrays; nothing here computes a transition — every call forwards to
libklara_hip.so (see include/klara_hip.h for the reference lines each entry point replaces).
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


# ------------------------------------------------------------------ target families
@dataclass
class GaussDiagTarget:
    """lt = c - sum_i w_i (x_i - mu_i)^2 (KLARA_TARGET_GAUSS_DIAG).

    README.md:23 `plogtarget(z) = -dot(z, z)` is `GaussDiagTarget.negdot(D)`;
    MvNormal(mu, sigma) closures of test/BasicContMuvParameter.jl:39-56,88-100 are `mvnormal(mu, sigma)`.
    """
    ndims: int
    w: Optional[np.ndarray] = None
    mu: Optional[np.ndarray] = None
    const: float = 0.0
    kind = L.TARGET_GAUSS_DIAG

    @classmethod
    def negdot(cls, ndims: int) -> "GaussDiagTarget":
        return cls(int(ndims))

    @classmethod
    def mvnormal(cls, mu, sigma) -> "GaussDiagTarget":
        mu = _f64(mu).ravel()
        sigma = np.broadcast_to(_f64(sigma).ravel(), mu.shape).astype(np.float64)
        d = mu.size
        const = -0.5 * d * np.log(2.0 * np.pi) - float(np.sum(np.log(sigma)))
        return cls(d, w=1.0 / (2.0 * sigma * sigma), mu=mu.copy(), const=float(const))


@dataclass
class GaussDenseTarget:
    """lt = c - 1/2 (x-mu)' P (x-mu) with a dense D x D precision matrix (KLARA_TARGET_GAUSS_DENSE, FP64 MFMA); mu = None is 0."""
    precision: np.ndarray
    const: float = 0.0
    mu: Optional[np.ndarray] = None
    kind = L.TARGET_GAUSS_DENSE

    def __post_init__(self):
        self.precision = _f64(self.precision)
        if self.precision.ndim != 2 or self.precision.shape[0] != self.precision.shape[1]:
            raise ValueError("precision must be square")
        if self.mu is not None:
            self.mu = _f64(self.mu)
            if self.mu.shape != (self.precision.shape[0],):
                raise ValueError("mu must have one entry per dimension")

    @property
    def ndims(self) -> int:
        return int(self.precision.shape[0])

    @classmethod
    def compound_symmetric(cls, ndims: int, rho: float = 0.5) -> "GaussDenseTarget":
        """Sigma = (1-rho) I + rho 11' ; closed-form inverse (SURVEY §8(d) cfg 3)."""
        d = int(ndims)
        prec = (np.eye(d) - (rho / (1.0 - rho + d * rho)) * np.ones((d, d))) / (1.0 - rho)
        return cls(prec)


@dataclass
class LogisticTarget:
    """Bayesian logistic regression, N(0, lambda I) prior (doc/examples/swiss/MALA/analytical.jl:11-18)."""
    X: np.ndarray
    y: np.ndarray
    lam: float = 100.0
    kind = L.TARGET_LOGISTIC

    def __post_init__(self):
        self.X = _f64(self.X)
        self.y = _f64(self.y).ravel()
        if self.X.ndim != 2 or self.X.shape[0] != self.y.size:
            raise ValueError("X must be (ndata, D) and y (ndata,)")

    @property
    def ndims(self) -> int:
        return int(self.X.shape[1])


@dataclass
class CustomTarget:
    """User-defined target: the device form of `BasicContMuvParameter(:p, logtarget=f, gradlogtarget=g)`
    (BasicContMuvParameter.jl:174-201,264-279).  `source` is C text defining

        KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata);
        KLARA_USER_FN void   klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g);

        KLARA_USER_FN void   klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G);

    (the gradient only for MALA / HMC / SMMALA; the tensor — the metric of `tensorlogtarget=`, a row-major symmetric D x D matrix — only for
    SMMALA, D <= 8, in this plain whole-vector form); it is compiled for gfx950 when the job is created (include/klara_hip.h,
    KLARA_TARGET_CUSTOM).  `data` is an optional read-only block of doubles handed to every function."""
    ndims: int
    source: str
    data: Optional[np.ndarray] = None
    kind = L.TARGET_CUSTOM

    def __post_init__(self):
        self.ndims = int(self.ndims)
        if self.data is not None:
            self.data = _f64(self.data).ravel()

    @classmethod
    def likelihood_prior(cls, ndims: int, loglikelihood: str, logprior: str, gradloglikelihood: str = "", gradlogprior: str = "",
                         data=None) -> "CustomTarget":
        """The likelihood + prior form of `BasicContMuvParameter(:p, loglikelihood=..., logprior=..., gradloglikelihood=...,
        gradlogprior=...)` (BasicContMuvParameter.jl:174-201): each argument is C text defining klara_user_loglikelihood /
        klara_user_logprior / klara_user_gradloglikelihood / klara_user_gradlogprior; the library composes
        logtarget = loglikelihood + logprior and gradlogtarget = gradloglikelihood + gradlogprior (klara_custom_compose.h)."""
        src = "#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + "\n".join(t for t in (loglikelihood, logprior, gradloglikelihood, gradlogprior) if t)
        return cls(ndims, src, data)

    @classmethod
    def pairwise(cls, ndims: int, pair_source: str, data=None) -> "CustomTarget":
        """Closures of a target that is a SUM OF TERMS OF ONE OR TWO NEIGHBOURING COORDINATES, one element pair at a time:
        `pair_source` is C text defining

            KLARA_USER_FN double klara_user_pair(double x0, double x1, int pair, int D, const double* data, long long ndata,
                                                 double* g0, double* g1);

        with logtarget(x) = sum over pairs P of klara_user_pair(x[2P], x[2P+1], P, ...) and (*g0, *g1) the pair's two partial
        derivatives (for the half pair of an odd D, x1 is 0 and *g1 is ignored).  Such a job runs on the few-lanes-per-chain
        kernels of the diagonal Gaussian (layout kind 3: 8 / 16 / 32 / 64 lanes per chain, 17 <= D <= 1024; MH, MALA, HMC with every tuner
        and monitor) instead of one chain per lane — the form for large D (include/klara_hip.h, KLARA_USER_PAIR_TARGET).  Below 17 dimensions, and
        the library sums the pairs' terms itself and runs the whole-vector form (D <= 1024); the slice sampler runs on them too (round 6: a probe compares the pair's own term)."""
        return cls(ndims, "#define KLARA_USER_PAIR_TARGET 1\n" + pair_source, data)

    @classmethod
    def autodiff(cls, ndims: int, source: str, data=None, order: int = 1, chunksize: int = 0) -> "CustomTarget":
        """Forward-mode automatic differentiation, the device form of `diffopts=DiffOptions(mode=:forward)` (src/autodiff/forward.jl,
        BasicContMuvParameter.jl:627-694): `source` defines no gradient, only the log-target, generic in its scalar type,

            template <class T, class V>
            KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata);

        where x[i] yields a T (a source in the likelihood + prior form — `#define KLARA_USER_LIKELIHOOD_PRIOR 1` — defines klara_user_loglikelihood_ad and
        klara_user_logprior_ad of the same shape instead).  The functions may use + - * / and comparisons between T and double, sqrt, fabs, kd_fma,
        kd_exp, kd_log, kd_erf and kd_softplus_logistic_rows.  `order=2` also forms the metric of the SMMALA sampler as minus the Hessian (D <= 8, not
        the likelihood + prior form); `chunksize` is DiffOptions.chunksize: the directions per sweep, 0 for the library's choice.  This prepends
        `#define KLARA_USER_AUTODIFF order` (and KLARA_USER_AUTODIFF_CHUNK) to the source (include/klara_hip.h)."""
        if int(order) not in (1, 2):
            raise ValueError("order must be 1 or 2")
        if int(chunksize) < 0:
            raise ValueError("chunksize can not be negative")
        head = f"#define KLARA_USER_AUTODIFF {int(order)}\n"
        if int(chunksize) > 0:
            head += f"#define KLARA_USER_AUTODIFF_CHUNK {int(chunksize)}\n"
        return cls(ndims, head + source, data)

    @property
    def autodiff_order(self) -> int:
        """value of the source's KLARA_USER_AUTODIFF marker (0: a source with hand-written gradients)"""
        m = re.search(r"KLARA_USER_AUTODIFF[ \t]+(\d)", self.source)
        return 0 if m is None else (2 if m.group(1) == "2" else 1)

    @property
    def has_parts(self) -> bool:
        return "KLARA_USER_LIKELIHOOD_PRIOR" in self.source

    @property
    def is_pairwise(self) -> bool:
        return "KLARA_USER_PAIR_TARGET" in self.source

    @property
    def has_tensor(self) -> bool:
        """the source defines klara_user_tensorlogtarget, or asks for second-order autodiff (what the SMMALA sampler needs)"""
        return "klara_user_tensorlogtarget" in self.source or self.autodiff_order == 2

    def check(self, sampler: int) -> None:
        """Compile only (no GPU needed); raises KlaraError with the compiler's log on failure (for SMMALA also when the source has no
        klara_user_tensorlogtarget, or is a likelihood + prior / pair-closure source, or D > 8)."""
        if int(sampler) == L.SAMPLER_SMMALA and not self.has_tensor:
            raise L.KlaraError(L.ERR_COMPILE, "klara_check_custom_target: the SMMALA sampler needs klara_user_tensorlogtarget")
        L.check(L.load().klara_check_custom_target(self.source.encode(), int(sampler), self.ndims), "klara_check_custom_target")

    def check_softabs(self) -> None:
        """check(SAMPLER_SMMALA) for the kernels with the softabs transform of the metric (Engine(..., smmala_softabs=a), SMMALA(h, SoftAbs(a)))"""
        if not self.has_tensor:
            raise L.KlaraError(L.ERR_COMPILE, "klara_check_custom_target_softabs: the SMMALA sampler needs klara_user_tensorlogtarget")
        L.check(L.load().klara_check_custom_target_softabs(self.source.encode(), self.ndims), "klara_check_custom_target_softabs")


@dataclass
class HierNormalTarget:
    """Hierarchical normal growth-curve model (BUGS "Rats"; BASELINE cfg 5, data/rats/*.csv).

    theta = (alpha_1, beta_1, ..., alpha_R, beta_R, alpha_c, beta_c, log sigma_c, log sigma_alpha, log sigma_beta),
    D = 2R + 5.  Builder-defined: the reference ships only the data (doc/examples/rats/Gibbs.jl is a stub).
    """
    Y: np.ndarray                 # (R, T) observations
    xc: np.ndarray                # (T,) centred covariate (age - 22 for the rats)
    prior_prec: float = 1e-4      # alpha_c, beta_c ~ N(0, 1/prior_prec)
    gamma_a: float = 1e-3         # precisions ~ Gamma(a, b)
    gamma_b: float = 1e-3
    kind = L.TARGET_HIER_NORMAL

    def __post_init__(self):
        self.Y = _f64(self.Y)
        self.xc = _f64(self.xc).ravel()
        if self.Y.ndim != 2 or self.Y.shape[1] != self.xc.size:
            raise ValueError("Y must be (R, T) and xc (T,)")

    @property
    def ndims(self) -> int:
        return 2 * int(self.Y.shape[0]) + 5

    def least_squares_start(self) -> np.ndarray:
        """Per-unit OLS fit -> a reasonable initial theta (SURVEY §8(d) cfg 5: 'least-squares fit + jitter')."""
        r, t = self.Y.shape
        sxx = float(self.xc @ self.xc)
        xbar = float(self.xc.mean())
        beta = ((self.Y - self.Y.mean(axis=1, keepdims=True)) @ (self.xc - xbar)) / float((self.xc - xbar) @ (self.xc - xbar))
        alpha = self.Y.mean(axis=1) - beta * xbar
        resid = self.Y - alpha[:, None] - beta[:, None] * self.xc[None, :]
        th = np.empty(2 * r + 5)
        th[0:2 * r:2] = alpha
        th[1:2 * r:2] = beta
        th[2 * r] = alpha.mean(); th[2 * r + 1] = beta.mean()
        th[2 * r + 2] = np.log(resid.std(ddof=2) + 1e-12)
        th[2 * r + 3] = np.log(alpha.std(ddof=1) + 1e-12)
        th[2 * r + 4] = np.log(beta.std(ddof=1) + 1e-12)
        del sxx, t
        return th


# ------------------------------------------------------------------ pooled marginal histograms
class Marginals:
    """Marginals(nbins, lo, hi): per dimension, `nbins` (1 .. 1024) equal bins over [lo, hi) plus an underflow and an overflow slot; lo and hi are scalars
    (every dimension the same) or D values, finite, lo < hi.  Handed to Engine / BasicMCJob as marginals=: the saved samples of all chains are then
    counted after every launch (Engine.pooled_histogram, K.pooled_hist, K.pooled_quantiles) — no stored history."""

    def __init__(self, nbins: int, lo, hi):
        self.nbins = int(nbins)
        self.lo, self.hi = lo, hi

    def bounds(self, ndims: int):
        lo = _f64(np.broadcast_to(_f64(self.lo).ravel(), (ndims,)))
        hi = _f64(np.broadcast_to(_f64(self.hi).ravel(), (ndims,)))
        return lo, hi

    def edges(self, ndims: int) -> np.ndarray:
        lo, hi = self.bounds(ndims)
        return lo[:, None] + np.arange(self.nbins + 1)[None, :] * ((hi - lo) / self.nbins)[:, None]


def histogram_quantiles(counts, nbins: int, lo, hi, probs) -> np.ndarray:
    """klara_histogram_quantiles: (D, len(probs)) quantiles from (D, nbins + 2) counts — the library's one statement of the rule (host code, no device)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    D = counts.shape[0]
    if counts.ndim != 2 or counts.shape[1] != int(nbins) + 2:
        raise ValueError(f"counts must be (D, nbins + 2), not {counts.shape}")
    lo, hi = Marginals(nbins, lo, hi).bounds(D)
    p = _f64(np.atleast_1d(probs).ravel())
    out = np.empty((D, p.size))
    L.check(L.load().klara_histogram_quantiles(counts.ctypes.data, D, int(nbins), lo.ctypes.data, hi.ctypes.data, p.size, p.ctypes.data, out.ctypes.data),
            "klara_histogram_quantiles")
    return out


# ------------------------------------------------------------------ derived quantities
class Derived:
    """Derived(nout, source, data=None, marginals=None): a function of the state, summarised on the device.  `source` is C text that defines

        KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K);

    (x: one saved sample, data: the closure's own block, out: K = nout <= 64 doubles; KLARA_D and KLARA_K are defined; the kd_* functions of detmath.h may
    be called; a pure function of its arguments).  Handed to Engine / BasicMCJob as derived=: after every launch the closure is evaluated on every saved
    sample of every chain and its outputs and their squares are summed per chain (Engine.derived_sums, derived_moments, derived_rhat; K.derived_mean,
    K.derived_var, K.derived_rhat) — no stored history.  `marginals`: a Marginals over the nout outputs, for their pooled histograms and quantiles
    (Engine.derived_histogram, K.derived_quantiles).  check_derived compiles a text without a GPU."""

    def __init__(self, nout: int, source: str, data=None, marginals=None):
        self.nout = int(nout)
        self.source = str(source)
        self.data = None if data is None else _f64(np.asarray(data, dtype=np.float64).ravel())
        self.marginals = None if marginals is None else marginals if isinstance(marginals, Marginals) else Marginals(*marginals)


def check_derived(source: str, ndims: int, nout: int) -> bool:
    """klara_check_derived: compile a derived-quantity closure for gfx950 as klara_create would (no handle, no GPU); raises KlaraError with the
    compiler's log when it does not compile."""
    L.check(L.load().klara_check_derived(str(source).encode(), int(ndims), int(nout)), "klara_check_derived")
    return True


# ------------------------------------------------------------------ engine
class Engine:
    def __init__(self, *, sampler: int, target, nchains: int, nsteps: int, burnin: int = 0, thinning: int = 1,
                 mh_sigma=None, driftstep: float = 1.0, leapstep: float = 0.1, nleaps: int = 10,
                 slice_widths=None, slice_stepout: bool = True,
                 tuner: int = L.TUNER_VANILLA, tuner_mode: int = L.TUNE_PER_CHAIN, targetrate: float = 0.0,
                 score_k: float = 7.0, tuner_score: int = 0, period: int = 100, verbose: bool = False,
                 da_nadapt: int = 0, da_eps0bar: float = 1.0, da_h0bar: float = 0.0, da_gamma: float = 0.05,
                 da_t0: int = 10, da_kappa: float = 0.75,
                 seed: int = 20260927, chain_offset: int = 0, device: int = 0, monitor: int = 0,
                 steps_per_launch: int = 0, stream: int = 0, nstreams: int = 0, bm_batchlen: int = 0, hist_ring_cols: int = 0,
                 acov_maxlag: int = 0, sparse_moves: int = 0, smmala_softabs: float = 0.0,
                 ram_S0=None, ram_targetrate: float = 0.0, ram_gamma: float = 0.0, marginals=None, derived=None,
                 am_C0=None, am_corescale: float = 0.0, am_minorscale: float = 0.0, am_c: float = 0.0, am_t0: int = 0,
                 amwg_logsigma0=None, mh_factor=None):
        self._lib = L.load()
        self.target = target
        self.ndims = int(target.ndims)
        self.nchains = int(nchains)
        self.nsteps, self.burnin, self.thinning = int(nsteps), int(burnin), int(thinning)
        self.sampler = int(sampler)
        self.monitor = int(monitor)
        d = L.KlaraDesc()
        d.struct_size = C.sizeof(L.KlaraDesc)
        d.abi_version = getattr(L.load(), "_klara_abi_override", L.KLARA_ABI_VERSION)   # (an older build under KLARA_ALLOW_ABI_MISMATCH=1: its own version)
        d.sampler, d.target, d.tuner, d.tuner_mode = int(sampler), int(target.kind), int(tuner), int(tuner_mode)
        d.nchains, d.chain_offset, d.ndims, d.device = self.nchains, int(chain_offset), self.ndims, int(device)
        keep = []  # keep host arrays alive until klara_create returns
        if mh_sigma is not None:
            a = _f64(np.broadcast_to(_f64(mh_sigma).ravel(), (self.ndims,))); keep.append(a); d.mh_sigma = _ptr(a)
        if slice_widths is not None:
            a = _f64(np.broadcast_to(_f64(slice_widths).ravel(), (self.ndims,))); keep.append(a); d.slice_widths = _ptr(a)
        d.driftstep, d.leapstep, d.nleaps, d.slice_stepout = float(driftstep), float(leapstep), int(nleaps), int(bool(slice_stepout))
        d.targetrate, d.score_k, d.period, d.verbose = float(targetrate), float(score_k), int(period), int(bool(verbose))
        d.nsteps, d.burnin, d.thinning = self.nsteps, self.burnin, self.thinning
        d.da_nadapt, d.da_eps0bar, d.da_h0bar = int(da_nadapt), float(da_eps0bar), float(da_h0bar)
        d.da_gamma, d.da_kappa, d.da_t0 = float(da_gamma), float(da_kappa), int(da_t0)
        d.tuner_score = int(tuner_score)
        if isinstance(target, GaussDiagTarget):
            if target.w is not None:
                a = _f64(target.w, (self.ndims,)); keep.append(a); d.gauss_w = _ptr(a)
            if target.mu is not None:
                a = _f64(target.mu, (self.ndims,)); keep.append(a); d.gauss_mu = _ptr(a)
            d.gauss_const = float(target.const)
        elif isinstance(target, GaussDenseTarget):
            a = _f64(target.precision); keep.append(a); d.gauss_prec = _ptr(a)
            if target.mu is not None:
                a = _f64(target.mu, (self.ndims,)); keep.append(a); d.gauss_mu = _ptr(a)
            d.gauss_const = float(target.const)
        elif isinstance(target, LogisticTarget):
            a = _f64(target.X); keep.append(a); d.logit_X = _ptr(a)
            b = _f64(target.y); keep.append(b); d.logit_y = _ptr(b)
            d.logit_ndata, d.logit_lambda = int(target.X.shape[0]), float(target.lam)
        elif isinstance(target, HierNormalTarget):
            a = _f64(target.Y); keep.append(a); d.hier_Y = _ptr(a)
            b = _f64(target.xc); keep.append(b); d.hier_xc = _ptr(b)
            d.hier_nunits, d.hier_ntimes = int(target.Y.shape[0]), int(target.Y.shape[1])
            d.hier_prior_prec, d.hier_gamma_a, d.hier_gamma_b = float(target.prior_prec), float(target.gamma_a), float(target.gamma_b)
        elif isinstance(target, CustomTarget):
            src = target.source.encode(); keep.append(src); d.custom_src = src
            if target.data is not None and target.data.size:
                a = _f64(target.data); keep.append(a); d.custom_data = _ptr(a); d.custom_ndata = int(a.size)
        else:
            raise TypeError(f"unknown target family {type(target).__name__}")
        d.seed, d.monitor, d.steps_per_launch = int(seed), self.monitor, int(steps_per_launch)
        d.nstreams = int(nstreams)
        d.bm_batchlen = int(bm_batchlen)
        d.hist_ring_cols, d.acov_maxlag, d.sparse_moves = int(hist_ring_cols), int(acov_maxlag), int(sparse_moves)
        # SMMALA(driftstep, H -> softabs(H, a)): the a of the metric's transform, 0 = none (klara_desc.smmala_softabs)
        if float(smmala_softabs) > 0.0 and isinstance(target, LogisticTarget):
            raise ValueError("softabs is not applied to the logistic target's metric: X' diag(r (1 - r)) X + I / lambda is positive definite by construction")
        d.smmala_softabs = float(smmala_softabs)
        # RAM(S0; targetrate, gamma): the initial factor (D x D, its lower triangle is read; a vector is its diagonal), RAM.jl:94-111
        if ram_S0 is not None:
            a = _f64(ram_S0)
            a = _f64(np.diag(a.ravel())) if a.ndim < 2 else a
            if a.shape != (self.ndims, self.ndims):
                raise ValueError(f"ram_S0 must be {self.ndims} x {self.ndims} (or its diagonal), not {a.shape}")
            keep.append(a); d.ram_S0 = _ptr(a)
        d.ram_targetrate, d.ram_gamma = float(ram_targetrate), float(ram_gamma)
        # AM(C0; corescale, minorscale, c, t0): the initial covariance (D x D symmetric, its upper triangle is read; a vector is its diagonal), AM.jl:131-154
        if am_C0 is not None:
            a = _f64(am_C0)
            a = _f64(np.diag(a.ravel())) if a.ndim < 2 else a
            if a.shape != (self.ndims, self.ndims):
                raise ValueError(f"am_C0 must be {self.ndims} x {self.ndims} (or its diagonal), not {a.shape}")
            keep.append(a); d.am_C0 = _ptr(a)
        d.am_corescale, d.am_minorscale, d.am_c, d.am_t0 = float(am_corescale), float(am_minorscale), float(am_c), int(am_t0)
        # MuvAMWG(sigma): the D initial log proposal scales (klara_desc.amwg_logsigma0; a number serves every coordinate), AMWG.jl:139-151
        if amwg_logsigma0 is not None:
            a = _f64(np.broadcast_to(_f64(amwg_logsigma0).ravel(), (self.ndims,))); keep.append(a); d.amwg_logsigma0 = _ptr(a)
        # MH(Σ): the D x D lower factor of the proposal covariance (klara_desc.mh_factor), MH.jl:63-66
        if mh_factor is not None:
            a = _f64(mh_factor)
            if a.shape != (self.ndims, self.ndims):
                raise ValueError(f"mh_factor must be {self.ndims} x {self.ndims}, not {a.shape}")
            keep.append(a); d.mh_factor = _ptr(a)
        # pooled marginal histograms (klara_desc.marg_lo / marg_hi / marg_nbins): a Marginals, or (nbins, lo, hi)
        self.marginals = None
        if marginals is not None:
            m = marginals if isinstance(marginals, Marginals) else Marginals(*marginals)
            lo, hi = m.bounds(self.ndims)
            keep.extend((lo, hi)); d.marg_lo, d.marg_hi, d.marg_nbins = _ptr(lo), _ptr(hi), m.nbins
            self.marginals = Marginals(m.nbins, lo.copy(), hi.copy())
        # derived quantities (klara_desc.derived_*): a Derived
        self.derived = None
        if derived is not None:
            if not isinstance(derived, Derived):
                raise TypeError("derived= takes a Derived(nout, source, data=None, marginals=None)")
            src = derived.source.encode(); keep.append(src); d.derived_src, d.derived_nout = src, derived.nout
            if derived.data is not None and derived.data.size:
                keep.append(derived.data); d.derived_data, d.derived_ndata = _ptr(derived.data), int(derived.data.size)
            dm = None
            if derived.marginals is not None:
                lo, hi = derived.marginals.bounds(derived.nout)
                keep.extend((lo, hi)); d.derived_lo, d.derived_hi, d.derived_nbins = _ptr(lo), _ptr(hi), derived.marginals.nbins
                dm = Marginals(derived.marginals.nbins, lo.copy(), hi.copy())
            self.derived = Derived(derived.nout, derived.source, derived.data, dm)
        d.stream = C.c_void_p(int(stream)) if stream else None
        self._h = C.c_void_p()
        L.check(self._lib.klara_create(C.byref(d), C.byref(self._h)), "klara_create")
        del keep

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            h, self._h = self._h, C.c_void_p()
            L.check(self._lib.klara_destroy(h), "klara_destroy")     # (KLARA_DEBUG_CANARY=1: fails when a kernel wrote outside an array)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state
    def set_state(self, x):
        x = _f64(x, (self.nchains, self.ndims))
        L.check(self._lib.klara_set_state(self._h, x.ctypes.data), "klara_set_state")

    def init_state_normal(self):
        L.check(self._lib.klara_init_state_normal(self._h), "klara_init_state_normal")

    def reset(self, x=None):
        if x is None:
            L.check(self._lib.klara_reset(self._h, None), "klara_reset")
        else:
            x = _f64(x, (self.nchains, self.ndims))
            L.check(self._lib.klara_reset(self._h, x.ctypes.data), "klara_reset")

    def stream_key(self):
        """(Philox key the job currently draws from, klara_reset calls so far) — include/klara_hip.h klara_reset."""
        k, e = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_stream_key(self._h, C.byref(k), C.byref(e)), "klara_stream_key")
        return int(k.value), int(e.value)

    def run(self, nsteps: int):
        L.check(self._lib.klara_run(self._h, int(nsteps)), "klara_run")

    def run_async(self, nsteps: int):
        L.check(self._lib.klara_run_async(self._h, int(nsteps)), "klara_run_async")

    def synchronize(self):
        L.check(self._lib.klara_synchronize(self._h), "klara_synchronize")

    # -- read-back
    def state(self):
        x = np.empty((self.nchains, self.ndims)); lt = np.empty(self.nchains); g = np.empty((self.nchains, self.ndims))
        L.check(self._lib.klara_get_state(self._h, x.ctypes.data, lt.ctypes.data, g.ctypes.data), "klara_get_state")
        return x, lt, g

    def accept_mask(self) -> np.ndarray:
        n = C.c_int64(0)
        L.check(self._lib.klara_get_accept_mask(self._h, None, 0, C.byref(n)), "klara_get_accept_mask")
        m = np.empty((n.value, self.nchains), dtype=np.uint8)
        L.check(self._lib.klara_get_accept_mask(self._h, m.ctypes.data, n.value, C.byref(n)), "klara_get_accept_mask")
        return m

    def accept_rows(self, first_step: int, nsteps: int) -> np.ndarray:
        """accept diagnostics of the transitions [first_step, first_step + nsteps) only: (nsteps, nchains) bytes"""
        m = np.empty((int(nsteps), self.nchains), dtype=np.uint8)
        L.check(self._lib.klara_get_accept_rows(self._h, int(first_step), int(nsteps), m.ctypes.data), "klara_get_accept_rows")
        return m

    def accept_counts(self):
        a = np.empty(self.nchains, dtype=np.uint64); n = C.c_uint64(0)
        L.check(self._lib.klara_get_accept_counts(self._h, a.ctypes.data, C.byref(n)), "klara_get_accept_counts")
        return a, int(n.value)

    def chain_sums(self):
        s = np.empty((self.nchains, self.ndims)); q = np.empty((self.nchains, self.ndims)); n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_sums(self._h, s.ctypes.data, q.ctypes.data, C.byref(n)), "klara_get_chain_sums")
        return s, q, int(n.value)

    def pooled_summaries(self, with_sums: bool = True):
        s = np.empty(self.ndims) if with_sums else None
        q = np.empty(self.ndims) if with_sums else None
        na, nt, ns = C.c_uint64(0), C.c_uint64(0), C.c_int64(0)
        L.check(self._lib.klara_get_pooled_summaries(
            self._h, s.ctypes.data if with_sums else None, q.ctypes.data if with_sums else None,
            C.byref(na), C.byref(nt), C.byref(ns)), "klara_get_pooled_summaries")
        return s, q, int(na.value), int(nt.value), int(ns.value)

    def pooled_moments(self, comm=None):
        """(mean[D], M2[D], nsamples, naccept, ntransitions, nchains) over this handle's chains — or, with a klara_comm handle,
        over every rank's — formed on the device without the cancellation of sumsq/n - mean^2 (klara_gather_moments)."""
        mean = np.empty(self.ndims); m2 = np.empty(self.ndims)
        ns, na, nt, nc = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_gather_moments(self._h, comm, mean.ctypes.data, m2.ctypes.data, C.byref(ns), C.byref(na), C.byref(nt),
                                               C.byref(nc)), "klara_gather_moments")
        return mean, m2, int(ns.value), int(na.value), int(nt.value), int(nc.value)

    def pooled_covariance(self, comm=None):
        """(mean[D], M[D, D], nsamples, nchains) over this handle's chains — or, with a klara_comm handle, over every rank's: M = sum (x - mean)(x - mean)'
        over all chains and saved steps, accumulated while sampling (monitor bit MON_COVARIANCE, klara_gather_covariance); cov = M / (nsamples - 1)."""
        mean = np.empty(self.ndims); m2 = np.empty((self.ndims, self.ndims))
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_gather_covariance(self._h, comm, mean.ctypes.data, m2.ctypes.data, C.byref(ns), C.byref(nc)), "klara_gather_covariance")
        return mean, m2, int(ns.value), int(nc.value)

    def pooled_histogram(self, comm=None):
        """(counts[D, nbins + 2] uint64, edges[D, nbins + 1], nsamples, nchains) over this handle's chains — or, with a klara_comm handle, over every
        rank's: the saved samples of every dimension counted into the job's `marginals` bins, columns 0 and nbins + 1 the underflow and the overflow
        (klara_gather_histogram).  edges[d, k] = lo[d] + k (hi[d] - lo[d]) / nbins is documentation: the index formula is the contract."""
        if self.marginals is None:
            raise ValueError("the job was built without marginals=")
        m = self.marginals
        counts = np.zeros((self.ndims, m.nbins + 2), dtype=np.uint64)
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_gather_histogram(self._h, comm, counts.ctypes.data, C.byref(ns), C.byref(nc)), "klara_gather_histogram")
        return counts, m.edges(self.ndims), int(ns.value), int(nc.value)

    # -- derived quantities (a job built with derived=)
    def _derived(self):
        if self.derived is None:
            raise ValueError("the job was built without derived=")
        return self.derived

    def derived_sums(self):
        """(sum[nchains, K], sumsq[nchains, K], nsaved): every chain's running sums of the closure's outputs and of their squares (klara_get_derived_sums)."""
        K = self._derived().nout
        s = np.empty((self.nchains, K)); q = np.empty((self.nchains, K)); n = C.c_int64(0)
        L.check(self._lib.klara_get_derived_sums(self._h, s.ctypes.data, q.ctypes.data, C.byref(n)), "klara_get_derived_sums")
        return s, q, int(n.value)

    def derived_moments(self, comm=None):
        """(mean[K], M2[K], nsamples, nchains) of the closure's outputs over this handle's chains — or, with a klara_comm handle, over every rank's: the
        reduction of pooled_moments on the derived sums (klara_gather_derived_moments); var = M2 / nsamples."""
        K = self._derived().nout
        mean = np.empty(K); m2 = np.empty(K)
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_gather_derived_moments(self._h, comm, mean.ctypes.data, m2.ctypes.data, C.byref(ns), C.byref(nc)), "klara_gather_derived_moments")
        return mean, m2, int(ns.value), int(nc.value)

    def derived_rhat(self, comm=None):
        """The Gelman–Rubin diagnostic of the closure's outputs (klara_gather_derived_rhat, the plain form of rhat()): dict of rhat[K], mean[K], wsum[K],
        bsum[K], nchains and nper."""
        K = self._derived().nout
        out = {k: np.empty(K) for k in ("rhat", "mean", "wsum", "bsum")}
        nc, npu = C.c_uint64(0), C.c_int64(0)
        L.check(self._lib.klara_gather_derived_rhat(self._h, comm, out["rhat"].ctypes.data, out["mean"].ctypes.data, out["wsum"].ctypes.data,
                                                    out["bsum"].ctypes.data, C.byref(nc), C.byref(npu)), "klara_gather_derived_rhat")
        out["nchains"], out["nper"] = int(nc.value), int(npu.value)
        return out

    def derived_histogram(self, comm=None):
        """(counts[K, nbins + 2] uint64, edges[K, nbins + 1], nsamples, nchains): the pooled histograms of the closure's outputs, as pooled_histogram's of
        the coordinates (klara_gather_derived_histogram); needs Derived(..., marginals=)."""
        dq = self._derived()
        if dq.marginals is None:
            raise ValueError("the job's Derived was built without marginals=")
        m = dq.marginals
        counts = np.zeros((dq.nout, m.nbins + 2), dtype=np.uint64)
        ns, nc = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.klara_gather_derived_histogram(self._h, comm, counts.ctypes.data, C.byref(ns), C.byref(nc)), "klara_gather_derived_histogram")
        return counts, m.edges(dq.nout), int(ns.value), int(nc.value)

    def rhat(self, split: bool = False, comm=None):
        """The Gelman–Rubin diagnostic over this handle's chains — or, with a klara_comm handle, over every rank's (klara_gather_rhat): dict of rhat[D],
        mean[D] (the mean of the chain means), wsum[D] (sum of the chains' M2), bsum[D] (sum of (chain mean - mean)^2), nchains and nper (the units the
        formulas ran on).  split=False works from the running sums (MON_SUMMARIES); split=True is the split form from the stored history (MON_HISTORY,
        no ring, at least 4 saved steps): nchains is then the number of half-chains and nper their length."""
        out = {k: np.empty(self.ndims) for k in ("rhat", "mean", "wsum", "bsum")}
        nc, npu = C.c_uint64(0), C.c_int64(0)
        L.check(self._lib.klara_gather_rhat(self._h, comm, 1 if split else 0, out["rhat"].ctypes.data, out["mean"].ctypes.data, out["wsum"].ctypes.data,
                                            out["bsum"].ctypes.data, C.byref(nc), C.byref(npu)), "klara_gather_rhat")
        out["nchains"], out["nper"] = int(nc.value), int(npu.value)
        return out

    def pooled_ess(self, mode: str = "streamed", maxlag=None, comm=None):
        """The pooled (multi-chain) effective sample size over this handle's chains — or, with a klara_comm handle, over every rank's (klara_gather_ess):
        ess = m n / tau from R-hat's within / between variances and the across-chain sums of the chains' lagged cross-products, Geyer's monotone pair sum.
        mode "streamed": from the autocovariances kept while sampling (acov_maxlag > 0; maxlag must be None); "history": from the stored history
        (MON_HISTORY, no ring) with window maxlag (1..127; None: min(127, n - 1)); "split": the same over every chain's two halves (at least 8 saved
        steps).  Dict of ess[D], tau[D], rho[D, L + 1], mean[D], wsum[D], bsum[D], pairs[D], window_exhausted[D] (the window ended before Geyer's rule
        did: ess is an overestimate there), nunits, nper, lags (= L)."""
        modes = {"streamed": L.ESS_STREAMED, "history": L.ESS_HISTORY, "split": L.ESS_SPLIT}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}")
        if mode == "streamed" and maxlag is not None:
            raise ValueError("the streamed mode's window is the job's acov_maxlag: maxlag must be None")
        out = {k: np.empty(self.ndims) for k in ("ess", "tau", "mean", "wsum", "bsum")}
        rho = np.empty((self.ndims, L.ESS_MAXLAG + 1)); pairs = np.zeros(self.ndims, dtype=np.int32)
        nu, npu, lg = C.c_uint64(0), C.c_int64(0), C.c_int32(0)
        L.check(self._lib.klara_gather_ess(self._h, comm, modes[mode], 0 if maxlag is None else int(maxlag), out["ess"].ctypes.data, out["tau"].ctypes.data,
                                           rho.ctypes.data, out["mean"].ctypes.data, out["wsum"].ctypes.data, out["bsum"].ctypes.data, pairs.ctypes.data,
                                           C.byref(nu), C.byref(npu), C.byref(lg)), "klara_gather_ess")
        lags = int(lg.value)
        out["rho"] = rho.ravel()[: self.ndims * (lags + 1)].reshape(self.ndims, lags + 1).copy()
        out["pairs"] = pairs
        out["window_exhausted"] = pairs == (max(lags - 1, 0) // 2 + 1)
        out["nunits"], out["nper"], out["lags"] = int(nu.value), int(npu.value), lags
        return out

    def chain(self, local_chain: int) -> np.ndarray:
        """One chain's saved values in Klara's NState layout: (ndims, nsaved), column-major."""
        n = C.c_int64(0)
        L.check(self._lib.klara_get_chain(self._h, int(local_chain), None, 0, C.byref(n)), "klara_get_chain")
        v = np.empty((self.ndims, n.value), order="F")
        L.check(self._lib.klara_get_chain(self._h, int(local_chain), v.ctypes.data, n.value, C.byref(n)), "klara_get_chain")
        return v

    def chain_fields(self, local_chain: int, logtarget: bool = True, gradlogtarget: bool = False):
        """logtarget (n,) and/or gradlogtarget (ndims, n) of one chain over the saved steps (NState fields)."""
        n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_fields(self._h, int(local_chain), None, None, 0, C.byref(n)), "klara_get_chain_fields")
        lt = np.empty(n.value) if logtarget else None
        g = np.empty((self.ndims, n.value), order="F") if gradlogtarget else None
        L.check(self._lib.klara_get_chain_fields(self._h, int(local_chain), lt.ctypes.data if logtarget else None,
                                                 g.ctypes.data if gradlogtarget else None, n.value, C.byref(n)),
                "klara_get_chain_fields")
        return lt, g

    def chain_likelihood_prior(self, local_chain: int):
        """(loglikelihood (n,), logprior (n,)) of one chain over the saved steps — a likelihood + prior user target monitored with
        MON_HIST_LLLP (:monitor => [:loglikelihood, :logprior])."""
        n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_likelihood_prior(self._h, int(local_chain), None, None, 0, C.byref(n)), "klara_get_chain_likelihood_prior")
        ll = np.empty(n.value); lp = np.empty(n.value)
        L.check(self._lib.klara_get_chain_likelihood_prior(self._h, int(local_chain), ll.ctypes.data, lp.ctypes.data, n.value, C.byref(n)),
                "klara_get_chain_likelihood_prior")
        return ll, lp

    def chain_mcvar(self, batchlen: int = 100, maxlag: int = 0, want=("iid", "bm", "imse")):
        """(mcvar_iid, mcvar_bm, mcvar_imse), each (nchains, ndims) or None when not in `want`, from the on-device history
        (mcvar.jl); an estimator that is not asked for is not computed (the IMSE pass costs O(n x stopping lag) per series)."""
        out = [np.empty((self.nchains, self.ndims)) if k in want else None for k in ("iid", "bm", "imse")]
        L.check(self._lib.klara_get_chain_mcvar(self._h, int(batchlen), int(maxlag), *[None if a is None else a.ctypes.data for a in out]),
                "klara_get_chain_mcvar")
        return tuple(out)

    def chain_acov_mcvar(self, want=("imse", "ipse")):
        """(mcvar_imse, mcvar_ipse, nsamples), each (nchains, ndims) or None: Geyer's estimators with maxlag = acov_maxlag from the
        autocovariances accumulated while sampling — no stored history (mcvar.jl:75-105, 137-158)."""
        out = [np.empty((self.nchains, self.ndims)) if k in want else None for k in ("imse", "ipse")]
        n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_acov_mcvar(self._h, *[None if a is None else a.ctypes.data for a in out], C.byref(n)),
                "klara_get_chain_acov_mcvar")
        return out[0], out[1], int(n.value)

    def chain_mcvar_ipse(self, maxlag: int = 0) -> np.ndarray:
        """mcvar(:ipse, maxlag) of every (chain, dimension) series over the stored history (mcvar.jl:137-158)."""
        out = np.empty((self.nchains, self.ndims))
        L.check(self._lib.klara_get_chain_mcvar_ipse(self._h, int(maxlag), out.ctypes.data), "klara_get_chain_mcvar_ipse")
        return out

    def zv_nterms(self, order: int) -> int:
        """Control variates of lzv (order 1: ndims) / qzv (order 2: ndims (ndims + 3) / 2, zv.jl:52)."""
        if order not in (L.ZV_LINEAR, L.ZV_QUADRATIC):
            raise ValueError(f"order must be 1 (lzv) or 2 (qzv), not {order!r}")
        return self.ndims if order == L.ZV_LINEAR else self.ndims * (self.ndims + 3) // 2

    def chain_zv(self, order: int, pooled: bool = False, want=("coef", "mean", "var")):
        """(coef, zv_mean, zv_var, info, nsamples) of lzv (order 1) / qzv (order 2) for every chain, from the on-device value and gradient
        histories (klara_get_chain_zv, zv.jl): coef (nchains, K, ndims) — or (K, ndims) when pooled —, zv_mean and zv_var (nchains, ndims),
        each None when not in `want`; info (nchains,) int32: 0, 1 (singular), 2 (too few samples) — such a chain's outputs are NaN."""
        k = self.zv_nterms(order)
        coef = np.empty((k, self.ndims) if pooled else (self.nchains, k, self.ndims)) if "coef" in want else None
        zm = np.empty((self.nchains, self.ndims)) if "mean" in want else None
        zv = np.empty((self.nchains, self.ndims)) if "var" in want else None
        info = np.empty(self.nchains, dtype=np.int32); n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_zv(self._h, int(order), int(bool(pooled)), *[None if a is None else a.ctypes.data for a in (coef, zm, zv)],
                                             info.ctypes.data, C.byref(n)), "klara_get_chain_zv")
        return coef, zm, zv, info, int(n.value)

    def chain_zv_series(self, chain: int, order: int, coef=None) -> np.ndarray:
        """chain + f a of one chain in NState layout (ndims, nsaved), column-major — zv.jl's first return value, transposed; coef None:
        the chain's own coefficients, else a given (K, ndims) matrix such as the pooled one."""
        k = self.zv_nterms(order)
        a = None if coef is None else _f64(coef, (k, self.ndims))
        n = C.c_int64(0)
        L.check(self._lib.klara_get_chain_zv_series(self._h, int(chain), int(order), None if a is None else a.ctypes.data, None, 0, C.byref(n)),
                "klara_get_chain_zv_series")
        v = np.empty((self.ndims, n.value), order="F")
        L.check(self._lib.klara_get_chain_zv_series(self._h, int(chain), int(order), None if a is None else a.ctypes.data, v.ctypes.data, n.value,
                                                    C.byref(n)), "klara_get_chain_zv_series")
        return v

    def chain_zv_one(self, chain: int, order: int):
        """(corrected series (ndims, nsaved) column-major, a (K, ndims), info) of ONE chain from one fit on the device (klara_get_chain_zv_one):
        what zv.jl's lzv(s) / qzv(s) return for that chain's NState, the series transposed."""
        k = self.zv_nterms(order)
        n, info = C.c_int64(0), C.c_int32(0)
        L.check(self._lib.klara_get_chain_zv_one(self._h, int(chain), int(order), None, None, None, 0, C.byref(n)), "klara_get_chain_zv_one")
        v = np.empty((self.ndims, n.value), order="F"); a = np.empty((k, self.ndims))
        L.check(self._lib.klara_get_chain_zv_one(self._h, int(chain), int(order), a.ctypes.data, C.byref(info), v.ctypes.data, n.value, C.byref(n)),
                "klara_get_chain_zv_one")
        return v, a, int(info.value)

    def saved_steps(self) -> int:
        n = C.c_int64(0)
        L.check(self._lib.klara_saved_steps(self._h, C.byref(n)), "klara_saved_steps")
        return int(n.value)

    def chain_bm(self):
        """(mcvar_bm (nchains, ndims), nbatches): streaming batch means (bm_batchlen > 0), no stored history (mcvar.jl:35-41)."""
        out = np.empty((self.nchains, self.ndims)); nb = C.c_int64(0)
        L.check(self._lib.klara_get_chain_bm(self._h, out.ctypes.data, C.byref(nb)), "klara_get_chain_bm")
        return out, int(nb.value)

    def tune(self):
        step = np.empty(self.nchains); a = np.empty(self.nchains, dtype=np.int64)
        p = np.empty(self.nchains, dtype=np.int64); t = np.empty(self.nchains, dtype=np.int64)
        L.check(self._lib.klara_get_tune(self._h, step.ctypes.data, a.ctypes.data, p.ctypes.data, t.ctypes.data), "klara_get_tune")
        return step, a, p, t

    def ram_factor(self):
        """(S (nchains, ndims, ndims) lower triangular, skipped): the RAM sampler's current factor of every chain and the number of factor
        updates skipped since set_state / reset (klara_get_ram_factor; 0 in exact arithmetic)."""
        S = np.empty((self.nchains, self.ndims, self.ndims)); k = C.c_int64(0)
        L.check(self._lib.klara_get_ram_factor(self._h, S.ctypes.data, C.byref(k)), "klara_get_ram_factor")
        return S, int(k.value)

    def set_ram_factor(self, S):
        """per-chain factors for a warm start of the RAM sampler: (nchains, ndims, ndims), or one ndims x ndims factor for every chain; the
        lower triangles are read (klara_set_ram_factor)"""
        S = _f64(S)
        S = _f64(np.broadcast_to(S, (self.nchains, self.ndims, self.ndims)))
        L.check(self._lib.klara_set_ram_factor(self._h, S.ctypes.data), "klara_set_ram_factor")

    def am_state(self):
        """(C (nchains, ndims, ndims) symmetric, lastmean (nchains, ndims), secondlastmean (nchains, ndims), fallbacks): the AM sampler's current
        covariance and running means of every chain, and the number of transitions since set_state / reset at which corescale C did not factor
        and the chain proposed from the minor component (klara_get_am_state)."""
        Cm = np.empty((self.nchains, self.ndims, self.ndims)); m = np.empty((self.nchains, self.ndims)); m2 = np.empty((self.nchains, self.ndims))
        k = C.c_int64(0)
        L.check(self._lib.klara_get_am_state(self._h, Cm.ctypes.data, m.ctypes.data, m2.ctypes.data, C.byref(k)), "klara_get_am_state")
        return Cm, m, m2, int(k.value)

    def amwg_state(self):
        """(logsigma (nchains, ndims), accepted (nchains, ndims) int32, naccept_coord (nchains, ndims) uint64): the AMWG sampler's current log proposal
        scales, the accepted proposals of the current tuning window and the accepted proposals since set_state / reset, per chain and coordinate
        (klara_get_amwg_state)."""
        ls = np.empty((self.nchains, self.ndims)); a = np.empty((self.nchains, self.ndims), dtype=np.int32); n = np.empty((self.nchains, self.ndims), dtype=np.uint64)
        L.check(self._lib.klara_get_amwg_state(self._h, ls.ctypes.data, a.ctypes.data, n.ctypes.data), "klara_get_amwg_state")
        return ls, a, n

    def set_amwg_logsigma(self, logsigma) -> None:
        """warm start of the AMWG sampler: log proposal scales per chain ((nchains, ndims); (ndims,) serves every chain); the schedule is kept"""
        a = _f64(np.broadcast_to(_f64(logsigma), (self.nchains, self.ndims)))
        L.check(self._lib.klara_set_amwg_logsigma(self._h, a.ctypes.data), "klara_set_amwg_logsigma")

    def amwg_accept_mask(self) -> np.ndarray:
        """(transitions, nchains) uint32, bit i set where coordinate i moved (needs MON_ACCEPT; klara_get_amwg_accept_mask)"""
        n = C.c_int64(0)
        L.check(self._lib.klara_get_amwg_accept_mask(self._h, None, 0, C.byref(n)), "klara_get_amwg_accept_mask")
        m = np.empty((n.value, self.nchains), dtype=np.uint32)
        L.check(self._lib.klara_get_amwg_accept_mask(self._h, m.ctypes.data, n.value, C.byref(n)), "klara_get_amwg_accept_mask")
        return m

    def mh_factor(self) -> np.ndarray:
        """(ndims, ndims): the MH(Σ) sampler's current proposal factor, zeros above the diagonal (klara_get_mh_factor)"""
        f = np.empty((self.ndims, self.ndims))
        L.check(self._lib.klara_get_mh_factor(self._h, f.ctypes.data), "klara_get_mh_factor")
        return f

    def set_mh_factor(self, factor) -> None:
        """a new proposal factor for the MH(Σ) sampler, in effect from the next transition (klara_set_mh_factor).  An adaptation step: it belongs before
        the samples that are kept.  reset() puts the job's own factor back."""
        a = _f64(factor)
        if a.shape != (self.ndims, self.ndims):
            raise ValueError(f"the factor must be {self.ndims} x {self.ndims}, not {a.shape}")
        L.check(self._lib.klara_set_mh_factor(self._h, a.ctypes.data), "klara_set_mh_factor")

    def dual_averaging(self):
        eb = np.empty(self.nchains); hb = np.empty(self.nchains)
        L.check(self._lib.klara_get_dual_averaging(self._h, eb.ctypes.data, hb.ctypes.data), "klara_get_dual_averaging")
        return eb, hb

    def last_run_ms(self):
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self._lib.klara_last_run_ms(self._h, C.byref(ms), C.byref(n)), "klara_last_run_ms")
        return float(ms.value), int(n.value)

    def layout(self):
        k, g, e = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(self._lib.klara_get_layout(self._h, C.byref(k), C.byref(g), C.byref(e)), "klara_get_layout")
        return int(k.value), int(g.value), int(e.value)

    def launch_modes(self):
        """(counts[3], last_mode[4], last_accepted[4]) — how the launches were issued (klara_get_launch_modes): 4-lane kernel alone,
        8-lane kernel alone, device-decided pair; the per-partition values may lag the device (never synchronises)."""
        cnt = np.zeros(3, dtype=np.int64); lm = np.zeros(4, dtype=np.int32); la = np.zeros(4, dtype=np.int64)
        L.check(self._lib.klara_get_launch_modes(self._h, cnt.ctypes.data, lm.ctypes.data, la.ctypes.data), "klara_get_launch_modes")
        return cnt, lm, la

    def kernel_attributes(self, which: int = 0, nsteps: int = 32):
        """(vgprs, scratch bytes, static LDS bytes) of the transition kernel a launch of `nsteps` transitions runs, from the loaded
        code object (klara_get_kernel_attributes); which = 1: the 8-lane sibling of jobs two kernel families can run."""
        v, s_, l = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        L.check(self._lib.klara_get_kernel_attributes(self._h, int(which), int(nsteps), C.byref(v), C.byref(s_), C.byref(l)), "klara_get_kernel_attributes")
        return int(v.value), int(s_.value), int(l.value)

    def shader_clock_mhz(self) -> float:
        """Shader clock during the last launch of a pair-transposed kernel (klara_get_shader_clock); 0.0 when unknown."""
        if not hasattr(self._lib, "klara_get_shader_clock"):
            return 0.0
        v = C.c_double(0.0)
        L.check(self._lib.klara_get_shader_clock(self._h, C.byref(v)), "klara_get_shader_clock")
        return float(v.value)

    def device_ptrs(self):
        x, lt, g = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._lib.klara_device_ptrs(self._h, C.byref(x), C.byref(lt), C.byref(g)), "klara_device_ptrs")
        return x.value, lt.value, g.value
