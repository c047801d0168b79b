"""Host-side mirror of Klara.jl's job / sampler / tuner / range API for the many-chain GPU path.

Julia is not installed in the build image, so the host side above the C ABI is Python with
the same names, argument meaning and error behaviour as the reference's constructors:

    p       = BasicContMuvParameter("p", logtarget=GaussDiagTarget.negdot(2))   # README.md:29
    model   = likelihood_model(p, False)                                        # README.md:34
    sampler = MH(np.ones(2))                                                    # README.md:38
    mcrange = BasicMCRange(nsteps=10000, burnin=1000)                           # README.md:42
    job     = BasicMCJob(model, sampler, mcrange, {"p": [5.1, -0.9]})           # README.md:50
    run(job); chain = output(job); mean(chain); acceptance(chain)               # README.md:54-66

Differences forced by the device: `logtarget=` takes a *target family object* (engine.GaussDiagTarget,
GaussDenseTarget, LogisticTarget) instead of an arbitrary closure, and `v0[key]` may be an
(nchains x D) matrix — one BasicMCJob then stands for nchains independent jobs
(`run(job::Vector) = map(run, job)`, src/jobs/jobs.jl:212, executed as one launch).
The Julia package a maintainer would ship is sketched in INTEGRATION.md.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib as L
from .engine import CustomTarget, Engine, GaussDenseTarget, GaussDiagTarget, HierNormalTarget, LogisticTarget, Marginals, histogram_quantiles


# ------------------------------------------------------------------ range (src/ranges/BasicMCRange.jl)
class BasicMCRange:
    """BasicMCRange(nsteps=100, burnin=0, thinning=1) — BasicMCRange.jl:36; asserts :22-24."""

    def __init__(self, nsteps: int = 100, burnin: int = 0, thinning: int = 1):
        assert burnin >= 0, "Number of burn-in iterations should be non-negative"
        assert thinning >= 1, "Thinning should be >= 1"
        assert nsteps > burnin, "Total number of MCMC iterations should be greater than number of burn-in iterations"
        self.burnin, self.thinning = int(burnin), int(thinning)
        self.postrange = range(self.burnin + 1, int(nsteps) + 1, self.thinning)  # (burnin+1):thinning:nsteps
        # Julia's StepRange normalises `last` (BasicMCRange.jl:20: nsteps = last(postrange))
        self.nsteps = self.postrange[-1]
        self.npoststeps = len(self.postrange)

    def __repr__(self):
        return f"BasicMCRange: number of steps = {self.nsteps}, burnin = {self.burnin}, thinning = {self.thinning}"


# ------------------------------------------------------------------ samplers (src/samplers/*.jl)
class MCSampler:
    pass


class MH(MCSampler):
    """MH(sigma::Real) / MH(sigma::Vector) / MH(Σ::Matrix): symmetric, normalised MvNormal(x, ·) random walk — MH.jl:63-66.  As in Distributions a
    number or a vector holds standard deviations and a matrix holds the covariance, so MH(np.diag(sigma**2)) is MH(sigma).  The matrix form proposes
    x + L z with L = cholesky(Σ), one factor for the whole job (`cov`, `factor`; BasicMCJob.engine.mh_factor() / set_mh_factor()); on the device for
    the logistic regression up to 16 parameters and user-defined whole-vector targets with D <= 32.  rwm_factor(cov) gives the factor of the
    classical (2.38² / D) Σ̂ from a pilot run's pooled_cov."""

    def __init__(self, sigma):
        a = np.asarray(sigma, dtype=np.float64)
        self.symmetric, self.normalised = True, True
        if a.ndim == 2:                                          # MH(σ::Matrix{N}) = MH(x -> MvNormal(x, σ))
            assert a.shape[0] == a.shape[1], "MH: the proposal covariance must be a square matrix"
            assert np.allclose(a, a.T, rtol=1e-12, atol=0.0), "MH: the proposal covariance must be symmetric"
            try:
                f = np.linalg.cholesky(a)
            except np.linalg.LinAlgError:
                f = None
            assert f is not None and np.all(np.isfinite(f)), "MH: the proposal covariance must be positive definite"
            self.cov, self.factor, self.kind = a.copy(), f, L.SAMPLER_MH_COV
        else:
            self.sigma = np.atleast_1d(a).copy()

    @classmethod
    def from_factor(cls, factor):
        """MH(Σ) from a lower factor the caller already holds (Σ = L L'; the lower triangle is read, its diagonal must be positive)"""
        f = np.asarray(factor, dtype=np.float64)
        assert f.ndim == 2 and f.shape[0] == f.shape[1], "MH.from_factor: the factor must be a square matrix"
        f = np.tril(f)
        assert np.all(np.isfinite(f)) and np.all(np.diag(f) > 0), "MH.from_factor: the factor needs finite entries and a positive diagonal"
        s = cls.__new__(cls)
        s.symmetric, s.normalised = True, True
        s.cov, s.factor, s.kind = f @ f.T, f.copy(), L.SAMPLER_MH_COV
        return s

    kind = L.SAMPLER_MH


def rwm_factor(cov, scale=None) -> np.ndarray:
    """cholesky(scale · cov), scale = 2.38² / D by default: the factor of the random-walk Metropolis proposal that is optimal for a Gaussian target
    of covariance `cov` (Gelman, Roberts and Gilks 1996; Roberts and Rosenthal 2001) — for MH.from_factor or Engine.set_mh_factor."""
    c = np.asarray(cov, dtype=np.float64)
    assert c.ndim == 2 and c.shape[0] == c.shape[1], "rwm_factor: the covariance must be a square matrix"
    s = 2.38 ** 2 / c.shape[0] if scale is None else float(scale)
    assert s > 0, "rwm_factor: the scale must be positive"
    return np.linalg.cholesky(s * c)


class MALA(MCSampler):
    """MALA(driftstep=1.) — MALA.jl:61-70."""
    kind = L.SAMPLER_MALA

    def __init__(self, driftstep: float = 1.0):
        assert driftstep > 0, "Drift step is not positive"
        self.driftstep = float(driftstep)


class SoftAbs:
    """H -> softabs(H, a) (stats/metrics.jl:1-4) as an object the device path can recognise: SMMALA(1.25, SoftAbs(1000.)) is the
    reference's SMMALA(1.25, H -> softabs(H, 1000.)) (doc/examples/BivariateNormal/SMMALA/analytical.jl:16).  Calling it gives
    klara_jl_amd.stats.softabs(H, a), the NumPy restatement; the job applies the transform on the device (klara_desc.smmala_softabs)."""

    def __init__(self, a: float = 1000.0):
        a = float(a)
        if not (a > 0.0 and np.isfinite(a)):
            raise ValueError("SoftAbs: a must be a positive finite number")
        self.a = a

    def __call__(self, H):
        from .stats import softabs
        return softabs(H, self.a)

    def __repr__(self):
        return f"SoftAbs({self.a!r})"


class SMMALA(MCSampler):
    """SMMALA(driftstep=1., transform=nothing) — SMMALA.jl:127-137.  The metric is the target's tensorlogtarget: on the device the
    logistic regression with D <= 8 (X' diag(r (1 - r)) X + I / lambda, doc/examples/swiss/SMMALA/analytical.jl:20-23) or a user-defined
    target's tensor / minus-Hessian.  `transform` is None or a SoftAbs (user-defined targets only: the transform runs on the device);
    any other callable is a closure the device cannot run and is refused."""
    kind = L.SAMPLER_SMMALA

    def __init__(self, driftstep: float = 1.0, transform=None):
        assert driftstep > 0, "Drift step is not positive"
        if transform is not None and not isinstance(transform, SoftAbs):
            raise NotImplementedError("SMMALA: the only transform of the metric that runs on the device is SoftAbs(a) "
                                      "(H -> softabs(H, a)); an arbitrary closure is not supported")
        self.driftstep, self.transform = float(driftstep), transform


class RAM(MCSampler):
    """RAM(S0::Matrix) / RAM(S0::Vector) / RAM(S0=1., n=1), keywords targetrate=0.234, gamma=0.7 (the reference's γ) — RAM.jl:94-111:
    the robust adaptive Metropolis sampler of Vihola (2012).  S0 is the initial lower-triangular factor of the proposal (a matrix: its
    lower triangle; a vector: its diagonal; a number: that number n times).  On the device for D <= 8: the logistic regression and
    user-defined whole-vector targets; a correlated Gaussian is run as such a closure.  Every chain adapts its own factor
    (BasicMCJob.engine.ram_factor())."""
    kind = L.SAMPLER_RAM

    def __init__(self, S0=1.0, n: int = 1, *, targetrate: float = 0.234, gamma: float = 0.7):
        a = np.asarray(S0, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(int(n), float(a))                        # RAM(S0::Real=1., n::Integer=1) = RAM(fill(S0, n))
        if a.ndim == 1:
            a = np.diag(a)                                       # RAM(S0::RealVector) = RAM(RealLowerTriangular(diagm(S0)))
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("RAM: S0 must be a square matrix, a vector (its diagonal) or a number")
        a = np.tril(a)                                           # RealLowerTriangular(S0)
        assert np.all(np.diag(a) > 0), "All diagonal elements of initial adaptation matrix must be positive"
        assert 0 < targetrate < 1, "Target acceptance rate should be between 0 and 1"
        assert 0.5 < gamma <= 1, "Exponent of stepsize must be greater than 0.5 and less or equal to 1"
        self.S0, self.targetrate, self.gamma = a.copy(), float(targetrate), float(gamma)


class AM(MCSampler):
    """AM(C0::Matrix) / AM(C0::Vector) / AM(C0::Real, d=1), keywords corescale=1., minorscale=1., c=0.05, t0=10 — AM.jl:131-154: the adaptive
    Metropolis sampler of Haario, Saksman and Tamminen (2001) with the mixture proposal of Roberts and Rosenthal (2009).  C0 is the initial
    covariance (a vector: its diagonal; a number: that number d times).  Up to transition t0 a chain proposes from N(x, minorscale I); after it,
    from the mixture of N(x, corescale C), weight 1 - c, and N(x, minorscale I), weight c, with C the covariance of its own states so far.  On the
    device for D <= 8, on RAM's targets; t0 = 1 and c >= 1 are refused by the library (BasicMCJob.engine.am_state())."""
    kind = L.SAMPLER_AM

    def __init__(self, C0, d: int = 1, *, corescale: float = 1.0, minorscale: float = 1.0, c: float = 0.05, t0: int = 10):
        a = np.asarray(C0, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(int(d), float(a))                        # AM(C0::Real, d::Integer=1) = AM(fill(C0, d))
        if a.ndim == 1:
            a = np.diag(a)                                       # AM(C0::RealVector) = AM(diagm(C0))
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("AM: C0 must be a square matrix, a vector (its diagonal) or a number")
        assert 0 < corescale, f"Constant corescale must be positive, got {corescale}"
        assert 0 < minorscale, f"Constant minorscale must be positive, got {minorscale}"
        assert 0 <= c, "Constant c must be non-negative"
        assert t0 > 0, "t0 is not positive"
        self.C0, self.corescale, self.minorscale, self.c, self.t0 = a.copy(), float(corescale), float(minorscale), float(c), int(t0)


class MuvAMWG(MCSampler):
    """MuvAMWG(σ::Vector) / MuvAMWG(d; lower=fill(-Inf, d), upper=fill(Inf, d), σ=1.) — AMWG.jl:139-151: adaptive Metropolis-within-Gibbs (Roberts and
    Rosenthal 2009, section 3).  A transition updates the coordinates one at a time, each with a normal proposal of its own scale; with
    RobertsRosenthalMCTuner every chain learns one scale per coordinate.  `logsigma0` is the reference's logσ0 = log.(σ) (the proposal's standard deviation is
    sqrt(exp(logσ)), iterate/AMWG.jl:98, kept).  Gradient-free, D <= 32 on the device: the logistic regression up to 16 parameters and user-defined
    whole-vector targets.  The truncated proposals of finite bounds are not built: a finite `lower` or `upper` is refused
    (BasicMCJob.engine.amwg_state())."""
    kind = L.SAMPLER_AMWG

    def __init__(self, sigma_or_d=None, *, lower=None, upper=None, sigma=None, **kw):
        if "σ" in kw:
            sigma = kw.pop("σ")
        if kw:
            raise TypeError(f"MuvAMWG: unexpected keyword arguments {sorted(kw)}")
        if sigma_or_d is None:
            raise TypeError("MuvAMWG needs the vector of σ or the number of dimensions d")
        if isinstance(sigma_or_d, (int, np.integer)) and not isinstance(sigma_or_d, bool):       # MuvAMWG(d::Integer; lower, upper, σ::Real=1.)
            d = int(sigma_or_d)
            s = np.full(d, 1.0 if sigma is None else float(sigma))
        else:                                                                                    # MuvAMWG(σ::RealVector)
            if lower is not None or upper is not None or sigma is not None:
                raise TypeError("MuvAMWG(σ::Vector) takes no keywords; use MuvAMWG(d; lower, upper, σ)")
            s = np.asarray(sigma_or_d, dtype=np.float64).ravel().copy()
            d = s.size
        self.lower = np.full(d, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64).ravel().copy()
        self.upper = np.full(d, np.inf) if upper is None else np.asarray(upper, dtype=np.float64).ravel().copy()
        if self.lower.size != d or self.upper.size != d:
            raise ValueError("MuvAMWG: lower and upper must have d elements")
        for name, b in (("lower", self.lower), ("upper", self.upper)):
            if np.any(np.isfinite(b)):
                raise NotImplementedError(f"MuvAMWG: a finite `{name}` bound asks for the truncated-normal proposal (iterate/AMWG.jl:100-115), "
                                          "which is not built on the device")
        with np.errstate(all="ignore"):
            self.logsigma0 = np.log(s)                                                           # map(log, σ)
        self.sigma = s


AMWG = MuvAMWG      # (the reference's abstract type over UnvAMWG / MuvAMWG; the univariate sampler is the vector one at d = 1)


class HMC(MCSampler):
    """HMC(leapstep=0.1, nleaps=10) — HMC.jl:89-100."""
    kind = L.SAMPLER_HMC

    def __init__(self, leapstep: float = 0.1, nleaps: int = 10):
        assert leapstep > 0, "Leapfrog step is not positive"
        assert nleaps > 0, "Number of leapfrog steps is not positive"
        self.leapstep, self.nleaps = float(leapstep), int(nleaps)


class SliceSampler(MCSampler):
    """SliceSampler(widths, stepout=true) / SliceSampler(width=1., n=1, stepout=true) — SliceSampler.jl:22-34."""
    kind = L.SAMPLER_SLICE

    def __init__(self, widths=1.0, n: Optional[int] = None, stepout: bool = True):
        if np.ndim(widths) == 0:
            widths = np.full(int(n) if n is not None else 1, float(widths))
        self.widths = np.asarray(widths, dtype=np.float64).copy()
        assert np.all(self.widths > 0), "All widths must be positive"
        self.stepout = bool(stepout)


# ------------------------------------------------------------------ tuners (src/tuners/*.jl)
class MCTuner:
    pass


class VanillaMCTuner(MCTuner):
    """VanillaMCTuner(period=100, verbose=false) — VanillaMCTuner.jl; defaults test/VanillaMCTuner.jl:6-9."""
    kind = L.TUNER_VANILLA

    def __init__(self, period: int = 100, verbose: bool = False):
        assert period > 0, "Tuning period should be positive"
        self.period, self.verbose = int(period), bool(verbose)


class RobertsRosenthalMCTuner(MCTuner):
    """RobertsRosenthalMCTuner(targetrate=0.44, period=50, verbose=false) — RobertsRosenthalMCTuner.jl:84-97: every `period` transitions a coordinate's
    log proposal scale moves by δ = min(0.01, batch^-1/2) towards the target acceptance rate.  The tuner of MuvAMWG, and of nothing else."""
    kind = L.TUNER_ROBERTS_ROSENTHAL

    def __init__(self, targetrate: float = 0.44, period: int = 50, verbose: bool = False):
        assert 0 < targetrate < 1, "Target acceptance rate should be between 0 and 1"
        assert period > 0, "Tuning period should be positive"
        self.targetrate, self.period, self.verbose = float(targetrate), int(period), bool(verbose)


def logistic(x, l=1.0, k=1.0, x0=0.0, y0=0.0):
    """stats/logistic.jl:11 (host convenience; the device uses its own deterministic exp)."""
    return l / (1.0 + np.exp(-k * (x - x0))) + y0


def logistic_rate_score(x, k=7.0):
    """AcceptanceRateMCTuner.jl:9."""
    return logistic(x, 2.0, k, 0.0, 0.0)


def erf_rate_score(x, k=3.0):
    """AcceptanceRateMCTuner.jl:17."""
    from math import erf
    return erf(k * x) + 1.0


class AcceptanceRateMCTuner(MCTuner):
    """AcceptanceRateMCTuner(targetrate; score=logistic_rate_score, period=100, verbose=false) — :38-44.

    `mode="per_chain"` keeps the reference's one-tune-per-job semantics; `mode="pooled"` shares one step
    per GPU with the acceptance rate pooled over that GPU's chains (BASELINE cfg 5).
    `score` is logistic_rate_score or erf_rate_score; `score_k` is its steepness (defaults 7 and 3).
    """
    kind = L.TUNER_ACCEPT_RATE

    def __init__(self, targetrate: float, score=logistic_rate_score, period: int = 100, verbose: bool = False,
                 score_k: float = 7.0, mode: str = "per_chain"):
        assert 0 < targetrate < 1, "Target acceptance rate should be between 0 and 1"
        assert period > 0, "Tuning period should be positive"
        if score not in (logistic_rate_score, erf_rate_score):
            raise NotImplementedError("device scores: logistic_rate_score, erf_rate_score")
        if score is erf_rate_score and score_k == 7.0:
            score_k = 3.0                       # erf_rate_score's own default steepness (AcceptanceRateMCTuner.jl:17)
        self.score_kind = 1 if score is erf_rate_score else 0
        assert mode in ("per_chain", "pooled")
        self.targetrate, self.period, self.verbose = float(targetrate), int(period), bool(verbose)
        self.score_k, self.mode = float(score_k), mode


class DualAveragingMCTuner(MCTuner):
    """DualAveragingMCTuner(targetrate, nadapt; ε0bar=1., h0bar=0., γ=0.05, t0=10, κ=0.75, period=100, verbose=false)
    — DualAveragingMCTuner.jl:54-93.  HMC only (as in the reference: HMC.jl:124-133)."""
    kind = L.TUNER_DUAL_AVERAGING

    def __init__(self, targetrate: float, nadapt: int, eps0bar: float = 1.0, h0bar: float = 0.0, gamma: float = 0.05,
                 t0: int = 10, kappa: float = 0.75, period: int = 100, verbose: bool = False):
        assert 0 < targetrate < 1, "Target acceptance rate should be between 0 and 1"
        assert nadapt > 0, "Number of adaptation steps should be positive"
        assert eps0bar > 0, "ε0bar should be positive"
        assert period > 0, "Period over which acceptance rate is reported in verbose mode should be positive"
        assert t0 > 0, "t0 should be positive"
        self.targetrate, self.nadapt, self.eps0bar, self.h0bar = float(targetrate), int(nadapt), float(eps0bar), float(h0bar)
        self.gamma, self.t0, self.kappa, self.period, self.verbose = float(gamma), int(t0), float(kappa), int(period), bool(verbose)


# ------------------------------------------------------------------ parameter / model
class DiffOptions:
    """DiffOptions(mode=:reverse, order=1, targets=fill(false, 3), chunksize=0, compiled=true) — src/autodiff/autodiff.jl:55-76, with
    its four assertions.  On the device only forward mode exists (klara_autodiff.h: dual numbers swept through the user's generic
    log-target; there are no tapes): `mode="reverse"` is accepted here as in the reference, and refused where a parameter is built
    with it.  `order=2` also gives the SMMALA sampler its metric, minus the Hessian (forward.jl:11-16); `chunksize` is the number of
    directions per sweep (0: the library's choice); `targets` and `compiled` are kept and have no meaning on the device."""

    def __init__(self, mode="reverse", order: int = 1, targets=None, chunksize: int = 0, compiled: bool = True):
        mode = str(mode).lstrip(":")
        targets = [False, False, False] if targets is None else [bool(t) for t in targets]
        assert mode in ("reverse", "forward"), f"Mode of automatic differentation must be :reverse or :forward, got {mode}"
        assert order in (1, 2), f"Order of differentiation must be 1 or 2, got order={order}"
        assert len(targets) == 3, f"Length of targets must be 3, got {len(targets)}-length vector"
        assert chunksize >= 0, f"chunksize can not be negative, got chunksize={chunksize}"
        self.mode, self.order, self.targets, self.chunksize, self.compiled = mode, int(order), targets, int(chunksize), bool(compiled)

    def __repr__(self):
        return f"DiffOptions(mode=:{self.mode}, order={self.order}, targets={self.targets}, chunksize={self.chunksize}, compiled={self.compiled})"

    def require_forward(self) -> None:
        if self.mode != "forward":
            raise NotImplementedError("DiffOptions(mode=:reverse): reverse-mode tapes do not exist on the device; use mode=:forward "
                                      "(forward-mode dual numbers, klara_autodiff.h)")


class BasicContMuvParameter:
    """BasicContMuvParameter(key; logtarget=...) — BasicContMuvParameter.jl:383-411.

    `logtarget` is a device target family; for LogisticTarget it plays the role of
    loglikelihood+logprior+gradlogtarget of doc/examples/swiss/MALA/analytical.jl:20-26.
    """

    def __init__(self, key: str, logtarget=None, loglikelihood: Optional[str] = None, logprior: Optional[str] = None,
                 gradloglikelihood: Optional[str] = None, gradlogprior: Optional[str] = None, ndims: Optional[int] = None, data=None,
                 diffopts: Optional[DiffOptions] = None, **unsupported):
        if unsupported:
            raise NotImplementedError(f"closure fields not available on device: {sorted(unsupported)}")
        if diffopts is not None:
            # diffopts=DiffOptions(mode=:forward) (doc/examples/swiss/MALA/forwarddiff.jl): the closures are generic C++ text without gradients
            # (klara_user_logtarget_ad, or klara_user_loglikelihood_ad + klara_user_logprior_ad), differentiated on the device
            diffopts.require_forward()
            if gradloglikelihood is not None or gradlogprior is not None:
                raise ValueError("diffopts and gradient closures are alternatives")
            if ndims is None:
                raise ValueError("ndims is required with diffopts")
            if isinstance(logtarget, str):
                if loglikelihood is not None or logprior is not None:
                    raise ValueError("logtarget and loglikelihood / logprior are alternatives")
                src = logtarget
            elif logtarget is None and loglikelihood is not None and logprior is not None:
                src = "#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + loglikelihood + "\n" + logprior
            else:
                raise ValueError("diffopts goes with logtarget (C++ source text) or with both loglikelihood and logprior")
            logtarget, loglikelihood, logprior = CustomTarget.autodiff(ndims, src, data, order=diffopts.order, chunksize=diffopts.chunksize), None, None
        if logtarget is None:
            # likelihood + prior closures (BasicContMuvParameter.jl:174-201): C text for each, composed on device as
            # logtarget = loglikelihood + logprior, gradlogtarget = gradloglikelihood + gradlogprior
            if loglikelihood is None or logprior is None:
                raise ValueError("give logtarget (a target family object) or both loglikelihood and logprior (C source text)")
            if ndims is None:
                raise ValueError("ndims is required with loglikelihood / logprior closures")
            if (gradloglikelihood is None) != (gradlogprior is None):
                raise ValueError("gradloglikelihood and gradlogprior go together")
            logtarget = CustomTarget.likelihood_prior(ndims, loglikelihood, logprior, gradloglikelihood or "", gradlogprior or "", data)
        elif loglikelihood is not None or logprior is not None:
            raise ValueError("logtarget and loglikelihood / logprior are alternatives")
        if not isinstance(logtarget, (GaussDiagTarget, GaussDenseTarget, LogisticTarget, HierNormalTarget, CustomTarget)):
            raise TypeError("logtarget must be GaussDiagTarget, GaussDenseTarget, LogisticTarget, HierNormalTarget or CustomTarget")
        self.key = str(key).lstrip(":")
        self.target = logtarget


@dataclass
class GenericModel:
    """Just enough of src/models/GenericModel.jl to route v0[key] to the parameter (BasicMCJob.jl:156-185)."""
    vertices: list
    ofkey: Dict[str, int] = field(default_factory=dict)


def likelihood_model(p, isindexed: bool = True) -> GenericModel:
    """likelihood_model(vs, isindexed) — src/models/generators.jl:5-18 (single-parameter form)."""
    vs = list(p) if isinstance(p, (list, tuple)) else [p]
    return GenericModel(vs, {v.key: i for i, v in enumerate(vs) if hasattr(v, "key")})


# ------------------------------------------------------------------ chain container
class MuvChains:
    """Output of a job: the BasicContMuvParameterNState of every chain
    (src/nstates/ParameterNStates/BasicContMuvParameterNState.jl:1-21).

    value(c)            (ndims x n) column-major matrix of chain c (requires :value monitored)
    diagnosticvalues    (nsaved_steps x nchains) accept flags over the postrange when :accept requested
    """

    def __init__(self, job: "BasicMCJob"):
        self._job = job
        eng = job.engine
        self.size, self.nchains = eng.ndims, eng.nchains
        self.n = job.range.npoststeps
        self.diagnostickeys = list(job.outopts.get("diagnostics", []))
        self._sums = eng.chain_sums() if eng.monitor & L.MON_SUMMARIES else None
        self._acc = None
        if eng.monitor & L.MON_ACCEPT:
            m = eng.accept_mask()
            post = np.asarray(job.range.postrange) - 1
            self._acc = m[post[post < m.shape[0]]]

    def value(self, chain: int = 0) -> np.ndarray:
        return self._job.engine.chain(chain)

    def logtarget(self, chain: int = 0) -> np.ndarray:
        return self._job.engine.chain_fields(chain, True, False)[0]

    def gradlogtarget(self, chain: int = 0) -> np.ndarray:
        return self._job.engine.chain_fields(chain, False, True)[1]

    def loglikelihood(self, chain: int = 0) -> np.ndarray:
        return self._job.engine.chain_likelihood_prior(chain)[0]

    def logprior(self, chain: int = 0) -> np.ndarray:
        return self._job.engine.chain_likelihood_prior(chain)[1]

    @property
    def diagnosticvalues(self):
        return self._acc


def mean(chains: MuvChains, chain: Optional[int] = None) -> np.ndarray:
    """mean(s::VariableNState{Multivariate}) — stats/mean.jl:7-11: per-dimension mean over saved steps.
    chain=None returns (nchains x D) from the on-device running sums; chain=c reads that chain's history."""
    if chains._sums is None:
        if not (chains._job.engine.monitor & L.MON_HISTORY):
            raise ValueError("mean needs the running sums (summaries=True) or the stored values (monitor value)")
        if chain is not None:
            return chains.value(chain).mean(axis=1)
        return np.stack([chains.value(c).mean(axis=1) for c in range(chains.nchains)])
    s, _, n = chains._sums
    m = s / n
    return m if chain is None else m[chain]


def mcvar_iid(chains: MuvChains) -> np.ndarray:
    """mcvar(s, Val{:iid}) = var(v)/length(v) — stats/variance/mcvar.jl:5 (per chain, per dimension)."""
    if chains._sums is None:
        if not (chains._job.engine.monitor & L.MON_HISTORY):
            raise ValueError("mcvar_iid needs the running sums (summaries=True) or the stored values (monitor value)")
        return chain_mcvar(chains, "iid")
    s, q, n = chains._sums
    var = (q - s * s / n) / (n - 1)
    return var / n


def chain_mcvar(chains: MuvChains, vtype: str = "imse", batchlen: int = 100, maxlag: Optional[int] = None) -> np.ndarray:
    """mcvar(s, Val{vtype}) for EVERY chain and dimension at once, computed on device over the stored history
    (stats/variance/mcvar.jl:5,35-41,75-105,137-158) — or, for "bm" / "imse" / "ipse", from what a job with bm_batchlen / acov_maxlag
    accumulated while sampling.  Returns (nchains x D); vtype in {"iid", "bm", "imse", "ipse"}.
    `maxlag` left at its default means the reference's default (0 = n - 1 lags, mcvar.jl:75) when the values are stored, and the job's own
    window `acov_maxlag` when the job streams its autocovariances without a value history — the estimate is then TRUNCATED at that lag
    (<= 31); an explicit maxlag other than the window is refused for such a job."""
    job = chains._job
    if vtype == "bm" and job.bm_batchlen == batchlen and not (job.engine.monitor & L.MON_HISTORY):
        return job.engine.chain_bm()[0]            # streaming batch means: no history was stored
    streamed = job.acov_maxlag > 0 and not (job.engine.monitor & L.MON_HISTORY)
    if vtype in ("imse", "ipse") and streamed:
        # The autocovariances kept while sampling stop at lag acov_maxlag (<= 127); the reference's maxlag = 0 means n - 1
        # (mcvar.jl:75).  The streamed estimator is therefore only returned for the lag window it was built for — asked for
        # explicitly, maxlag == acov_maxlag — and anything else needs the stored values (a slowly mixing chain whose
        # Geyer sequence has not turned non-positive by lag 31 would be silently underestimated).
        if maxlag is not None and maxlag != job.acov_maxlag:
            raise ValueError(f"this job keeps streaming autocovariances up to lag {job.acov_maxlag} and no value history: "
                             f"mcvar(:{vtype}) is available for maxlag={job.acov_maxlag} only (asked for maxlag={maxlag}, where 0 means n - 1)")
        imse, ipse, _ = job.engine.chain_acov_mcvar(want=(vtype,))
        return imse if vtype == "imse" else ipse
    maxlag = 0 if maxlag is None else maxlag
    if vtype == "ipse":
        return job.engine.chain_mcvar_ipse(maxlag)
    return job.engine.chain_mcvar(batchlen, maxlag, want=(vtype,))[{"iid": 0, "bm": 1, "imse": 2}[vtype]]


def _mcvar_pair(chains: MuvChains, vtype: str, batchlen: int, maxlag: Optional[int]):
    """(mcvar_iid, mcvar_vtype) of every chain and dimension; vtype in {"bm", "imse", "ipse"}."""
    if vtype not in ("bm", "imse", "ipse"):
        raise ValueError(f"vtype must be 'bm', 'imse' or 'ipse', not {vtype!r}")
    has_history = bool(chains._job.engine.monitor & L.MON_HISTORY)      # (two-pass variance over the stored values when they exist)
    return (chain_mcvar(chains, "iid") if has_history else mcvar_iid(chains)), chain_mcvar(chains, vtype, batchlen, maxlag)


def chain_ess(chains: MuvChains, vtype: str = "imse", batchlen: int = 100, maxlag: Optional[int] = None) -> np.ndarray:
    """ess(s, vtype) = n * mcvar_iid / mcvar_vtype (stats/convergence/ess.jl:3) for every chain and dimension."""
    iid, v = _mcvar_pair(chains, vtype, batchlen, maxlag)
    with np.errstate(invalid="ignore", divide="ignore"):       # (a series that never moved: 0 / 0 = NaN, as in the reference's arithmetic)
        return chains.n * iid / v


def chain_iact(chains: MuvChains, vtype: str = "imse", batchlen: int = 100, maxlag: Optional[int] = None) -> np.ndarray:
    """iact(s, vtype) = mcvar_vtype / mcvar_iid (stats/convergence/iact.jl:3) for every chain and dimension."""
    iid, v = _mcvar_pair(chains, vtype, batchlen, maxlag)
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / iid


def _zv_engine(chains: MuvChains, name: str):
    eng = chains._job.engine
    missing = [f for f, bit in (("value", L.MON_HISTORY), ("gradlogtarget", L.MON_HIST_GRAD)) if not (eng.monitor & bit)]
    if missing:
        raise ValueError(f"{name} needs the stored value and gradlogtarget of every saved step: add {' and '.join(repr(m) for m in missing)} "
                         f"to outopts monitor (missing: {', '.join(missing)})")
    return eng


def _chain_zv(chains: MuvChains, order: int, pooled: bool, name: str):
    eng = _zv_engine(chains, name)
    coef, zm, zv, info, _ = eng.chain_zv(order, pooled)
    return zm, zv, coef, info


def chain_lzv(chains: MuvChains, pooled: bool = False):
    """lzv (stats/variance/zv.jl:16-34) for EVERY chain at once, on the device over the stored value and gradlogtarget histories:
    (zv_mean (nchains x D), zv_var (nchains x D), a (nchains x D x D; pooled: D x D), info (nchains)) — mean and sample variance of the
    corrected series chain + z a with z = -gradlogtarget / 2.  pooled=True fits ONE coefficient matrix to the concatenation of all
    chains' samples (many short replicas); means and variances stay per chain.  info 1 (singular, e.g. a chain that never moved) or
    2 (fewer than K + 2 samples) marks chains whose outputs are NaN."""
    return _chain_zv(chains, L.ZV_LINEAR, pooled, "chain_lzv")


def chain_qzv(chains: MuvChains, pooled: bool = False):
    """qzv (zv.jl:50-80) for every chain at once: as chain_lzv with the K = D (D + 3) / 2 quadratic control variates (D <= 14)."""
    return _chain_zv(chains, L.ZV_QUADRATIC, pooled, "chain_qzv")


def _zv_one(chains: MuvChains, chain: int, order: int, name: str):
    series, a, _ = _zv_engine(chains, name).chain_zv_one(chain, order)      # one fit of that chain on the device
    return series.T, a


def lzv(chains: MuvChains, chain: int = 0):
    """lzv(s::ParameterNState{Continuous, Multivariate}) (zv.jl:38) of chain `chain`: (chain + z a (n x D), a (D x D)), from the device."""
    return _zv_one(chains, chain, L.ZV_LINEAR, "lzv")


def qzv(chains: MuvChains, chain: int = 0):
    """qzv(s::ParameterNState{Continuous, Multivariate}) (zv.jl:84) of chain `chain`: (chain + qz a (n x D), a (K x D)), from the device."""
    return _zv_one(chains, chain, L.ZV_QUADRATIC, "qzv")


def pooled_cov(job_or_chains, comm=None) -> np.ndarray:
    """The posterior covariance pooled over all chains and saved steps of a job run with covariance=True: M / (n - 1), M = sum (x - mean)(x - mean)'
    accumulated while sampling (Engine.pooled_covariance); `comm`: a klara_comm handle, to pool over every rank's chains."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    _, m2, ns, _ = job.engine.pooled_covariance(comm)
    if ns < 2:
        raise ValueError("pooled_cov needs at least two saved samples")
    return m2 / (ns - 1)


def pooled_hist(job_or_chains, comm=None):
    """(counts[D, nbins + 2], edges[D, nbins + 1]) of a job run with marginals=: every dimension's saved samples over all chains, counted while sampling
    (Engine.pooled_histogram); columns 0 and nbins + 1 are the underflow and the overflow.  `comm`: a klara_comm handle, to pool over every rank's chains."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    counts, edges, _, _ = job.engine.pooled_histogram(comm)
    return counts, edges


def pooled_quantiles(job_or_chains, probs, comm=None) -> np.ndarray:
    """(D, len(probs)) posterior quantiles from pooled_hist's counts (klara_histogram_quantiles): within one bin width of the order statistic; -inf / +inf
    where it lies outside the job's [lo, hi) — a range chosen badly is never clipped silently."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    m = job.engine.marginals
    counts, _, _, _ = job.engine.pooled_histogram(comm)
    return histogram_quantiles(counts, m.nbins, m.lo, m.hi, probs)


def derived_mean(job_or_chains, comm=None) -> np.ndarray:
    """(K,) posterior mean of every output of the job's derived= closure over all chains and saved steps (Engine.derived_moments); `comm`: a klara_comm
    handle, to pool over every rank's chains."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    return job.engine.derived_moments(comm)[0]


def derived_var(job_or_chains, comm=None) -> np.ndarray:
    """(K,) pooled variance M2 / n of every output of the job's derived= closure — var(chain) over the pooled chains, without the cancellation of
    sumsq / n - mean^2 (Engine.derived_moments)."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    _, m2, ns, _ = job.engine.derived_moments(comm)
    if ns < 1:
        raise ValueError("derived_var needs at least one saved sample")
    return m2 / ns


def derived_rhat(job_or_chains, comm=None) -> np.ndarray:
    """(K,) R-hat of every output of the job's derived= closure over all chains, from their running sums (Engine.derived_rhat)."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    return job.engine.derived_rhat(comm)["rhat"]


def derived_quantiles(job_or_chains, probs, comm=None) -> np.ndarray:
    """(K, len(probs)) posterior quantiles of the outputs of a derived= closure built with marginals=, from their pooled histograms
    (Engine.derived_histogram, klara_histogram_quantiles): as pooled_quantiles for the coordinates."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    counts, _, _, _ = job.engine.derived_histogram(comm)
    m = job.engine.derived.marginals
    return histogram_quantiles(counts, m.nbins, m.lo, m.hi, probs)


def rhat(job_or_chains, split: bool = False, comm=None) -> np.ndarray:
    """The potential scale reduction factor R-hat (Gelman & Rubin 1992) per dimension over all chains of a job, formed on the device (Engine.rhat):
    from the running sums, or with split=True the split form (BDA3 section 11.4) from the stored history; `comm`: a klara_comm handle, to take every
    rank's chains.  Values near 1 say the chains agree; the reference has no counterpart (its job is one chain)."""
    job = getattr(job_or_chains, "_job", job_or_chains)
    return job.engine.rhat(split=split, comm=comm)["rhat"]


def _pooled_ess(job_or_chains, split, maxlag, comm):
    job = getattr(job_or_chains, "_job", job_or_chains)
    if job.acov_maxlag > 0 and not split and maxlag is None:
        return job.engine.pooled_ess("streamed", None, comm)
    return job.engine.pooled_ess("split" if split else "history", maxlag, comm)


def pooled_ess(job_or_chains, split: bool = False, maxlag=None, comm=None) -> dict:
    """The pooled (multi-chain) effective sample size per dimension over all chains of a job, formed on the device (Engine.pooled_ess): how many
    independent draws the chains together are worth — the number to report beside rhat.  From the autocovariances kept while sampling when the job was
    built with acov_maxlag and neither split nor maxlag is given; otherwise from the stored history (window maxlag, None: min(127, n - 1)), with
    split=True over every chain's two halves.  `comm`: a klara_comm handle, to take every rank's chains.  Returns Engine.pooled_ess's dict: look at
    window_exhausted before quoting ess.  The reference has no counterpart (its ess is per chain)."""
    return _pooled_ess(job_or_chains, split, maxlag, comm)


def pooled_iact(job_or_chains, split: bool = False, maxlag=None, comm=None) -> np.ndarray:
    """The integrated autocorrelation time tau of pooled_ess's call: ess = (chains x saved steps) / tau."""
    return _pooled_ess(job_or_chains, split, maxlag, comm)["tau"]


def pooled_cor(job_or_chains, comm=None) -> np.ndarray:
    """The correlations of pooled_cov: cov_ij / sqrt(cov_ii cov_jj) (NaN where a coordinate never moved)."""
    c = pooled_cov(job_or_chains, comm)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.diag(c))
        return c / np.outer(sd, sd)


def acceptance(chains: MuvChains, diagnostics: bool = True) -> np.ndarray:
    """acceptance(s::MultivariateParameterNState; key=:accept) — stats/acceptance.jl:28-34:
    mean of the accept diagnostics over the saved steps (per chain)."""
    if isinstance(chains._job.sampler, MuvAMWG):
        # MuvAMWG: a rate per coordinate — the accepted proposals of every coordinate since the start state over the transitions done (nchains x D)
        eng = chains._job.engine
        return eng.amwg_state()[2].astype(np.float64) / float(max(eng.accept_counts()[1], 1))
    if chains._acc is None:
        raise ValueError("request outopts diagnostics=['accept'] to record the accept diagnostics")
    return chains._acc.mean(axis=0)


# ------------------------------------------------------------------ random streams of jobs
# Determinism contract.  A job's noise is a pure function of (seed, global chain id, transition index) — Philox4x32-10, key =
# seed (csrc/detmath.h) — so an explicit `seed=` reproduces a job bit for bit on any number of GPUs.  Klara's own jobs draw from
# Julia's global, unseeded generator: two jobs built the same way are independent (`run([job1, job2])`, jobs.jl:212).  To keep
# that, a job built WITHOUT `seed=` takes a fresh key: splitmix64 of (a per-process random base from os.urandom + a counter), so
# chain c of one job never shares its stream with chain c of another; `job.seed` reports the key that was used.  The keys are
# HASHED, not an arithmetic progression: `reset(job)` moves a job to seed + k * KLARA_EPOCH_KEY_STRIDE (include/klara_hip.h), and a
# progression of default keys with that same stride would make job i after k resets replay job i + k.
_SEED_BASE = int.from_bytes(os.urandom(8), "little")
_seed_counter = 0
_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _next_job_seed() -> int:
    global _seed_counter
    _seed_counter += 1
    return _splitmix64((_SEED_BASE + _seed_counter) & _M64)


# ------------------------------------------------------------------ job (src/jobs/BasicMCJob.jl)
class BasicMCJob:
    """BasicMCJob(model, sampler, range, v0; tuner=VanillaMCTuner(), outopts=...) — BasicMCJob.jl:107-185.

    outopts keys follow jobs.jl:9-43: destination in {"nstate", "none"}, monitor (["value"]),
    diagnostics ([] or ["accept"]).  Extra keyword arguments pick the shard: `chain_offset` (global id of
    the first chain), `device`, `seed` (default: a fresh key per job, see "random streams of jobs" above), `steps_per_launch`; `bm_batchlen` > 0 keeps streaming batch means so that
    `chain_mcvar(chain, "bm", bm_batchlen)` needs no stored history (destination "none"); `acov_maxlag` > 0 does the same for
    `chain_mcvar(chain, "imse" | "ipse", maxlag=acov_maxlag)` (autocovariances accumulated while sampling); `covariance=True` accumulates the
    pooled D x D cross-products of all chains' saved samples on the matrix cores (`pooled_cov`, `pooled_cor`), again with no stored history;
    `marginals=Marginals(nbins, lo, hi)` counts every dimension's saved samples into bins (`pooled_hist`, `pooled_quantiles`), likewise.
    `derived=Derived(nout, source, data, marginals)` evaluates a user function of the state on every saved sample of every chain and sums its outputs
    (`derived_mean`, `derived_var`, `derived_rhat`, `derived_quantiles`), likewise.
    """

    def __init__(self, model: GenericModel, sampler: MCSampler, mcrange: BasicMCRange, v0: Dict[str, Sequence],
                 tuner: Optional[MCTuner] = None, outopts: Optional[dict] = None, *, seed: Optional[int] = None,
                 chain_offset: int = 0, device: int = 0, steps_per_launch: int = 0, summaries: bool = True,
                 bm_batchlen: int = 0, acov_maxlag: int = 0, sparse_moves: int = 0, covariance: bool = False, marginals=None, derived=None):
        self.model, self.sampler, self.range = model, sampler, mcrange
        self.seed = _next_job_seed() if seed is None else int(seed)
        seed = self.seed
        self.tuner = tuner if tuner is not None else VanillaMCTuner()
        self.outopts = dict(outopts) if outopts is not None else {}
        self.outopts.setdefault("destination", "nstate")              # jobs.jl:10
        if self.outopts["destination"] != "none":
            self.outopts.setdefault("monitor", ["value"])             # jobs.jl:13-15
            self.outopts.setdefault("diagnostics", [])                # jobs.jl:37-39
        if self.outopts["destination"] not in ("nstate", "iostream", "none"):
            raise ValueError("outopts destination must be nstate, iostream or none")
        if self.outopts["destination"] == "iostream":                  # jobs.jl:17-29
            self.outopts.setdefault("filepath", "")
            self.outopts.setdefault("filesuffix", "csv")
            self.outopts.setdefault("flush", False)
            # saved steps held on the device between two writes (a ring of that many columns): the sink streams, as the
            # reference's does (one write per saved step), instead of keeping the whole run in memory
            self.outopts.setdefault("chunk", 256)
        params = [v for v in model.vertices if isinstance(v, BasicContMuvParameter)]
        if len(params) != 1:
            raise ValueError("model must hold exactly one BasicContMuvParameter")
        self.parameter = params[0]
        x0 = np.asarray(v0[self.parameter.key] if self.parameter.key in v0 else v0[":" + self.parameter.key],
                        dtype=np.float64)
        x0 = np.atleast_2d(x0)
        nchains, ndims = x0.shape
        if ndims != self.parameter.target.ndims:
            raise ValueError("v0 has the wrong number of dimensions for the target")
        monitor = 0
        if "accept" in self.outopts.get("diagnostics", []):
            monitor |= L.MON_ACCEPT
        if self.outopts["destination"] in ("nstate", "iostream"):
            mon = [str(m).lstrip(":") for m in self.outopts.get("monitor", [])]
            known = {"value", "logtarget", "gradlogtarget", "loglikelihood", "logprior"}
            if set(mon) - known:
                raise NotImplementedError(f"monitor fields not kept on device: {sorted(set(mon) - known)}")
            if "value" in mon:
                monitor |= L.MON_HISTORY
            if "logtarget" in mon:
                monitor |= L.MON_HIST_LT
            if "gradlogtarget" in mon:
                monitor |= L.MON_HIST_GRAD
            if "loglikelihood" in mon or "logprior" in mon:          # iterate/MALA.jl:104-109: kept when the parameter has the closures
                if not getattr(self.parameter.target, "has_parts", False):
                    raise ValueError("loglikelihood / logprior can only be monitored for a parameter built from those closures")
                monitor |= L.MON_HIST_LLLP
        if summaries:
            monitor |= L.MON_SUMMARIES
        if covariance:                                                # the pooled D x D cross-products, accumulated while sampling (pooled_cov)
            monitor |= L.MON_COVARIANCE
        self.covariance = bool(covariance)
        kw = dict(sampler=sampler.kind, target=self.parameter.target, nchains=nchains, nsteps=mcrange.nsteps,
                  burnin=mcrange.burnin, thinning=mcrange.thinning, tuner=self.tuner.kind,
                  period=self.tuner.period, verbose=self.tuner.verbose, seed=seed, chain_offset=chain_offset,
                  device=device, monitor=monitor, steps_per_launch=steps_per_launch, bm_batchlen=int(bm_batchlen),
                  acov_maxlag=int(acov_maxlag), sparse_moves=int(sparse_moves), marginals=marginals, derived=derived,
                  hist_ring_cols=int(self.outopts["chunk"]) if self.outopts["destination"] == "iostream" else 0)
        self.bm_batchlen, self.acov_maxlag = int(bm_batchlen), int(acov_maxlag)
        if isinstance(sampler, MH) and sampler.kind == L.SAMPLER_MH_COV:               # MH.jl:63-66, the matrix form; the tuner only counts, as for MH
            if not isinstance(self.tuner, VanillaMCTuner):
                raise NotImplementedError("MH(Σ) is not tuned: only VanillaMCTuner (which counts proposals when verbose) is accepted")
            kw["mh_factor"] = sampler.factor
        elif isinstance(sampler, MH):
            kw["mh_sigma"] = sampler.sigma
        elif isinstance(sampler, (MALA, SMMALA)):
            kw["driftstep"] = sampler.driftstep
            if isinstance(sampler, SMMALA) and sampler.transform is not None:          # SMMALA.jl:167-168, iterate/SMMALA.jl:117-118
                if isinstance(self.parameter.target, LogisticTarget):
                    raise ValueError("SMMALA: SoftAbs is not applied to LogisticTarget, whose metric is positive definite by construction")
                kw["smmala_softabs"] = sampler.transform.a
        elif isinstance(sampler, RAM):                                                 # RAM.jl:94-111; the tuner only counts (iterate/RAM.jl:68-69)
            if not isinstance(self.tuner, VanillaMCTuner):
                raise NotImplementedError("RAM adapts by itself: only VanillaMCTuner (which counts proposals when verbose) is accepted")
            kw["ram_S0"], kw["ram_targetrate"], kw["ram_gamma"] = sampler.S0, sampler.targetrate, sampler.gamma
        elif isinstance(sampler, AM):                                                  # AM.jl:131-154; the tuner only counts (iterate/AM.jl:80-82)
            if not isinstance(self.tuner, VanillaMCTuner):
                raise NotImplementedError("AM adapts by itself: only VanillaMCTuner (which counts proposals when verbose) is accepted")
            kw["am_C0"], kw["am_corescale"], kw["am_minorscale"] = sampler.C0, sampler.corescale, sampler.minorscale
            kw["am_c"], kw["am_t0"] = sampler.c, sampler.t0
        elif isinstance(sampler, MuvAMWG):                                             # AMWG.jl:139-151 with RobertsRosenthalMCTuner.jl:84-97
            if tuner is None:
                self.tuner = RobertsRosenthalMCTuner()
                kw.update(tuner=self.tuner.kind, period=self.tuner.period, verbose=self.tuner.verbose)
            if not isinstance(self.tuner, RobertsRosenthalMCTuner):
                raise NotImplementedError("MuvAMWG is tuned by RobertsRosenthalMCTuner alone (AMWG.jl:165-170)")
            kw["amwg_logsigma0"], kw["targetrate"] = sampler.logsigma0, self.tuner.targetrate
        elif isinstance(sampler, HMC):
            kw["leapstep"], kw["nleaps"] = sampler.leapstep, sampler.nleaps
        elif isinstance(sampler, SliceSampler):
            kw["slice_widths"], kw["slice_stepout"] = sampler.widths, sampler.stepout
        if isinstance(self.tuner, DualAveragingMCTuner):
            if not isinstance(sampler, HMC):
                raise NotImplementedError("DualAveragingMCTuner is wired into HMC only (HMC.jl:124-133)")
            kw.update(targetrate=self.tuner.targetrate, da_nadapt=self.tuner.nadapt, da_eps0bar=self.tuner.eps0bar,
                      da_h0bar=self.tuner.h0bar, da_gamma=self.tuner.gamma, da_t0=self.tuner.t0, da_kappa=self.tuner.kappa)
        if isinstance(self.tuner, AcceptanceRateMCTuner):
            kw["targetrate"], kw["score_k"] = self.tuner.targetrate, self.tuner.score_k
            kw["tuner_score"] = self.tuner.score_kind
            kw["tuner_mode"] = L.TUNE_POOLED if self.tuner.mode == "pooled" else L.TUNE_PER_CHAIN
        if isinstance(self.tuner, RobertsRosenthalMCTuner) and not isinstance(sampler, MuvAMWG):
            raise NotImplementedError("RobertsRosenthalMCTuner is the tuner of MuvAMWG alone")
        self.engine = Engine(**kw)
        # initialize!(pstate, parameter, sampler, outopts): BasicMCJob.jl:73 (finite asserts on device)
        try:
            self.engine.set_state(x0)
        except L.KlaraError as e:
            if e.status == L.ERR_NONFINITE_INIT:
                raise AssertionError("Log-target (or its gradient) not finite: initial values out of support") from e
            raise
        self._ran = False

    def close(self):
        self.engine.close()


def run(job):
    """run(job::BasicMCJob) — BasicMCJob.jl:212-244; run(jobs::Vector) = map(run, jobs) — jobs.jl:212."""
    if isinstance(job, (list, tuple)):
        return [run(j) for j in job]
    if job.outopts["destination"] == "iostream":
        _run_to_iostream(job)
    else:
        job.engine.run(job.range.nsteps)
    job._ran = True
    return job


def _run_to_iostream(job: "BasicMCJob") -> None:
    """:destination => :iostream — CSV files per monitored field (jobs.jl:193-202; BasicContParamIOStream.jl:152-159), written
    WHILE the job runs: the device keeps a ring of outopts["chunk"] saved steps, the loop below runs until the ring is full (or
    the job is done), appends those steps to every chain's files and, with :flush, flushes them (jobs.jl:17-29) — the host
    memory a long job needs does not grow with its length (only the rows of the newly saved steps of the accept diagnostics are read
    back, klara_get_accept_rows; the device keeps one byte per transition and chain of them)."""
    from .iostream import ChainWriter
    eng = job.engine
    base = job.outopts.get("filepath", "") or "."
    suffix = job.outopts.get("filesuffix", "csv")
    chunk, thin = int(job.outopts["chunk"]), job.range.thinning
    has_v, has_lt, has_g = bool(eng.monitor & L.MON_HISTORY), bool(eng.monitor & L.MON_HIST_LT), bool(eng.monitor & L.MON_HIST_GRAD)
    has_acc, has_lllp = bool(eng.monitor & L.MON_ACCEPT), bool(eng.monitor & L.MON_HIST_LLLP)
    width = len(str(eng.nchains))
    writers = [ChainWriter(base if eng.nchains == 1 else os.path.join(base, f"chain_{c + 1:0{width}d}"), suffix, has_v, has_lt, has_g, has_acc, has_lllp)
               for c in range(eng.nchains)]
    post = np.asarray(job.range.postrange) - 1                    # 0-based transition index of every saved step
    written, done = 0, 0
    try:
        while done < job.range.nsteps:
            # transitions until `chunk` more steps have been saved (none are saved during burn-in)
            k = min(job.range.nsteps - done, max(1, (job.range.burnin - done) if done < job.range.burnin else chunk * thin))
            eng.run(k); done += k
            new = eng.saved_steps() - written
            if new <= 0:
                continue
            assert new <= chunk
            acc = None
            if has_acc:      # only the rows of the newly saved steps come back (not every transition since the start)
                first, last = int(post[written]), int(post[written + new - 1])
                acc = eng.accept_rows(first, last - first + 1)[::thin]
            for c, w in enumerate(writers):
                value = eng.chain(c)[:, -new:] if has_v else None
                lt, g = eng.chain_fields(c, has_lt, has_g) if (has_lt or has_g) else (None, None)
                ll, lp = eng.chain_likelihood_prior(c) if has_lllp else (None, None)
                w.append(value, None if lt is None else lt[-new:], None if g is None else g[:, -new:], None if acc is None else acc[:, c],
                         None if ll is None else ll[-new:], None if lp is None else lp[-new:])
                if job.outopts.get("flush", False):
                    w.flush()
            written += new
    finally:
        for w in writers:
            w.close()


def output(job: BasicMCJob) -> MuvChains:
    """output(job) — BasicMCJob.jl:279."""
    return MuvChains(job)


def reset(job: BasicMCJob, x=None):
    """reset(job[, x]) — BasicMCJob.jl:187-201."""
    if x is not None:
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    job.engine.reset(x)
    job._ran = False
    return job
