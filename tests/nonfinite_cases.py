"""Small jobs whose proposals are regularly NOT FINITE: a log-target of -inf or NaN, a Metropolis ratio or a Hamiltonian that overflows.

The parity cases of tests/cases.py are well scaled: no transition kernel ever proposes a point whose log-target, gradient, ratio or Hamiltonian is -inf or NaN.
Such proposals are ordinary in use (a divergent trajectory, an overflowing drift, an MH step far into a tail, a closure with bounded support), and DESIGN.md
section 2 fixes what happens then: a ratio of -inf or NaN rejects, after a rejection nothing of the proposal survives, a committed state is finite, and a chain
never influences another chain.  tests/test_nonfinite_host.py replays these jobs on the CPU (shipped oracle, literal oracle, NumPy mirror) and asserts that the
INPUTS do what they are here for (the coverage conditions, counted by the mirror's hook); tests/test_gpu_nonfinite.py runs them on the device.

How a job is made.  Every job has `hot` chains (the odd ones) and ordinary chains (the even ones), so that both kinds sit in every wavefront and in every tile of
16 chains that the matrix-core kernels share.  All numbers below were chosen on the CPU (oracle and mirror); none comes from a kernel.

  * the overflow sphere.  In a drawn direction u, `_edge` finds by bisection the largest scale at which the mirror's log-target is still finite: there the
    quadratic form, or one square or product inside it, reaches DBL_MAX.  A hot chain starts at sqrt(f) times that scale.
  * MH (mh_sigma is one vector for all chains): coordinate 0 carries a proposal scale S0 = 2e152, a hundredth of the sphere's radius.  A hot chain starts with
    coordinate 0 just inside the sphere (f = 0.9999 .. 0.999999: within a few S0), so a proposal that moves outward has lt' = -inf and one that moves inward is
    accepted; an ordinary chain starts 5 .. 12 S0 from the origin, far inside: it accepts about every second proposal (those that move inward) and never
    overflows.  Every accepted move is inward, so a hot chain leaves the edge within a few transitions: the MH jobs are 6 transitions long.  (The issue's recipe
    — a scale of 1e154 for everybody — leaves no chain that never sees an overflow, which its own first coverage condition asks for.)
  * HMC: a hot chain starts on the sphere with f = 0.8 .. 0.9999 and a step near the stiffest coordinate's stability limit (eps omega about 1).  The dynamics of
    a quadratic target are scale free, so it moves like any other chain where nothing overflows, and is rejected with -inf where the leapfrog's energy error
    crosses DBL_MAX.
  * MALA: with a stable step MALA's proposal x + (h/2) g contracts every direction of a Gaussian and its second quadratic sum stays below 0.6 of the energy, so
    nothing overflows.  The targets therefore have ONE stiff direction with h lambda / 2 a little above 2: the proposal over-relaxes it by a factor
    |1 - h lambda / 2| > 1, and a hot chain overflows or not with the share of its energy in that direction.  The other directions are far inside the stable
    range, so ordinary chains keep a usable acceptance.
  * the Gamma closure (bounded support; an explicit guard returns -inf in one variant and NaN in the other): hot chains start next to the boundary; the first
    coordinate has shape 1/2 (MH, MALA: the density rises towards it) or 1 (HMC: a constant gradient, no pole for a trajectory to amplify).
  * logistic regression: the MH recipe on coefficient 0 (the prior's sum of squares overflows); for MALA and HMC a per-chain start scale on it (GRADIENT_ONLY).

`why_no_nan`, `why_no_both`: a job must show a NaN (not only -inf) and five chains that both accept and see a non-finite proposal, unless its arithmetic cannot:
then the reason stands in that field, and profiles/nonfinite_proposals.txt lists it.

Jobs that cannot form a non-finite proposal are still here where the issue names them, held to conditions of their own (`screen_only`): MALA at D = 100,
h = 0.9 on the headline kernels (for the screen's gate and the kept drift means at 1e154) and MALA / HMC on the logistic targets (x'b = +-1e153 in a shared tile).
Infinite proposals (`_mh_inf`), the dual-averaging jobs and the layout kind each family must report stand with their jobs in jobs().
"""
from __future__ import annotations

import sys

import numpy as np

import cases
import klara_jl_amd as K
import numpy_mirror as M
import oracle_ffi as O
from klara_jl_amd import _lib as L

SEED = 20260927
DBL_MAX = sys.float_info.max
MONITOR = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_GRAD

# ---- the closure: a product of Gamma(a_i, 1) densities on x > 0, lt = sum (a_i - 1) log x_i - x_i, data = a.  The guard is explicit: outside the support the
# closure returns GUARD (-inf in one variant, NaN in the other) and never calls log.  The gradient is log's own formula (a_i - 1) / x_i - 1, finite wherever x_i != 0.
_SRC_GAMMA = r"""
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) if (!(x[i] > 0.0)) return GUARD;
    for (int i = 0; i < KLARA_D; ++i) s = s + ((data[i] - 1.0) * kd_log(x[i]) - x[i]);
    return s;
}
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    for (int i = 0; i < KLARA_D; ++i) g[i] = (data[i] - 1.0) / x[i] - 1.0;
}
"""
SRC_GAMMA_INF = _SRC_GAMMA.replace("GUARD", "(-__builtin_inf())")
SRC_GAMMA_NAN = _SRC_GAMMA.replace("GUARD", '__builtin_nan("")')

NO_NAN_SQUARES = ("lt' is a finite constant minus a sum of products of non-negative factors (for the logistic target plus a finite likelihood term): an overflow is "
                  "+inf in that sum and -inf in lt'; the ratio subtracts the finite lt, MALA adds a finite and subtracts a non-negative sum, HMC subtracts a "
                  "non-negative kinetic term: -inf throughout, no inf - inf and no 0 * inf; x' itself stays below 1e156")
NO_NAN_DENSE = ("the terms x_i (P x)_i of the dense form have both signs, so two overflows of opposite sign would be a NaN; a negative term is at most a third of "
                "the positive ones here, and it overflows only 1.8 sphere radii out, which neither a proposal scale that leaves the ordinary chains alone nor a "
                "stable step reaches (the mirror's hook counts 0 on the CPU)")
NO_BOTH_MALA = ("at 1e154 the proposal's noise sqrt(h) z is below half an ulp of x: a hot chain's proposal, and with it the decision, is a function of its state "
                "alone.  It accepts while its energy share in the stiff direction is below about a half (each accepted move raises the share), then repeats one "
                "rejected proposal for ever; that proposal overflows only if the new energy exceeds DBL_MAX, i.e. from a share above 0.8, which a chain that has "
                "just accepted does not have.  So a hot chain of a Gaussian MALA job either overflows from its first transition on or never")
NO_BOTH_HIER = ("a start from which a trajectory overflows has a frequency sqrt(w_alpha) that exceeds the stability limit 2 / eps by more than a hundred orders of "
                "magnitude: every trajectory of such a chain diverges, whatever the tuner does to its step within the job, so it never accepts; a start that "
                "is mild enough to accept does not overflow (log sigma_alpha itself escapes upwards in the first step and switches the force off)")
SCREEN_ONLY = ("MALA at h = 0.9 on -|x|^2: the proposal is 0.1 x + sqrt(h) z, so lt' >= lt - |z|^2-sized terms, the first sum is h |z|^2 / 2h and the second is "
               "0.5445 |x'|^2-sized: from a finite state no term of the ratio can reach DBL_MAX.  The job is here for the sure-rejection screen's gate T = 2^1000 "
               "(klara_mala_screen.h: beyond it the screen answers 'not certain') and for the kept drift means at |x| up to 1e154, not for the coverage quota")
GRADIENT_ONLY = ("the only term that can overflow is the prior's sum of squares, an oscillator of frequency 1 / sqrt(lambda): MALA's h / (2 lambda) and HMC's "
                 "eps / sqrt(lambda) are far inside the stable range, a coefficient of 1e153 moves inward only (noise and momentum are below half an ulp of it) and "
                 "the kinetic term stays below a tenth of DBL_MAX.  The job puts x'b = +-1e153 into the rows of a tile that ordinary chains share")
NO_LITERAL_LOGIT = ("literal mode takes log(1 + exp(x'b)) as the example writes it, which is +inf from x'b = 710 on: every start with a coefficient of 1e153 is "
                    "refused there.  The shipped arithmetic and the mirror (logaddexp) are finite; they are compared")
NO_NAN_GUARD = "the guard returns -inf: the ratio is -inf - lt and HMC's a is exp(-inf) = 0; the closure forms no other non-finite value at x != 0"


def gamma_mirror(a, guard):
    a = np.asarray(a, float)

    def lt(x):
        if not bool(np.all(x > 0.0)):
            return guard
        return float(np.sum((a - 1.0) * np.log(x) - x))

    return lt, (lambda x: (a - 1.0) / x - 1.0)


def _hot(n):
    return np.arange(n) % 2 == 1


def _edge(ltf, u):
    """the largest scale s (to a relative 1e-12) at which ltf(s u) is finite"""
    lo, hi = 1e140, 1e160
    with np.errstate(all="ignore"):
        for _ in range(80):
            mid = np.sqrt(lo) * np.sqrt(hi)
            lo, hi = (mid, hi) if np.isfinite(ltf(mid * u)) else (lo, mid)
    return lo


def _energy_starts(rng, n, d, ltf, flo, fhi, mu=None, stiff=None, every=8):
    """even chains ~ mu + N(0, I); odd chains on the overflow sphere, sqrt(f) of the edge with f ~ U(flo, fhi): chains every - 1, 2 every - 1, .. in a uniformly drawn direction,
    the other odd chains along +-`stiff` (the target's stiffest direction) where one is given -> (x0, x0 with the hot rows ordinary too)"""
    cool = rng.standard_normal((n, d)) + (0.0 if mu is None else mu[None, :])
    x0 = cool.copy()
    for k in np.flatnonzero(_hot(n)):
        u = rng.standard_normal(d)
        u /= np.sqrt(u @ u)
        along = stiff is not None and k % every != every - 1
        if along:
            u = rng.choice([-1.0, 1.0]) * stiff + 0.05 * u
        # (a drawn direction stays at 0.9 f: the dense form's terms have both signs, and a partial sum of the positive ones must not overflow at the start)
        x0[k] = u * (np.sqrt(rng.uniform(flo, fhi) * (1.0 if along else 0.9)) * _edge(ltf, u))       # (|mu| is far below one ulp of these values)
    return x0, cool


def _mh_starts(rng, n, d, ltf, s0, flo=0.9999, fhi=0.999999, inner=(5.0, 12.0)):
    """MH: coordinate 0 of a hot chain just inside the overflow sphere, of an ordinary chain at +-U(inner) s0; the other coordinates ~ N(0, I)"""
    cool = rng.standard_normal((n, d))
    cool[:, 0] = rng.choice([-1.0, 1.0], n) * rng.uniform(*inner, n) * s0
    x0 = cool.copy()
    e0 = np.zeros(d); e0[0] = 1.0
    hot = _hot(n)
    x0[hot, 0] = rng.choice([-1.0, 1.0], hot.sum()) * np.sqrt(rng.uniform(flo, fhi, hot.sum())) * _edge(ltf, e0)
    return x0, cool


def _job(sampler, target, n, nsteps, x0, cool, layout, mirror, *, why_no_nan="", why_no_both="", why_no_literal="", screen_only="", spl=(0, 3), bm=0,
         min_plain=0.25, gtol=1e-12, **kw):
    """why_no_nan / why_no_both / why_no_literal: the reason why the job cannot show a NaN / a chain that both accepts and sees a non-finite proposal / be
    replayed in literal mode; empty where it must.  screen_only: the reason why the job can form no non-finite value at all (the headline MALA job, which is
    here for the screen's gate).  spl: the steps_per_launch values the device runs it with."""
    # (rtol: the bound on X and lt against literal mode, 1e-12; dual averaging: tests/test_gpu_literal.py's DUALAVG_RTOL = 1e-10, measured there oracle against
    # oracle — the step is exp(mu - sqrt(t) h_bar / gamma) of the continuous acceptance probability, so an ulp of dH is amplified and fed back)
    rtol = 1e-10 if kw.get("tuner") == L.TUNER_DUAL_AVERAGING else 1e-12
    gtol = max(gtol, rtol)
    return dict(kw=dict(sampler=sampler, target=target, **kw), n=n, nsteps=nsteps, x0=np.ascontiguousarray(x0), cool=np.ascontiguousarray(cool), hot=_hot(n),
                layout=tuple(layout), mirror=mirror, bm=bm, min_plain=min_plain, gtol=gtol, rtol=rtol, why_no_nan=why_no_nan, why_no_both=why_no_both,
                why_no_literal=why_no_literal, screen_only=screen_only, spl=tuple(spl))


S0 = 2e152          # MH: the proposal scale of coordinate 0
HIER_LOG_SIGMA = -300.0


def _gauss(J, prefix, target, mtarget, n, layout, rng, *, why, stiff, sigma=None, h=None, eps=None, nleaps=5, nsteps=12, mu=None, hmc_kw=None, bm_on=(), f=(0.9, 0.9999), hmc_every=4, nsteps_hmc=None):
    """MH (sigma given) / MALA (h given) / HMC (eps given) jobs on one Gaussian target"""
    d = target.ndims
    if sigma is not None:
        sg = np.array(sigma, float).copy(); sg[0] = S0
        x0, cool = _mh_starts(rng, n, d, mtarget[0], S0)
        J[prefix + "_mh"] = _job(L.SAMPLER_MH, target, n, 6, x0, cool, layout, ("mh", mtarget, dict(sigma=sg)), why_no_nan=why, mh_sigma=sg, bm=4 if "mh" in bm_on else 0)
    if h is not None:
        x0, cool = _energy_starts(rng, n, d, mtarget[0], *f, mu, stiff)
        J[prefix + "_mala"] = _job(L.SAMPLER_MALA, target, n, nsteps, x0, cool, layout, ("mala", mtarget, dict(driftstep=h)), why_no_nan=why, why_no_both=NO_BOTH_MALA, driftstep=h,
                                   bm=4 if "mala" in bm_on else 0)
    if eps is not None:
        x0, cool = _energy_starts(rng, n, d, mtarget[0], *f, mu, stiff, every=hmc_every)
        hk = dict(hmc_kw or {})
        mk = dict(leapstep=eps, nleaps=nleaps)
        if hk.get("tuner") == L.TUNER_ACCEPT_RATE:
            mk.update(tuner="rate", targetrate=hk["targetrate"], period=hk["period"], verbose=bool(hk.get("verbose")))
        J[prefix + "_hmc"] = _job(L.SAMPLER_HMC, target, n, nsteps_hmc or nsteps, x0, cool, layout, ("hmc", mtarget, mk), why_no_nan=why, leapstep=eps, nleaps=nleaps,
                                  bm=4 if "hmc" in bm_on else 0, **hk)


STIFF = 20.0


def _dense(d, seed):
    """a dense precision with entries of both signs and one stiff direction: cases.rank_one_precision (diagonal in [1, 2) plus three rank-one terms) plus
    STIFF v v' for a unit vector v — element-wise operations only, no matrix product; its largest eigenvalue is STIFF + v' B v, between 21 and 22.5"""
    rng = np.random.default_rng(seed)
    pm = cases.rank_one_precision(d, rng)
    v = rng.standard_normal(d)
    v /= np.sqrt(np.sum(v * v))
    pm = pm + STIFF * np.outer(v, v)
    return K.GaussDenseTarget(pm, const=0.75), M.dense_target(pm, np.zeros(d), 0.75), v


KIND_OF = {"group_": 0, "closure_": 0, "dense_d20": 1, "dense_d37": 1, "dense_d160": 1, "dense_d260": 6, "logit_swiss": 2, "pair_": 3, "hier_": 4, "logit_mfma": 5}
_cache = None


def jobs():
    """name -> job (built once per process; nothing here touches a device)"""
    global _cache
    if _cache is not None:
        return _cache
    rng = np.random.default_rng(SEED)
    J = {}
    # ---- kind 0, the group layout: a diagonal Gaussian of 7 dimensions (two lanes per chain, the second with a padding element).  sigma_0 = 0.5 is the stiff
    # coordinate: w_0 = 2, MALA's h w_0 = 2.1, HMC's eps omega_0 = 1.  HMC with the per-chain accept-rate tuner, verbose
    mu7, sg7 = np.linspace(-2.0, 3.0, 7), np.linspace(0.5, 2.0, 7)
    t7 = K.GaussDiagTarget.mvnormal(mu7, sg7)
    _gauss(J, "group_diag_d7", t7, M.diag_target(t7.w, t7.mu, t7.const), 130, O.default_layout(L.TARGET_GAUSS_DIAG, 7), rng, why=NO_NAN_SQUARES, stiff=np.eye(7)[0], sigma=0.8 * sg7, h=1.05,
           eps=0.5, mu=mu7, hmc_kw=dict(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.65, period=4, burnin=8, verbose=True), bm_on=("mala",))
    # ---- kind 0, run-time compiled whole-vector closure kernels: the Gamma product, D = 3, both guards
    n = 130
    lay3 = O.default_layout(L.TARGET_CUSTOM, 3)

    def gamma_starts(far, near):
        """coordinate 0 of an ordinary chain `far` from the boundary, of a hot chain at U(near)"""
        cool = np.abs(rng.standard_normal((n, 3))) * 0.5 + np.array([far, 3.0, 4.0])
        x0 = cool.copy()
        x0[_hot(n), 0] = rng.uniform(*near, _hot(n).sum())
        return x0, cool

    # shape 1/2 in coordinate 0 for MH and MALA (the density rises towards the boundary, the drift points at it); shape 1 for HMC: the density exp(-x) is
    # largest at the boundary and its gradient is the constant -1, so no trajectory amplifies the rounding of 1 / x next to the pole (literal mode's 1e-12)
    for tag, src, guard in (("inf", SRC_GAMMA_INF, -np.inf), ("nan", SRC_GAMMA_NAN, np.nan)):
        why = "" if tag == "nan" else NO_NAN_GUARD
        a = np.array([0.5, 4.0, 5.0])
        t, m = K.CustomTarget(3, src, a), gamma_mirror(a, guard)
        sg = np.array([0.5, 0.8, 0.8])
        x0, cool = gamma_starts(6.0, (0.05, 0.6))
        J[f"closure_gamma_{tag}_mh"] = _job(L.SAMPLER_MH, t, n, 12, x0, cool, lay3, ("mh", m, dict(sigma=sg)), why_no_nan=why, mh_sigma=sg)
        x0, cool = gamma_starts(12.0, (0.5, 2.5))
        J[f"closure_gamma_{tag}_mala"] = _job(L.SAMPLER_MALA, t, n, 8, x0, cool, lay3, ("mala", m, dict(driftstep=2.0)), why_no_nan=why, driftstep=2.0)
        a = np.array([1.0, 4.0, 5.0])
        t, m = K.CustomTarget(3, src, a), gamma_mirror(a, guard)
        x0, cool = gamma_starts(20.0, (0.3, 1.5))
        J[f"closure_gamma_{tag}_hmc"] = _job(L.SAMPLER_HMC, t, n, 8, x0, cool, lay3, ("hmc", m, dict(leapstep=1.8, nleaps=1)), why_no_nan=why,
                                             leapstep=1.8, nleaps=1)
        if tag == "nan":
            # dual averaging on a target that forms NaN: a = NaN reaches the tuner at every proposal outside the support.  It counts as 0 there (DESIGN.md
            # section 2, D1), so the step stays finite and the trip count round(lambda / eps) small: the host test asserts both, the device job compares
            # step, eps_bar and h_bar bit for bit.  (min_plain 0.10, the hierarchical job's bound: dual averaging starts from 10 x the step and settles near an
            # acceptance of 0.65 + within eight transitions, so fewer chains end inside 20 - 90 %; the job is here for the tuner's state.)  (Carried into h_bar, the first NaN would leave the chain with a NaN step and 65,536 leapfrogs per transition.)
            x0, cool = gamma_starts(60.0, (0.3, 1.5))
            J["closure_gamma_nan_hmc_dualavg"] = _job(L.SAMPLER_HMC, t, n, 12, x0, cool, lay3,
                                                      ("hmc", m, dict(leapstep=0.1, nleaps=10, tuner="da", targetrate=0.65, nadapt=8, gamma=0.5)), leapstep=0.1, nleaps=10,
                                                      tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.65, da_nadapt=8, da_gamma=0.5, min_plain=0.10)
    # ---- kind 1, dense tiles: D = 20 and the ragged D = 37 (16 chains share a tile of the matrix cores; 70 chains: four tiles and a ragged one of 6);
    # kind 1 streamed (D = 160) and kind 6, split over a workgroup (D = 260): MALA and HMC.  h lambda_max / 2 = 2.1 .. 2.25, eps sqrt(lambda_max) = 1.4
    for d, n in ((20, 70), (37, 70), (160, 37), (260, 37)):
        t, m, v = _dense(d, 2000 + d)
        _gauss(J, f"dense_d{d}", t, m, n, O.default_layout(L.TARGET_GAUSS_DENSE, d), rng, why=NO_NAN_DENSE, stiff=v, sigma=np.full(d, 0.25) if d < 100 else None, h=0.2, eps=0.44, nleaps=2, hmc_every=8,
               hmc_kw=dict(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.65, period=3, burnin=6), nsteps_hmc=9,
               bm_on=("mala",) if d == 37 else ())
    # ---- kind 3, pair-transposed: D = 18 (two pairs per lane, the last seven of them padding); sigma_0 = 0.3 is the stiff coordinate (w_0 = 5.56)
    mu18, sg18 = np.linspace(-1.0, 2.0, 18), np.concatenate([[0.3], np.linspace(0.4, 1.7, 17)])
    t18 = K.GaussDiagTarget.mvnormal(mu18, sg18)
    _gauss(J, "pair_diag_d18", t18, M.diag_target(t18.w, t18.mu, t18.const), 130, O.default_layout(L.TARGET_GAUSS_DIAG, 18, sampler=L.SAMPLER_MALA), rng,
           why=NO_NAN_SQUARES, stiff=np.eye(18)[0], sigma=0.5 * sg18, h=0.38, eps=0.36, nleaps=6, mu=mu18,
           hmc_kw=dict(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.65, period=3, burnin=6), nsteps_hmc=9)
    # ---- kind 2, logistic regression with the rows split over lanes (swiss, D = 4): MH
    X, y = cases.swiss_data()
    ts = K.LogisticTarget(X, y, 100.0)
    ms = M.logistic_target(X, y, 100.0)
    sg = np.full(4, 0.3); sg[0] = S0
    x0, cool = _mh_starts(rng, 130, 4, ms[0], S0)
    J["logit_swiss_mh"] = _job(L.SAMPLER_MH, ts, 130, 6, x0, cool, O.default_layout(L.TARGET_LOGISTIC, 4, ndata=X.shape[0], sampler=L.SAMPLER_MH),
                               ("mh", ms, dict(sigma=sg)), why_no_nan=NO_NAN_SQUARES, why_no_literal=NO_LITERAL_LOGIT, mh_sigma=sg)
    # ---- kind 5, logistic regression on the matrix cores (D = 20, 50 rows: the last row tile holds 2): MH and HMC
    X, y = cases.synthetic_logit(50, 20)
    tl = K.LogisticTarget(X, y, 10.0)
    ml = M.logistic_target(X, y, 10.0)
    lay5 = O.default_layout(L.TARGET_LOGISTIC, 20, ndata=50, sampler=L.SAMPLER_MH)
    sg = np.full(20, 0.15); sg[0] = S0
    x0, cool = _mh_starts(rng, 70, 20, ml[0], S0)
    J["logit_mfma_d20_mh"] = _job(L.SAMPLER_MH, tl, 70, 6, x0, cool, lay5, ("mh", ml, dict(sigma=sg)), why_no_nan=NO_NAN_SQUARES, why_no_literal=NO_LITERAL_LOGIT, mh_sigma=sg)
    # ---- kind 4, the hierarchical (rats) target: HMC with the per-chain accept-rate tuner.  A hot chain starts with log sigma_alpha = -300: w_alpha = exp(600)
    # kicks the unit intercepts to 1e257 within one step (and log sigma_alpha itself to 1e260, where w_alpha is 0), their squares overflow and 0 * inf is a NaN.
    # The tuner cuts such a chain's step by 0.021 every three rejections, which does not bring a displacement of eps^2 * 5e262 below 1e154 in 12 transitions
    tr = cases.rats_target()
    mr = M.hier_normal_target(tr.Y, tr.xc, tr.prior_prec, tr.gamma_a, tr.gamma_b)
    n = 37
    cool = tr.least_squares_start()[None, :] + 0.05 * rng.standard_normal((n, tr.ndims))
    x0 = cool.copy()
    x0[_hot(n), tr.ndims - 2] = HIER_LOG_SIGMA
    hk = dict(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.65, period=3, burnin=9)
    # (gtol: tests/test_gpu_literal.py's 1e-10 for this target's gradient, here chain by chain)
    J["hier_rats_hmc"] = _job(L.SAMPLER_HMC, tr, n, 12, x0, cool, O.default_layout(L.TARGET_HIER_NORMAL, tr.ndims, sampler=L.SAMPLER_HMC, hier_nunits=tr.Y.shape[0],
                                                                                 hier_ntimes=tr.Y.shape[1]),
                              ("hmc", mr, dict(leapstep=0.03, nleaps=16, tuner="rate", targetrate=0.65, period=3)), leapstep=0.03, nleaps=16, min_plain=0.10, gtol=1e-10, why_no_both=NO_BOTH_HIER, **hk)
    # ---- kind 3, D = 100 on -|x|^2: the headline kernels (MALA at h = 0.9 with the sure-rejection screen and the kept drift means), also with one transition per
    # launch.  MALA: every fourth chain (2, 6, 10, ..) starts at |x| = 2^498 .. 2^502, so that sum x^2 straddles the screen's gate 2^1000; the odd chains on the
    # overflow sphere as everywhere.  No proposal of this job can be non-finite (SCREEN_ONLY): what it holds the kernel to is (a), (b), (c) at those magnitudes
    t100 = K.GaussDiagTarget.negdot(100)
    m100 = M.diag_target(np.ones(100), np.zeros(100), 0.0)
    lay100 = O.default_layout(L.TARGET_GAUSS_DIAG, 100, sampler=L.SAMPLER_MALA)
    _gauss(J, "pair_negdot_d100", t100, m100, 130, lay100, rng, why=NO_NAN_SQUARES, stiff=np.eye(100)[0], sigma=np.full(100, 0.1), eps=0.35, nleaps=3,
           hmc_kw=dict(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.65, period=3, burnin=6), nsteps_hmc=9)
    x0, cool = _energy_starts(rng, 130, 100, m100[0], 0.9, 0.9999)
    for k in range(2, 130, 4):
        u = rng.standard_normal(100)
        x0[k] = u / np.sqrt(u @ u) * 2.0 ** rng.uniform(498.0, 502.0)
        cool[k] = x0[k]
    J["pair_negdot_d100_mala"] = _job(L.SAMPLER_MALA, t100, 130, 12, x0, cool, lay100, ("mala", m100, dict(driftstep=0.9)), screen_only=SCREEN_ONLY,
                                      why_no_nan=SCREEN_ONLY, why_no_both=SCREEN_ONLY, driftstep=0.9)
    for k in ("pair_negdot_d100_mh", "pair_negdot_d100_mala", "pair_negdot_d100_hmc"):
        J[k]["spl"] = (0, 1, 3)
    # ---- kind 3, D = 18: HMC with dual averaging, da_nadapt = 8.  With the default gamma = 0.05 a chain that rejects eight times has its step cut to 1e-6 of the
    # start and its trip count lambda / eps capped at 65,536 (seen on the CPU oracle: the job does not end in minutes); gamma = 0.5 keeps every step within a
    # factor of 5 of the start.  No a of this job is a NaN (NO_NAN_SQUARES: a = exp(-inf) = 0), so every step stays finite; the host test asserts both
    rda = np.random.default_rng(5)
    x0, cool = _energy_starts(rda, 130, 18, M.diag_target(t18.w, t18.mu, t18.const)[0], 0.9, 0.9999, mu18, np.eye(18)[0], every=4)
    J["pair_diag_d18_hmc_dualavg"] = _job(L.SAMPLER_HMC, t18, 130, 12, x0, cool, O.default_layout(L.TARGET_GAUSS_DIAG, 18, sampler=L.SAMPLER_HMC),
                                          ("hmc", M.diag_target(t18.w, t18.mu, t18.const), dict(leapstep=0.1, nleaps=5, tuner="da", targetrate=0.65, nadapt=8, gamma=0.5)),
                                          why_no_nan=NO_NAN_SQUARES, leapstep=0.1, nleaps=5, tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.65, da_nadapt=8, da_gamma=0.5)
    # ---- an INFINITE proposal (an MH step far into a tail), kinds 1, 3 and 0.  Coordinate 1 is a flat direction of the target (its row and column of the
    # precision, its diagonal weight, are exactly 0) and carries a proposal scale of 3e307 (dense) / 4e152 (diagonal).  An ordinary chain's coordinate 1 wanders
    # at that scale and enters nothing: 0 * finite = 0.  A hot chain starts it at 0.95 .. 0.999 of DBL_MAX (diagonal: of sqrt(DBL_MAX), where the square
    # overflows): a step outward is +-inf, and 0 * inf is a NaN in every row of P x' (in w (x' - mu)^2) — the product of a zero with an infinity that padded
    # and ragged tiles are exposed to — so lt' is NaN and the proposal is rejected; a step inward is an ordinary proposal, decided by the other coordinates
    for d in (20, 37):
        t, m, v = _dense(d, 2000 + d)
        pm = t.precision.copy()
        pm[1, :] = 0.0
        pm[:, 1] = 0.0
        tf, mf = K.GaussDenseTarget(pm, const=0.75), M.dense_target(pm, np.zeros(d), 0.75)
        sg = np.full(d, 0.12); sg[1] = 3e307
        cool = rng.standard_normal((70, d)) * 0.5
        x0 = cool.copy()
        x0[_hot(70), 1] = rng.choice([-1.0, 1.0], 35) * rng.uniform(0.98, 0.9999, 35) * DBL_MAX
        J[f"dense_d{d}_mh_inf"] = _job(L.SAMPLER_MH, tf, 70, 8, x0, cool, O.default_layout(L.TARGET_GAUSS_DENSE, d), ("mh", mf, dict(sigma=sg)), mh_sigma=sg)
    for name, tg, mu_, sg_, lay in (("pair_diag_d18_mh_inf", t18, mu18, sg18, O.default_layout(L.TARGET_GAUSS_DIAG, 18, sampler=L.SAMPLER_MH)),
                                    ("group_diag_d7_mh_inf", t7, mu7, sg7, O.default_layout(L.TARGET_GAUSS_DIAG, 7))):
        d = tg.ndims
        w = tg.w.copy(); w[1] = 0.0
        tf = K.GaussDiagTarget(d, w=w, mu=tg.mu.copy(), const=tg.const)
        sg = 0.5 * sg_; sg[1] = 4e152
        cool = rng.standard_normal((130, d)) * sg_ + mu_
        x0 = cool.copy()
        x0[_hot(130), 1] = rng.choice([-1.0, 1.0], 65) * rng.uniform(0.98, 0.9999, 65) * np.sqrt(DBL_MAX)
        J[name] = _job(L.SAMPLER_MH, tf, 130, 8, x0, cool, lay, ("mh", M.diag_target(w, tg.mu, tg.const), dict(sigma=sg)), mh_sigma=sg)
    # ---- logistic regression with gradients beside hot chains (kind 2: MALA; kind 5: MALA and HMC).  The issue's recipe, a per-chain start scale on
    # coefficient 0: a hot chain starts it at 1e153, so that its x'b is +-1e153 in every data row of the tile it shares with 15 other chains.  No proposal
    # of these jobs can be non-finite (GRADIENT_ONLY), so like the headline MALA job they are held to conditions of their own on the host
    for name, tg, mg, n, lay, smp, ck, kw, scale in (
            ("logit_swiss_mala", ts, ms, 130, O.default_layout(L.TARGET_LOGISTIC, 4, ndata=200, sampler=L.SAMPLER_MALA), L.SAMPLER_MALA, dict(driftstep=0.1), dict(driftstep=0.1), None),
            ("logit_mfma_d20_mala", tl, ml, 70, lay5, L.SAMPLER_MALA, dict(driftstep=0.1), dict(driftstep=0.1), 0.1),
            ("logit_mfma_d20_hmc", tl, ml, 70, lay5, L.SAMPLER_HMC, dict(leapstep=0.15, nleaps=4), dict(leapstep=0.15, nleaps=4), 0.1)):
        d = tg.ndims
        cool = (np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * rng.standard_normal((n, d))) if scale is None else scale * rng.standard_normal((n, d))
        x0 = cool.copy()
        x0[_hot(n), 0] = rng.choice([-1.0, 1.0], _hot(n).sum()) * rng.uniform(0.5, 2.0, _hot(n).sum()) * 1e153
        J[name] = _job(smp, tg, n, 12, x0, cool, lay, ("mala" if smp == L.SAMPLER_MALA else "hmc", mg, ck), screen_only=GRADIENT_ONLY, why_no_nan=GRADIENT_ONLY,
                       why_no_both=GRADIENT_ONLY, why_no_literal=NO_LITERAL_LOGIT, **kw)
    # the layout kind the issue's table names for each family, as literals: a job that drifts to another kernel family with the layout mirror fails here
    for name, job in J.items():
        job["kind"] = next(k for prefix, k in KIND_OF.items() if name.startswith(prefix))
        assert job["layout"][0] == job["kind"], (name, job["layout"])
    _cache = J
    return J
