"""The run-time compiled closure kernels over every plan shape — TEST INFRASTRUCTURE shared by tests/test_closure_sweep_host.py (no GPU) and
tests/test_gpu_closure_sweep.py (-m gpu).

A whole-vector closure beyond 32 dimensions runs staged through LDS (klara.jl_amd/csrc/klara_custom.h): its plan is (G lanes per chain, E elements per
lane, wavefronts per workgroup `wpb`) plus a 2-double pad on a chain's row stride wherever (2 stride) % 64 == 0 (klara_plan.h custom_layout /
custom_stage_bytes).  `plan` is oracle_ffi.staged_plan — the arithmetic default_layout itself runs —, `classes` the distinct plans over D = 33 .. 1024, and the
dimension tables below name one job per class.  The host file proves that the tables cover the classes and that every job's steps are sane on the oracle
alone; the GPU file runs them bit for bit."""
from __future__ import annotations

import numpy as np

import autodiff_cases as A
import cases
import klara_jl_amd as K
import oracle_ffi as O
from klara_jl_amd import _lib as L

LDS_BYTES = 57344          # klara_launch.h KLARA_LDS_DEFAULT_DYNAMIC: the dynamic LDS a launch gets without asking
DIMS = range(33, 1025)     # the staged form's dimensions


def plan(d, rows):
    """(G, E, wpb, padded) of a staged closure with `rows` vectors per chain in LDS (2: x and gradient; 3: the likelihood + prior form)"""
    return O.staged_plan(d, rows)[:4]


def stage_bytes(d, rows):
    """dynamic LDS of the plan's workgroup: wpb wavefronts x 64 / G chains x stride doubles"""
    g, _, wpb, _, stride = O.staged_plan(d, rows)
    return wpb * (64 // g) * stride * 8


def classes(rows):
    """{(G, E, wpb, padded): [every D of 33 .. 1024 with that plan]} in order of first appearance"""
    out = {}
    for d in DIMS:
        out.setdefault(plan(d, rows), []).append(d)
    return out


def nchains(d, rows):
    """one full workgroup, one full wavefront of a second, one chain in a third"""
    g, _, wpb, _ = plan(d, rows)
    return wpb * (64 // g) + 64 // g + 1


# ---- the coupled likelihood + prior closure: cases.SRC_QUARTIC_CHAIN split into its site terms (likelihood) and its coupling term (prior).  Both the
# value and the prior's gradient row read neighbours across lane boundaries.  ll + lp = -s + -(k/2 t) has the bits of the whole-vector closure's
# -s - (k/2) t; gll + glp is another rounding than its gradient (one addition of two rows instead of one chain of additions), so the jobs differ.
QC_DATA = np.array([0.05, 0.4])
SRC_QC_LL = r"""
/* the site terms of cases.SRC_QUARTIC_CHAIN: ll = -sum_i (x_i^2 / 2 + c x_i^4), data = [c, k] */
KLARA_USER_FN double klara_user_loglikelihood(const double* x, int D, const double* data, long long ndata)
{
    const double c = data[0];
    double s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const double q = x[i] * x[i]; s = s + (0.5 * q + c * (q * q)); }
    return -s;
}
"""
SRC_QC_LP = r"""
/* its coupling term: lp = -k/2 sum_i (x_{i+1} - x_i)^2 */
KLARA_USER_FN double klara_user_logprior(const double* x, int D, const double* data, long long ndata)
{
    const double k = data[1];
    double t = 0.0;
    for (int i = 0; i + 1 < KLARA_D; ++i) { const double d = x[i + 1] - x[i]; t = t + d * d; }
    return -((0.5 * k) * t);
}
"""
SRC_QC_GLL = r"""
KLARA_USER_FN void klara_user_gradloglikelihood(const double* x, int D, const double* data, long long ndata, double* g)
{
    const double c = data[0];
    for (int i = 0; i < KLARA_D; ++i) { const double q = x[i] * x[i]; g[i] = -(x[i] + (4.0 * c) * (q * x[i])); }
}
"""
SRC_QC_GLP = r"""
KLARA_USER_FN void klara_user_gradlogprior(const double* x, int D, const double* data, long long ndata, double* g)
{
    const double k = data[1];
    for (int i = 0; i < KLARA_D; ++i) {
        double v = 0.0;
        if (i + 1 < KLARA_D) v = v + k * (x[i + 1] - x[i]);
        if (i > 0) v = v - k * (x[i] - x[i - 1]);
        g[i] = v;
    }
}
"""
AD_QC_LL = r"""
/* closure_sweep.SRC_QC_LL, generic in its scalar type */
template <class T, class V>
KLARA_USER_FN T klara_user_loglikelihood_ad(const V& x, int D, const double* data, long long ndata)
{
    const double c = data[0];
    T s = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { const T q = x[i] * x[i]; s = s + (0.5 * q + c * (q * q)); }
    return -s;
}
"""
AD_QC_LP = r"""
template <class T, class V>
KLARA_USER_FN T klara_user_logprior_ad(const V& x, int D, const double* data, long long ndata)
{
    const double k = data[1];
    T t = 0.0;
    for (int i = 0; i + 1 < KLARA_D; ++i) { const T d = x[i + 1] - x[i]; t = t + d * d; }
    return -((0.5 * k) * t);
}
"""
# a SEPARABLE likelihood + prior pair (no element reads another): what the coupled closure is compared with in the host file's worked example
SRC_SEP_LP = r"""
KLARA_USER_FN double klara_user_logprior(const double* x, int D, const double* data, long long ndata)
{
    const double k = data[1];
    double t = 0.0;
    for (int i = 0; i < KLARA_D; ++i) t = t + x[i] * x[i];
    return -((0.5 * k) * t);
}
"""
SRC_SEP_GLP = r"""
KLARA_USER_FN void klara_user_gradlogprior(const double* x, int D, const double* data, long long ndata, double* g)
{
    const double k = data[1];
    for (int i = 0; i < KLARA_D; ++i) g[i] = -(k * x[i]);
}
"""

QUARTIC_LT_ONLY = cases.SRC_QUARTIC_CHAIN[:cases.SRC_QUARTIC_CHAIN.index("KLARA_USER_FN void")]      # MH / slice need no gradient closure


def coupled_target(d, gradients=True):
    """the coupled likelihood + prior closure as a CustomTarget (three rows of LDS per chain)"""
    return K.CustomTarget.likelihood_prior(d, SRC_QC_LL, SRC_QC_LP, SRC_QC_GLL if gradients else "", SRC_QC_GLP if gradients else "", QC_DATA)


def separable_target(d):
    return K.CustomTarget.likelihood_prior(d, SRC_QC_LL, SRC_SEP_LP, SRC_QC_GLL, SRC_SEP_GLP, QC_DATA)


def quartic_target(d, gradients=True):
    return K.CustomTarget(d, cases.SRC_QUARTIC_CHAIN if gradients else QUARTIC_LT_ONLY, QC_DATA)


# ---- the sweep's tables: (D, sampler / tuner).  One row per plan class (tests/test_closure_sweep_host.py holds them to `classes`).
GRADIENT_KINDS = ("mala", "hmc", "mala_pooled", "hmc_da", "hmc_rate")
# (a) two rows — the quartic chain —: the 24 (G, E, wpb) classes; the stride pad cannot occur (2 dp + 2 = 0 mod 32 needs an odd dp)
TWO_ROW_JOBS = [(33, "mala"), (47, "mh"), (54, "hmc"), (55, "slice"), (79, "mala_pooled"), (96, "hmc_da"), (109, "hmc_rate"), (111, "mala"), (127, "hmc"),
                (129, "mala_pooled"), (177, "mh"), (222, "hmc_da"), (223, "hmc_rate"), (255, "mala"), (319, "hmc"), (383, "slice"), (385, "mala_pooled"),
                (448, "hmc_da"), (511, "hmc_rate"), (513, "mala"), (767, "hmc"), (893, "mala_pooled"), (895, "hmc_da"), (1023, "hmc_rate")]
# (b) three rows — the coupled likelihood + prior closure —: the 23 (G, E, wpb) classes at a padded D wherever the class has one, and an unpadded
# neighbour for every class that has both (40 plans in all)
THREE_ROW_JOBS = [(35, "mala"), (41, "hmc"), (43, "mh"), (57, "slice"), (71, "mala_pooled"), (73, "hmc_da"), (77, "hmc_rate"), (95, "mala"), (105, "hmc"),
                  (107, "mala_pooled"), (128, "hmc_da"), (138, "hmc_rate"), (139, "mh"), (159, "mala"), (169, "hmc"), (171, "mala_pooled"), (202, "hmc_da"),
                  (203, "hmc_rate"), (233, "mala"), (256, "hmc"), (265, "mala_pooled"), (267, "slice"), (297, "hmc_da"), (299, "hmc_rate"), (362, "mala"),
                  (363, "hmc"), (393, "mala_pooled"), (395, "hmc_da"), (490, "hmc_rate"), (491, "mala"), (521, "hmc"), (523, "hmc_da"), (617, "hmc_da"),
                  (619, "hmc_rate"), (746, "mala"), (747, "hmc"), (777, "mala_pooled"), (779, "mala_pooled"), (1002, "hmc_rate"), (1003, "mala")]
# (c) the same job at 2 and at 4 wavefronts per workgroup: (rows, D, sampler) of three classes whose rows fit at both, G = 8, 16 and 64 (the last one padded)
WPB_JOBS = [(3, 70, "mala"), (2, 200, "hmc"), (3, 553, "mala")]
# (d) staged forward-mode autodiff: (rows, D, sampler, chunksize) — the quartic chain's generic form at E = 8, 10 (G = 64), 12 (and again at a chunk of 5),
# 14 and 16 (both at wpb = 2); the likelihood + prior form at E = 6, E = 16 and at a padded D
AD_JOBS = [(2, 60, "hmc", 0), (2, 600, "mala", 0), (2, 45, "hmc", 0), (2, 45, "hmc", 5), (2, 224, "mala", 0), (2, 120, "hmc", 0),
           (3, 40, "mala", 0), (3, 118, "hmc", 0), (3, 106, "mala", 0)]
AD_EXPECTED = {(2, 60): (8, 8, 4), (2, 600): (64, 10, 4), (2, 45): (4, 12, 4), (2, 224): (16, 14, 2), (2, 120): (8, 16, 2),
               (3, 40): (8, 6, 4), (3, 118): (8, 16, 2), (3, 106): (8, 14, 2)}
# (e) pair closures on the few-lanes kernels (k_diagt<.., USERPAIR>, layout kind 3)
PAIR_DIMS = [17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97, 100, 104, 127, 128, 129, 255, 256, 257, 511, 512, 513, 777, 1023, 1024]
PAIR_JOBS = [(d, "mala") for d in PAIR_DIMS] + [(d, s) for s in ("hmc", "mh", "slice") for d in PAIR_DIMS[::3]]


# ---- step sizes: a rule in D (the named cases' driftstep ~ D^(-1/3), leapstep ~ D^(-1/4); MH's sigma ~ D^(-1/2)), held to 5 % .. 95 % acceptance on the
# oracle alone by tests/test_closure_sweep_host.py
def driftstep(d):
    return 0.7 / d ** (1.0 / 3.0)


def leapstep(d):
    return 0.8 / d ** 0.25


def mh_sigma(d):
    return np.full(d, 0.9 / np.sqrt(d))


NLEAPS = 3


def _sampler_kw(kind, d, nsteps):
    if kind == "slice":
        return dict(sampler=L.SAMPLER_SLICE, slice_widths=np.linspace(0.8, 2.0, d), slice_stepout=True)
    if kind == "mh":
        return dict(sampler=L.SAMPLER_MH, mh_sigma=mh_sigma(d))
    if kind.startswith("mala"):
        kw = dict(sampler=L.SAMPLER_MALA, driftstep=driftstep(d))
        if kind == "mala_pooled":
            kw.update(tuner=L.TUNER_ACCEPT_RATE, tuner_mode=L.TUNE_POOLED, targetrate=0.574, period=4)
        return kw
    kw = dict(sampler=L.SAMPLER_HMC, leapstep=leapstep(d), nleaps=NLEAPS)
    if kind == "hmc_rate":
        kw.update(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.6, period=4)
    if kind == "hmc_da":
        kw.update(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.65, da_nadapt=9)
    return kw


def staged_case(rows, d, kind, target=None, n=None):
    """one sweep job of (a) - (d): Engine keyword arguments + "x0" + "name" (cases.engine_kwargs / cases.oracle_kwargs take it)"""
    nograd = kind in ("mh", "slice")
    if target is None:
        target = (coupled_target if rows == 3 else quartic_target)(d, gradients=not nograd)
    n = nchains(d, rows) if n is None else n
    nsteps = (4 if d <= 512 else 3) if kind == "slice" else (10 if d > 512 else 12)      # (a slice transition is D x ~6 full evaluations on the oracle's side)
    c = dict(target=target, nchains=n, nsteps=nsteps, burnin=(1 if kind == "slice" else 2), thinning=2, seed=20261020 + d,
             x0=0.5 * np.random.default_rng(1000 * rows + d).standard_normal((n, d)), name=f"sweep{rows}_{kind}_d{d}", **_sampler_kw(kind, d, nsteps))
    return c


def ad_case(rows, d, kind, chunksize=0):
    text = AD_QC_LL + AD_QC_LP if rows == 3 else A.AD_QUARTIC_CHAIN
    target = K.CustomTarget(d, A.marked(text, 1, chunksize, parts=(rows == 3)), QC_DATA)
    return dict(staged_case(rows, d, kind, target=target), name=f"sweep{rows}_ad_{kind}_d{d}_c{chunksize}")


def pair_case(d, kind):
    """(e): 11 chains, 6 transitions; MALA alternates the pair-coupled quartic and the coordinate-indexed target along PAIR_DIMS"""
    indexed = PAIR_DIMS.index(d) % 2 == 1
    target = (K.CustomTarget.pairwise(d, cases.SRC_PAIR_INDEXED, np.linspace(0.5, 2.0, d)) if indexed
              else K.CustomTarget.pairwise(d, cases.SRC_PAIR_QUARTIC, QC_DATA))
    kw = _sampler_kw(kind, d, 6)
    if kind == "slice":
        kw["slice_widths"] = np.full(d, 1.5)
    return dict(target=target, nchains=11, nsteps=6, burnin=0, seed=d, x0=0.5 * np.random.default_rng(7000 + d).standard_normal((11, d)),
                name=f"pair_{kind}_d{d}", **kw)


def pair_lanes(d):
    return 8 if d <= 128 else 16 if d <= 256 else 32 if d <= 512 else 64


def monitor(case, lllp=False):
    nograd = case["sampler"] in (L.SAMPLER_MH, L.SAMPLER_SLICE)
    m = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT | (0 if nograd else L.MON_HIST_GRAD)
    return m | (L.MON_HIST_LLLP if (lllp and not nograd) else 0)


def oracle_alone(case, layout, ad=False):
    """the job on the CPU reference only: (status, acceptance, job)"""
    import autodiff_ref as R
    job = (R.ref_job(case, layout=layout, want_hist=True) if ad else O.OracleJob(**cases.oracle_kwargs(case, layout=layout), want_hist=True))
    assert job.set_state(case["x0"]) == 0
    st = job.run(case["nsteps"])
    return st, float(job.accept.mean()), job
