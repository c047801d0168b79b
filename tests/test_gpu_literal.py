"""The HIP path against the LITERAL Julia arithmetic and against the independent NumPy mirror — on the GPU box, at the BASELINE sizes.

Why this file exists.  Every other `-m gpu` parity test compares the kernels with the shipped mode of
oracle/klara_oracle.c, which shares a few deliberate deviations from the literal Julia expressions with the kernels (DESIGN.md section 2:
merged fma leapfrog, abs2(.)*(0.5/h), one exponential per logistic row, the slice sampler's difference-form comparison) and the library's
own transcendental functions (detmath.h).  Two other checkers exist that do NOT move with the kernels:

  * the oracle's LITERAL mode (`ko_set_literal(1)`): the arithmetic exactly as the reference writes it — leapfrog! as four unmerged,
    unfused updates (/root/reference/src/samplers/samplers.jl:122-134), 0.5*(abs2.(..)/step) (src/samplers/iterate/MALA.jl:88-92), both
    exponentials of the swiss example (doc/examples/swiss/MALA/analytical.jl:13,17), and a full log-target evaluation for every probe of
    the slice sampler compared with log(rand()) + lt (src/samplers/iterate/SliceSampler.jl:66-95);
  * tests/numpy_mirror.py: a second restatement of the same Julia sources in plain Python / NumPy that shares no code with the oracle or
    with detmath.h (its own Philox, libm transcendentals, NumPy sums).

Here the full-size GPU jobs of BASELINE cfg 2 (h = 0.9 as stated, and a step that mixes), cfg 3, cfg 4 (one GPU's share), cfg 5 without the
pooled tuner (one GPU's share), the slice sampler at D = 100 and (round 5's new kernels) the slice sampler on dense precisions of 100 and 160 dimensions are run through the C ABI, and three blocks of 16 chains (first, across the
chain-partition boundary / middle, the ragged last wavefront group) are replayed by the literal-mode oracle; one block of 8 chains is
replayed by the NumPy mirror.  Asserted: EVERY accept decision of every transition identical, final states / log-targets within 1e-12
relative (literal) resp. 1e-9 (mirror: libm vs table functions, NumPy's pairwise sums).  A change of the kernels' arithmetic or of the
random stream that moved a single decision away from the literal Julia arithmetic fails here whatever the shipped oracle does.

The newer kernel families (NEW_JOB_NAMES).  The jobs above are the kernels of the early rounds.  Everything written since was compared with the shipped oracle
only, whose branches were written with the kernels and share their summation orders per layout kind, and the golden fixtures of layout kind 6 were regenerated when
its tile deal changed: a kernel and its oracle branch that are wrong in the same way stayed green.  The same machinery now runs, full size, on: the workgroup-split
dense layout (kind 6: HMC D = 512, MALA D = 1024 with a mean, MH D = 700 with a mean, the slice sampler D = 260, HMC D = 300 with dual averaging), the matrix-core
logistic regression (kind 5: MALA D = 64, HMC D = 128 on 1,000 rows, MH D = 33 on 70 rows, the slice sampler D = 20), the slice sampler on a pair closure (kind 3,
USERPAIR: D = 100 and the odd D = 37; literal mode evaluates the whole target for every probe, the kernel compares the pair's own term), the pair-transposed kernels at
64 and 32 lanes per chain (MALA D = 1024; HMC D = 300 with the per-chain accept-rate tuner) and MALA on the streamed dense layout (kind 1, D = 256).  Each job asserts
the layout the device reports, and each MH / MALA / HMC job that the acceptance of its first block lies in ACCEPT_WINDOW, so that both branches of the accept
decision are compared.  Pooled tuners stay out: they couple all chains, so a block cannot be replayed alone.  Tolerances are the same 1e-12 / 1e-9 except for dual
averaging (DUALAVG_RTOL, measured oracle against oracle).  tests/test_literal_jobs_cpu.py runs every new job cut short on the CPU.

How small an error the new jobs catch (a record, no threshold).  On a scratch copy of the oracle the target's gradient was scaled by 1 + 2^-k in the SHIPPED
branch only — an arithmetic error that a kernel and its oracle branch would share — and the CPU stand-in check (`python tests/test_gpu_literal.py`) repeated; the
largest k at which the job turns red (k = 52 is one ulp):

    split_hmc_dense_d512 45   split_mala_dense_d1024 41   split_hmc_dense_d300_dualavg 40   logitm_mala_d64_n200 41
    logitm_hmc_d128_n1000 45  diag_mala_d1024 41          diag_hmc_d300_rate 45             stream_mala_dense_d256 41

i.e. a relative error of 5e-13 (MALA, dual averaging: 1e-12) or 3e-14 (HMC, L = 10 / 6 gradient evaluations per transition) in the gradient is caught, by the state
tolerance where no decision flips first.

`python tests/test_gpu_literal.py` replays the same blocks WITHOUT a GPU (shipped oracle in place of the device, which the -m gpu parity
tests show bit-identical to it): the pre-flight used before GPU time is spent.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent)); sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
import numpy_mirror as M  # noqa: E402
import oracle_ffi as O  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

SEED = 20260927
BLOCK, MIRROR_CHAINS = 16, 8
OLD_JOB_NAMES = ("cfg2_mala_h0.9", "cfg2_mala_h0.02", "cfg3_hmc_dense", "hmc_iso_d100", "cfg4_mala_swiss", "cfg5_hmc_rats_untuned", "slice_mvnormal_d100",
                 "slice_dense_d100", "slice_dense_d160_stream")
# the kernel families written after those (see the module docstring): workgroup-split dense (layout kind 6), matrix-core logistic (kind 5), the slice sampler on
# pair closures and the 32 / 64-lane forms of the pair-transposed kernels (kind 3), streamed dense MALA (kind 1), and the first MH and tuned jobs of this file
NEW_JOB_NAMES = ("split_hmc_dense_d512", "split_mala_dense_d1024", "split_mh_dense_d700_mean", "split_slice_dense_d260", "split_hmc_dense_d300_dualavg",
                 "logitm_mala_d64_n200", "logitm_hmc_d128_n1000", "logitm_mh_d33_n70", "logitm_slice_d20_n50", "pair_quartic_slice_d100", "pair_quartic_slice_d37",
                 "diag_mala_d1024", "diag_hmc_d300_rate", "stream_mala_dense_d256")
JOB_NAMES = OLD_JOB_NAMES + NEW_JOB_NAMES
# steps of the new jobs, chosen on the CPU so that the first block's acceptance lies inside ACCEPT_WINDOW (the acceptance is in each job's report)
HMC512_EPS, DA300_EPS, MALA64_H, HMC128_EPS, MALA1024_H, RATE300_EPS = 0.32, 0.1, 0.03, 0.1, 0.15, 0.45
# The dual-averaging job's own tolerances.  Measured on the CPU, oracle against oracle and oracle against mirror (no kernel involved), on the job's three blocks
# at its final chain count and seed, decisions identical throughout: literal against shipped 3.41e-12 (per block 3.4e-12, 7.1e-14, 3.8e-13; states,
# log-targets and gradients), mirror against shipped 5.67e-13.  Tolerance = 8 x that, rounded up to a power of ten (caps: 1e-9, 1e-7): 2.7e-11 -> 1e-10 and
# 4.5e-12 -> 1e-11.  The job is 16 transitions with 8 of adaptation: at 20 / 10 the same measurement gives 2.8e-11 and 6.0e-12, at 24 / 12 3.7e-11 and 5.3e-12,
# which would put the literal tolerance on its cap of 1e-9; the shorter job keeps it ten times tighter and still runs 8 transitions at the adapted step.
DUALAVG_RTOL, DUALAVG_MIRROR_RTOL = 1e-10, 1e-11
ACCEPT_WINDOW = (0.2, 0.9)      # of every new MH / MALA / HMC job, first block: a job that accepts (or rejects) everything compares one branch only


def _jobs():
    """name -> dict(kw = sampler / target keywords shared by Engine and OracleJob, n, nsteps, x0 (None: x0 ~ N(0, I) from the stream),
    mirror = (sampler name, target closures, Chain keywords, transitions replayed by the mirror))"""
    d = 100
    neg = K.GaussDiagTarget.negdot(d)
    dense = K.GaussDenseTarget.compound_symmetric(d, 0.5)
    dense160 = K.GaussDenseTarget.compound_symmetric(160, 0.3)
    X, y = cases.swiss_data()
    rats = cases.rats_target()
    n4, n5 = 32768 - 3, 131072 - 3
    x4 = np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(4).standard_normal((n4, 4))
    x5 = rats.least_squares_start()[None, :] + 0.05 * np.random.default_rng(11).standard_normal((n5, rats.ndims))
    mv = K.GaussDiagTarget.mvnormal(np.linspace(-2.0, 3.0, d), np.linspace(0.5, 2.0, d))
    wid = np.linspace(0.6, 3.0, d)
    return {
        # BASELINE cfg 2 as stated (the bench job): MALA driftstep 0.9, lt = -|x|^2, D = 100, 65,536-chain shape with a ragged tail
        "cfg2_mala_h0.9": dict(kw=dict(sampler=L.SAMPLER_MALA, target=neg, driftstep=0.9), n=65536 - 5, nsteps=1000, x0=None,
                               mirror=("mala", M.diag_target(np.ones(d), np.zeros(d), 0.0), dict(driftstep=0.9), 1000)),
        # ... and at a drift step that moves (99 % acceptance): thousands of accepted proposals per chain feed the next comparison
        "cfg2_mala_h0.02": dict(kw=dict(sampler=L.SAMPLER_MALA, target=neg, driftstep=0.02), n=65536 - 5, nsteps=1000, x0=None,
                                mirror=("mala", M.diag_target(np.ones(d), np.zeros(d), 0.0), dict(driftstep=0.02), 1000)),
        # BASELINE cfg 3: HMC eps = 0.1, L = 10 on the dense compound-symmetric Gaussian (FP64 MFMA kernels)
        "cfg3_hmc_dense": dict(kw=dict(sampler=L.SAMPLER_HMC, target=dense, leapstep=0.1, nleaps=10), n=65536 - 5, nsteps=1000, x0=None,
                               mirror=("hmc", M.dense_target(dense.precision, np.zeros(d), dense.const), dict(leapstep=0.1, nleaps=10), 500)),
        # north_star's "100-dim Gaussian HMC" on the README target (pair-transposed kernels)
        "hmc_iso_d100": dict(kw=dict(sampler=L.SAMPLER_HMC, target=neg, leapstep=0.1, nleaps=10), n=65536 - 5, nsteps=1000, x0=None,
                             mirror=("hmc", M.diag_target(np.ones(d), np.zeros(d), 0.0), dict(leapstep=0.1, nleaps=10), 1000)),
        # BASELINE cfg 4, one GPU's share: MALA 0.1 on the swiss logistic regression
        "cfg4_mala_swiss": dict(kw=dict(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), driftstep=0.1), n=n4, nsteps=2000, x0=x4,
                                mirror=("mala", M.logistic_target(X, y, 100.0), dict(driftstep=0.1), 2000)),
        # BASELINE cfg 5, one GPU's share, WITHOUT the pooled tuner (which couples all chains through one rate: a replay of a block needs the
        # device's step schedule, tests/test_gpu_workloads.py does that against the shipped oracle): HMC L = 32 on the rats model
        "cfg5_hmc_rats_untuned": dict(kw=dict(sampler=L.SAMPLER_HMC, target=rats, leapstep=0.02, nleaps=32), n=n5, nsteps=1000, x0=x5, gtol=1e-10,
                                      mirror=("hmc", M.hier_normal_target(rats.Y, rats.xc, rats.prior_prec, rats.gamma_a, rats.gamma_b),
                                              dict(leapstep=0.02, nleaps=32), 300)),
        # the slice sampler at D = 100 on a non-unit diagonal Gaussian with step-out: the kernels compare in difference form, lane by lane; the
        # literal oracle evaluates the whole log-target for every probe (SliceSampler.jl:66-95)
        "slice_mvnormal_d100": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=mv, slice_widths=wid, slice_stepout=True), n=65536 - 5, nsteps=200, x0=None,
                                    mirror=("slice", M.diag_target(mv.w, mv.mu, mv.const), dict(widths=wid, stepout=True), 40)),
        # the slice sampler on cfg 3's dense precision (round 5: the chains of a tile take their probes out of lockstep, each probe a matrix pass), and
        # beyond D = 128 on the streamed layouts (was the closure form): a full-size launch against the serial literal procedure
        "slice_dense_d100": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=dense, slice_widths=np.linspace(0.8, 2.4, d), slice_stepout=True), n=65536 - 5, nsteps=3, x0=None,
                                 mirror=("slice", M.dense_target(dense.precision, np.zeros(d), dense.const), dict(widths=np.linspace(0.8, 2.4, d), stepout=True), 3)),
        "slice_dense_d160_stream": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=dense160, slice_widths=np.linspace(0.8, 2.4, 160), slice_stepout=True), n=16384 - 5, nsteps=2,
                                        x0=None, mirror=("slice", M.dense_target(dense160.precision, np.zeros(160), dense160.const),
                                                         dict(widths=np.linspace(0.8, 2.4, 160), stepout=True), 2)),
        **_new_jobs(),
    }


def _split_dense(d, mean=False):
    """the BLAS-free precision of cases.SPLIT_CASES (diagonal plus three rank-one terms) -> (target, mirror closures)"""
    rng = np.random.default_rng(2000 + d)
    pm = cases.rank_one_precision(d, rng)
    mu = rng.standard_normal(d) if mean else None
    t = K.GaussDenseTarget(pm, const=0.75, mu=mu)
    return t, M.dense_target(pm, np.zeros(d) if mu is None else mu, 0.75)


def _around(mu, n, seed):
    """x0 = mu + N(0, I), made when the job runs (n x D doubles)"""
    return lambda: mu[None, :] + np.random.default_rng(seed).standard_normal((n, mu.size))


def _logit(nd, d, n, seed):
    """cases.synthetic_logit(nd, d) under a N(0, 10 I) prior, started from 0.1 N(0, I) (a start from N(0, I) at D = 64 saturates every row)
    -> (target, mirror closures, x0)"""
    X, y = cases.synthetic_logit(nd, d)
    return K.LogisticTarget(X, y, 10.0), M.logistic_target(X, y, 10.0), (lambda: 0.1 * np.random.default_rng(seed).standard_normal((n, d)))


def _new_jobs():
    """The jobs of NEW_JOB_NAMES.  Beyond the keys of _jobs(): layout = the (kind, lanes per chain, elements per lane) the device must report (a job that silently
    runs on another kernel tests nothing new), accept = the window the first block's acceptance must lie in, rtol / mirror_rtol = the tolerance of the states against
    literal mode / the mirror where it is not 1e-12 / 1e-9 (dual averaging only; origin beside the key)."""
    nbig, nwide = 65536 - 5, 16384 - 5          # D >= 512: X and G are N x D doubles each
    win = ACCEPT_WINDOW
    d512, m512 = _split_dense(512)
    d1024, m1024 = _split_dense(1024, mean=True)
    d700, m700 = _split_dense(700, mean=True)
    d260, m260 = _split_dense(260)
    d300, m300 = _split_dense(300)
    d256, m256 = _split_dense(256)
    l64, ml64, x64 = _logit(200, 64, nbig, 64)
    l128, ml128, x128 = _logit(1000, 128, nbig, 128)
    l33, ml33, x33 = _logit(70, 33, nbig, 33)
    l20, ml20, x20 = _logit(50, 20, nbig, 20)
    q100 = K.CustomTarget.pairwise(100, cases.SRC_PAIR_QUARTIC, [0.1, 0.4])
    q37 = K.CustomTarget.pairwise(37, cases.SRC_PAIR_QUARTIC, [0.1, 0.4])
    mv1024 = K.GaussDiagTarget.mvnormal(np.linspace(-2.0, 3.0, 1024), np.linspace(0.5, 2.0, 1024))
    mv300 = K.GaussDiagTarget.mvnormal(np.linspace(-1.0, 1.0, 300), np.linspace(0.5, 1.5, 300))
    sig700 = np.linspace(0.02, 0.08, 700)
    w260, w100, w37 = np.linspace(0.5, 2.0, 260), np.linspace(0.8, 2.4, 100), np.linspace(0.8, 2.4, 37)
    rate = dict(targetrate=0.65, period=5, burnin=30)
    da = dict(targetrate=0.65, da_nadapt=8)
    return {
        # ---- dense targets of 257 .. 1024 dimensions: a tile of 16 chains on a workgroup of wavefronts (klara_dense_split.h, layout kind 6)
        "split_hmc_dense_d512": dict(kw=dict(sampler=L.SAMPLER_HMC, target=d512, leapstep=HMC512_EPS, nleaps=10), n=nwide, nsteps=200, x0=None,
                                     layout=O.split_dense_layout(512), accept=win, mirror=("hmc", m512, dict(leapstep=HMC512_EPS, nleaps=10), 200)),
        # (the precision matrix, 8 MB, is larger than the L2 cache)
        "split_mala_dense_d1024": dict(kw=dict(sampler=L.SAMPLER_MALA, target=d1024, driftstep=0.15), n=nwide, nsteps=100, x0=_around(d1024.mu, nwide, 1024),
                                       layout=O.split_dense_layout(1024), accept=win, mirror=("mala", m1024, dict(driftstep=0.15), 100)),
        # the first MH job of this file: per-coordinate proposal scales, a target with a mean
        "split_mh_dense_d700_mean": dict(kw=dict(sampler=L.SAMPLER_MH, target=d700, mh_sigma=sig700), n=nwide, nsteps=100, x0=_around(d700.mu, nwide, 700),
                                         layout=O.split_dense_layout(700), accept=win, mirror=("mh", m700, dict(sigma=sig700), 100)),
        # the slice sampler with step-out: the chains of a tile take their probes out of lockstep, every probe a pass over P
        "split_slice_dense_d260": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=d260, slice_widths=w260, slice_stepout=True), n=nbig, nsteps=2, x0=None,
                                       layout=O.split_dense_layout(260), mirror=("slice", m260, dict(widths=w260, stepout=True), 2)),
        # HMC with dual averaging: a per-chain step AND trip count (a wavefront runs to the longest trajectory of its chains).  The step is
        # exp(mu - sqrt(t) hbar / gamma) of the continuous acceptance probability min(1, exp(dH)), so an ulp of dH is amplified in the first adaptation steps and
        # fed back: the shipped and the literal oracle themselves part by more than 1e-12 (see DUALAVG_RTOL below, measured oracle against oracle)
        "split_hmc_dense_d300_dualavg": dict(kw=dict(sampler=L.SAMPLER_HMC, target=d300, leapstep=DA300_EPS, nleaps=5, tuner=L.TUNER_DUAL_AVERAGING, **da), n=nbig, nsteps=16,
                                             x0=None, layout=O.split_dense_layout(300), accept=win, rtol=DUALAVG_RTOL, gtol=DUALAVG_RTOL, mirror_rtol=DUALAVG_MIRROR_RTOL,
                                             mirror=("hmc", m300, dict(leapstep=DA300_EPS, nleaps=5, tuner="da", targetrate=0.65, nadapt=8), 16)),
        # ---- logistic regression of 17 .. 256 parameters on the matrix cores (klara_logit_mfma.h, layout kind 5); literal mode takes both exponentials of every row
        "logitm_mala_d64_n200": dict(kw=dict(sampler=L.SAMPLER_MALA, target=l64, driftstep=MALA64_H), n=nbig, nsteps=500, x0=x64, layout=(5, 4, 16), accept=win,
                                     mirror=("mala", ml64, dict(driftstep=MALA64_H), 500)),
        "logitm_hmc_d128_n1000": dict(kw=dict(sampler=L.SAMPLER_HMC, target=l128, leapstep=HMC128_EPS, nleaps=10), n=nbig, nsteps=60, x0=x128, layout=(5, 4, 32), accept=win,
                                      mirror=("hmc", ml128, dict(leapstep=HMC128_EPS, nleaps=10), 60)),
        # odd D, 70 rows: the last row tile holds 6 rows
        "logitm_mh_d33_n70": dict(kw=dict(sampler=L.SAMPLER_MH, target=l33, mh_sigma=np.full(33, 0.05)), n=nbig, nsteps=200, x0=x33, layout=(5, 4, 16), accept=win,
                                  mirror=("mh", ml33, dict(sigma=np.full(33, 0.05)), 200)),
        "logitm_slice_d20_n50": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=l20, slice_widths=np.full(20, 1.5), slice_stepout=True), n=nbig, nsteps=10, x0=x20,
                                     layout=(5, 4, 8), mirror=("slice", ml20, dict(widths=np.full(20, 1.5), stepout=True), 10)),
        # ---- the slice sampler on a pair closure (k_diagt<SLICE, .., USERPAIR>): the kernel compares the pair's own term, literal mode evaluates the whole
        # target for every probe; coupled within the pair, and at an odd D the half pair
        "pair_quartic_slice_d100": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=q100, slice_widths=w100, slice_stepout=True), n=nbig, nsteps=40, x0=None,
                                        layout=(3, 8, 14), mirror=("slice", M.pair_quartic_target(0.1, 0.4, 100), dict(widths=w100, stepout=True), 40)),
        "pair_quartic_slice_d37": dict(kw=dict(sampler=L.SAMPLER_SLICE, target=q37, slice_widths=w37, slice_stepout=True), n=nbig, nsteps=20, x0=None,
                                       layout=(3, 8, 6), mirror=("slice", M.pair_quartic_target(0.1, 0.4, 37), dict(widths=w37, stepout=True), 20)),
        # ---- the pair-transposed kernels at 64 and 32 lanes per chain (one chain per wavefront; two), the second with the per-chain accept-rate tuner
        # (its step depends on decisions only, so the untuned tolerances hold)
        "diag_mala_d1024": dict(kw=dict(sampler=L.SAMPLER_MALA, target=mv1024, driftstep=MALA1024_H), n=nwide, nsteps=200, x0=None, layout=(3, 64, 16), accept=win,
                                mirror=("mala", M.diag_target(mv1024.w, mv1024.mu, mv1024.const), dict(driftstep=MALA1024_H), 200)),
        "diag_hmc_d300_rate": dict(kw=dict(sampler=L.SAMPLER_HMC, target=mv300, leapstep=RATE300_EPS, nleaps=6, tuner=L.TUNER_ACCEPT_RATE, **rate), n=nbig, nsteps=60, x0=None,
                                   layout=(3, 32, 10), accept=win, mirror=("hmc", M.diag_target(mv300.w, mv300.mu, mv300.const),
                                                                           dict(leapstep=RATE300_EPS, nleaps=6, tuner="rate", **rate), 60)),
        # ---- MALA on the streamed dense layout (k_dense_big, P read from memory at every pass; only its slice kernel was under these checkers)
        "stream_mala_dense_d256": dict(kw=dict(sampler=L.SAMPLER_MALA, target=d256, driftstep=0.25), n=nbig, nsteps=100, x0=None, layout=(1, 4, 64), accept=win,
                                       mirror=("mala", m256, dict(driftstep=0.25), 100)),
    }


def _offsets(n, nparts=2):
    blocks = (n + 15) // 16                               # chain partitions are cut in blocks of 16 chains (klara_run.hip part_range)
    boundary = ((blocks + 1) // 2) * 16
    return (0, boundary - 8, n - BLOCK)


def _close(a, b, rel):
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.abs(b) + np.abs(b).mean()
    return bool(np.all(np.abs(a - b) <= rel * scale))


def _dev(a, b):
    """the deviation _close bounds: max |a - b| / (|b| + mean |b|)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / (np.abs(b) + np.abs(b).mean())))


def _device_run(job):
    """the full-size job through the C ABI -> (accept mask (nsteps x n), x, lt, g)"""
    eng = K.Engine(nchains=job["n"], nsteps=job["nsteps"], seed=SEED, monitor=L.MON_ACCEPT | L.MON_SUMMARIES, **job["kw"])
    if job["x0"] is None:
        eng.init_state_normal()
    else:
        eng.set_state(job["x0"])
    eng.run(job["nsteps"])
    mask = eng.accept_mask()
    x, lt, g = eng.state()
    lay = tuple(eng.layout())
    eng.close()
    return mask, x, lt, g, lay


def _oracle_block(job, off, nchains, nsteps, literal, layout=None):
    lib = O.load()
    case = dict(job["kw"], nchains=nchains, nsteps=job["nsteps"], name="literal", x0=None, seed=SEED)
    oj = O.OracleJob(**cases.oracle_kwargs(case, layout=layout, chain_offset=off))
    lib.ko_set_literal(1 if literal else 0)
    try:
        if job["x0"] is None:
            assert oj.init_state_normal() == 0
        else:
            assert oj.set_state(job["x0"][off:off + nchains]) == 0
        assert oj.run(nsteps) == 0
    finally:
        lib.ko_set_literal(0)
    return oj


def _stand_in_run(job):
    """no GPU: the shipped oracle on the blocks the checks look at (everything else stays zero) — the pre-flight of __main__"""
    n, ns = job["n"], job["nsteps"]
    mask = np.zeros((ns, n), np.uint8); x = np.zeros((n, job["kw"]["target"].ndims)); lt = np.zeros(n); g = np.zeros_like(x)
    for off in _offsets(n):
        oj = _oracle_block(job, off, BLOCK, ns, literal=False)
        sl = slice(off, off + BLOCK)
        mask[:, sl], x[sl], lt[sl], g[sl] = oj.accept, oj.X, oj.LT, oj.G
    return mask, x, lt, g, (oj.layout.kind, oj.layout.G, oj.layout.E)      # (the layout oracle_ffi.default_layout expects the device to choose)


def check_job(name, run, max_steps=None):
    """`max_steps`: the job cut to that many transitions (the CPU test that keeps the jobs runnable; the full length is what -m gpu and __main__ run)"""
    job = dict(_jobs()[name])
    if callable(job["x0"]):
        job["x0"] = job["x0"]()
    if max_steps is not None and max_steps < job["nsteps"]:
        smp, tgt, ckw, nm = job["mirror"]
        job["nsteps"], job["mirror"] = max_steps, (smp, tgt, ckw, min(nm, max_steps))
    mask, x, lt, g, lay = run(job)
    n, ns = job["n"], job["nsteps"]
    assert mask.shape == (ns, n)
    if "layout" in job:
        assert tuple(lay) == tuple(job["layout"]), (name, "the job did not run on the kernel family it is here for", lay, job["layout"])
    needg = job["kw"]["sampler"] in (L.SAMPLER_MALA, L.SAMPLER_HMC)
    rtol, mirror_rtol = job.get("rtol", 1e-12), job.get("mirror_rtol", 1e-9)
    report = {"job": name, "chains": n, "transitions": ns, "layout": lay}
    worst = 0.0
    # (1) literal Julia arithmetic, three blocks of 16 chains, all transitions
    ndec = 0
    for off in _offsets(n):
        oj = _oracle_block(job, off, BLOCK, ns, literal=True, layout=lay)
        sl = slice(off, off + BLOCK)
        assert np.array_equal(mask[:, sl], oj.accept), (name, off, "an accept decision differs from the literal Julia arithmetic",
                                                        int((mask[:, sl] != oj.accept).sum()))
        worst = max(worst, _dev(x[sl], oj.X), _dev(lt[sl], oj.LT))
        assert _close(x[sl], oj.X, rtol) and _close(lt[sl], oj.LT, rtol), (name, off, float(np.max(np.abs(x[sl] - oj.X))), worst)
        if needg:
            # (the rats gradient at a posterior point is a cancelling sum of ~150 residual terms, each hundreds of times larger than the result:
            # the state agrees to 2e-16, the gradient formed from it to 1e-12 of ITS size, which is 1e-14 of the terms')
            assert _close(g[sl], oj.G, job.get("gtol", 1e-12)), (name, off)
        ndec += oj.accept.size
    report["decisions_vs_literal"] = ndec
    report["dev_vs_literal"] = worst                      # largest |a - b| / (|b| + mean |b|) of states and log-targets over the three blocks
    report["acceptance"] = float(mask[:, :BLOCK].mean())
    if "accept" in job:
        assert job["accept"][0] <= report["acceptance"] <= job["accept"][1], (name, "acceptance of the first block outside the window", report["acceptance"])
    # (2) the independent NumPy mirror, one block of 8 chains at the partition boundary, the first `nm` transitions
    smp, (ltf, gradf), ckw, nm = job["mirror"]
    off = _offsets(n)[1]
    if job["x0"] is None:
        x0 = np.stack([M.init_state_normal(SEED, off + k, x.shape[1]) for k in range(MIRROR_CHAINS)])
    else:
        x0 = job["x0"][off:off + MIRROR_CHAINS]
    chains = [M.Chain(smp, ltf, gradf, x0[k], SEED, off + k, nsteps=ns, **ckw) for k in range(MIRROR_CHAINS)]
    for k, c in enumerate(chains):
        c.run(nm)
        assert np.array_equal(mask[:nm, off + k].astype(bool), np.array(c.accepts)), (name, off + k, "an accept decision differs from the NumPy mirror")
    if nm == ns:
        report["dev_vs_mirror"] = max(_dev(x[off + k], c.x) for k, c in enumerate(chains))
        for k, c in enumerate(chains):
            assert _close(x[off + k], c.x, mirror_rtol), (name, k, report["dev_vs_mirror"])
    report["decisions_vs_mirror"] = MIRROR_CHAINS * nm
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("name", JOB_NAMES)
def test_hip_path_equals_literal_julia_arithmetic_and_numpy_mirror(name, gpu_required):
    r = check_job(name, _device_run)
    print(r)
    if name != "cfg2_mala_h0.9":
        assert r["acceptance"] > 0.1, r          # (the comparison is only worth something if the chains move; the new jobs: ACCEPT_WINDOW, in check_job)


if __name__ == "__main__":
    import json
    import time
    assert tuple(_jobs().keys()) == JOB_NAMES
    for nm in (sys.argv[1:] or JOB_NAMES):
        t0 = time.time()
        r = check_job(nm, _stand_in_run)
        r["seconds"] = round(time.time() - t0, 1)
        print(json.dumps(r))
