"""Random jobs for the samplers that carry a per-chain matrix in registers — SMMALA, SMMALA with the softabs transform, RAM — shared by
tests/test_matrix_samplers_host.py and tests/test_gpu_matrix_samplers.py.

`random_case(seed, family)` returns a case in the shape smmala_cases.make / softabs_cases.make / ram_cases.make return (Engine keyword
arguments plus "x0" and "name"; softabs: plus "mirror"), so `engine_kwargs`, `ref_job` and `mirror_chains` of those modules take it as it is.
How the job is run — monitor word, transitions per launch, the pieces the run is split into, the shard's chain offset — is no Engine
keyword of the case: it hangs on the dict as the attribute `run`.  `instantiation(case)` restates klara_plan.h: the (sampler, E, MODE) of the
k_transitions instantiation the job launches.
"""
import numpy as np

import autodiff_cases as AC
import cases
import klara_jl_amd as K
import ram_cases as RC
import smmala_cases as SC
import softabs_cases as SAC
from klara_jl_amd import _lib as L

FAMILIES = ("smmala", "softabs", "ram")
MODULES = {"smmala": SC, "softabs": SAC, "ram": RC}

# rng = default_rng(BASE[family] + seed).  The three ranges do not overlap; each base is the first multiple of 100 from the family's starting
# point (smmala 0, ram 700, softabs 1400) at which seeds 0 .. NSEEDS - 1 fill the whole ledger of tests/test_matrix_samplers_host.py (every (E, MODE)
# pair, every D with both target kinds, every tuner, both row-split states: the seeds do not reach all of that at every base — smmala 0 .. 200 and ram
# 700 .. 1200 leave entries empty, and softabs' 24 seeds have 15 (D, source) pairs to fill: 8000 is the first base where they do) and the C reference and the
# NumPy restatement agree on the first 4 chains of every seed (test_reference_matches_restatement excludes no seed; a family that cannot meet it at a base moves
# on to the next instead.  None of these three bases had to: the one thing met while the generator was written was a softabs job — doublewell, D = 4, start scale
# 1.0, 36 transitions — whose accept masks agreed and whose states ended 1.7e-9 apart where the comparison allows 1e-10: the two sides' rounding difference of one
# chain, 8e-16 after the first transition, grew 3 to 5 fold with each of its 14 accepted moves.  That is the double well's own sensitivity to its start, not a
# near-tie and not an error of either side.)
# softabs has 24 seeds where the others have 48: every (source, D, MODE) of its jobs is a run-time compilation of up to 3 s (the Jacobi sweeps at D = 8), and with
# 48 the GPU file took 3 x the three per-sampler files together (profiles/matrix_sampler_sweep.txt).  No dimension, row count or chain count was cut.
BASE = {"smmala": 300, "softabs": 8000, "ram": 1300}
NSEEDS = {"smmala": 48, "softabs": 24, "ram": 48}

ROWS = (1, 5, 39, 63, 64, 65, 66, 71, 131, 300)        # 63 / 64 / 65: the row split (RS = 4) starts at 64; 66, 71, 131: no multiple of RS x the two-row batch
CHAINS = (1, 2, 31, 63, 64, 65, 100, 256, 257)         # one wavefront and one more, one workgroup and one more
HIST_SMMALA = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT | L.MON_HIST_GRAD
HIST_RAM = L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT

# every user-defined source is one of five fixed texts — SC.SRC_QUAD_TENSOR ("quad"), RC.SRC_HALFSPACE ("halfspace"), cases.SRC_NN_LL + SRC_NN_LP ("likprior"),
# SAC.AD_DOUBLEWELL ("doublewell"), SAC.SRC_MIXED ("mixed") — with the dimension as the only compile-time parameter that varies: everything else a job draws
# for its target is data, so the run-time compilations are bounded by sources x dimensions x kernel MODE sets and the compilation cache makes repeats free


class Case(dict):
    """a case dict (what the *_cases modules read) with the run shape beside it"""
    run = None


def pad_of(d):
    """elements per lane of a D-vector, D <= 8 (klara_plan.h select_layout: the logistic target's E; custom_layout: pow2ceil(max(D, 2)))"""
    return 2 if d <= 2 else 4 if d <= 4 else 8


def _split(rng, nsteps):
    """the run in 1 - 3 pieces"""
    k = int(rng.integers(1, 4))
    cuts = sorted(int(c) for c in rng.integers(1, nsteps, size=k - 1)) if nsteps > 1 else []
    edges = [0] + cuts + [nsteps]
    return [b - a for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _logit(rng, seed, d):
    nrows = int(rng.choice(ROWS))
    X, y = cases.synthetic_logit(nrows, d, seed)
    return K.LogisticTarget(X, y, float(rng.choice([1.0, 25.0, 100.0])))


def random_case(seed, family):
    assert family in FAMILIES
    rng = np.random.default_rng(BASE[family] + seed)
    d = int(rng.integers(1, 9))
    n = int(rng.choice(CHAINS))
    # which kernel MODE the job is for (klara_plan.h:300-303), drawn first — left to independent draws of tuner, monitor and launch length, MODE 7 would be one
    # job in sixty: a tuned or counting job (0; two in five, it has four tuners to go through), a plain job with a monitor (1), a plain job without (3), and that
    # one in one-transition launches (7; one in five each)
    mode = int(rng.choice([0, 1, 3, 7], p=[0.4, 0.2, 0.2, 0.2]))
    hist = HIST_RAM if family == "ram" else HIST_SMMALA
    monitor = 0 if mode in (3, 7) else int(rng.choice([L.MON_ACCEPT, L.MON_ACCEPT | L.MON_SUMMARIES, hist] + ([0] if mode == 0 else [])))
    spl = 1 if mode == 7 else int(rng.choice([0, 7] + ([1] if mode in (0, 1) else [])))
    burnin = int(rng.choice([0, 3, 20])); thinning = int(rng.choice([1, 1, 2, 5]))
    nsteps = burnin + int(rng.integers(6, 41))
    c = Case(nchains=n, nsteps=nsteps, burnin=burnin, thinning=thinning, seed=int(rng.integers(1, 2 ** 40)))
    logistic = family != "softabs" and bool(rng.integers(0, 2))
    kind = "logit"
    if family == "smmala":
        c.update(sampler=L.SAMPLER_SMMALA, driftstep=float(rng.uniform(0.4, 1.2)))
        if logistic:
            c.update(target=_logit(rng, seed, d), x0=0.3 * rng.standard_normal((n, d)))
        else:
            kind = "quad"
            P = SC.conditioned_precision(d, float(rng.choice([1.0, 50.0, 1e4])), seed=int(rng.integers(1, 1 << 30)))
            c.update(target=SC.quad_target(0.5, P, P), x0=0.5 * rng.standard_normal((n, d)))
    elif family == "softabs":
        kind = "mixed" if d >= 2 and bool(rng.integers(0, 2)) else "doublewell"            # (SRC_MIXED divides by D - 1)
        a, scale = float(rng.choice([0.5, 1.0, 2.0, 1000.0])), float(rng.choice([0.25, 1.0]))
        c.update(sampler=L.SAMPLER_SMMALA, smmala_softabs=a, driftstep=float(rng.uniform(0.4, 1.0)))
        if kind == "doublewell":             # at start scale 1.0 minus the Hessian (diagonal 12 x^2 - 4 + k deg) is indefinite for a good share of the chains
            k = float(rng.uniform(0.2, 1.0))
            c.update(target=AC.target(SAC.AD_DOUBLEWELL, d, np.array([k]), order=2), x0=scale * rng.standard_normal((n, d)), mirror=SAC._doublewell(d, k))
        else:                                # neighbouring lanes: condition 1 to a spread of 1e6, some chains exactly at condition 1
            R, _ = np.linalg.qr(rng.standard_normal((d, d)))
            x0 = scale * rng.standard_normal((n, d))
            x0[:, 0] = rng.uniform(0.0, 3.3, n) * rng.choice([-1.0, 1.0], n)
            x0[::7, 0] = 0.0
            c.update(target=K.CustomTarget(d, SAC.SRC_MIXED, data=np.ascontiguousarray(R).ravel()), x0=x0,
                     mirror=((lambda x: -0.5 * float(x @ x)), (lambda x: -x), SAC._mixed_tensor(R)))
    else:
        c.update(sampler=L.SAMPLER_RAM, ram_targetrate=float(rng.uniform(0.15, 0.5)), ram_gamma=float(1.0 - rng.uniform(0.0, 0.5)))      # gamma in (0.5, 1]
        S0 = rng.uniform(0.2, 0.8, d)
        if bool(rng.integers(0, 2)):          # a full lower triangle with a positive diagonal
            S0 = np.diag(S0) + np.tril(0.15 * rng.standard_normal((d, d)), -1)
        c["ram_S0"] = S0
        if logistic:
            c.update(target=_logit(rng, seed, d), x0=0.3 * rng.standard_normal((n, d)))
        else:
            kind = str(rng.choice(["quad", "halfspace", "likprior"]))
            if kind == "quad":
                P = SC.conditioned_precision(d, float(rng.choice([1.0, 50.0, 1e4])), seed=int(rng.integers(1, 1 << 30)))
                c.update(target=RC.quad_target(0.5, P, P), x0=0.5 * rng.standard_normal((n, d)))
            elif kind == "halfspace":        # started inside the support; proposals leave it (log-target -inf)
                c.update(target=K.CustomTarget(d, RC.SRC_HALFSPACE), x0=np.abs(rng.standard_normal((n, d))) * 0.3 + 0.05)
            else:                            # likelihood + prior form, no gradient closures
                data = np.concatenate([rng.standard_normal(d) * 2, rng.uniform(0.5, 2.0, d), rng.uniform(-1.0, 1.0, d), rng.uniform(1.0, 5.0, d)])
                c.update(target=K.CustomTarget.likelihood_prior(d, cases.SRC_NN_LL, cases.SRC_NN_LP, data=data), x0=rng.standard_normal((n, d)))
    # the tuner: a plain job (MODE 1, 3, 7) has VanillaMCTuner without counting; MODE 0 takes one of the others
    if mode == 0:
        tun = "verbose" if family == "ram" else str(rng.choice(["verbose", "rate", "rate_erf", "pooled"]))
        if tun == "verbose":
            c.update(verbose=True, period=int(rng.integers(3, 12)))
        else:
            c.update(tuner=L.TUNER_ACCEPT_RATE, targetrate=float(rng.uniform(0.3, 0.8)), period=int(rng.integers(3, 12)))
            if tun == "rate_erf":
                c.update(tuner_score=1, score_k=3.0)
            if tun == "pooled":
                c.update(tuner_mode=L.TUNE_POOLED)
    c["name"] = f"random_{family}_{seed}_{kind}_d{d}"
    c.run = dict(monitor=monitor, steps_per_launch=spl, runs=_split(rng, nsteps), chain_offset=int(rng.choice([0, 1, 64, 1000])), kind=kind)
    return c


def tuner_kind(case):
    if case.get("tuner", L.TUNER_VANILLA) == L.TUNER_ACCEPT_RATE:
        return "pooled" if is_pooled(case) else "rate_erf" if has_erf_score(case) else "rate"
    return "verbose" if case.get("verbose", False) else "vanilla"


def has_erf_score(case):
    return case.get("tuner_score", 0) == 1


def is_pooled(case):
    return case.get("tuner_mode", L.TUNE_PER_CHAIN) == L.TUNE_POOLED


def nrows(case):
    """data rows of a logistic case, None otherwise"""
    t = case["target"]
    return int(t.X.shape[0]) if isinstance(t, K.LogisticTarget) else None


def instantiation(case, monitor=None, steps_per_launch=None):
    """(sampler, E, MODE) of the k_transitions instantiation klara_plan.h picks for the job (launch_transitions instantiates MODE 0, 1, 3, 7 per
    sampler and E).  cnt_predicate: RAM counts when verbose, SMMALA when verbose under VanillaMCTuner or under AcceptanceRateMCTuner; plain
    (klara_plan.h:300): nothing counts, the tuner state is per chain, no dual averaging.  A plain job without a monitor runs MODE 3, its
    one-transition launches MODE 7 (klara_run.hip launch_steps: `steps_per_launch = 1` makes every launch one), with a monitor MODE 1; any other job MODE 0."""
    monitor = case.run["monitor"] if monitor is None else monitor
    spl = case.run["steps_per_launch"] if steps_per_launch is None else steps_per_launch
    sampler, tuner, verbose = case["sampler"], case.get("tuner", L.TUNER_VANILLA), bool(case.get("verbose", False))
    cnt = verbose if sampler == L.SAMPLER_RAM else ((tuner == L.TUNER_VANILLA and verbose) or tuner == L.TUNER_ACCEPT_RATE or
                                                     (tuner == L.TUNER_DUAL_AVERAGING and verbose))
    plain = not cnt and not is_pooled(case) and tuner != L.TUNER_DUAL_AVERAGING
    mode = (7 if spl == 1 else 3) if plain and monitor == 0 else 1 if plain else 0
    return sampler, pad_of(case["target"].ndims), mode
