#!/usr/bin/env python3
"""MH(Σ) (KLARA_SAMPLER_MH_COV) on one GPU, measured against what the build already has.
(a) The mat-vec's price: the job with mh_factor = diag(σ) against the MH job with mh_sigma = σ — the same chain bit for bit (tests/test_gpu_mhcov.py) — on
    the cfg 4 swiss job and on quadratic closures at D = 8, 16, 32 (condition number 50): 262,144 chains, 32 transitions per launch, running sums on, the
    two samplers alternating, five rounds; transitions/s from the library's own event timing (klara_last_run_ms), the median of the five; the loaded
    kernels' registers and scratch.
(b) What the feature is for: pooled ESS (klara_gather_ess, streamed, the smallest over the dimensions) per second of device time on the swiss job and on a
    D = 16 Gaussian with every correlation 0.9.  A pilot MH job with covariance=True's monitor gives the pooled covariance Σ̂; then MH(rwm_factor(Σ̂)),
    MH(σ) with σ the pilot's marginal standard deviations times 2.38 / sqrt(D), and AMWG — started at 2.38 times the conditional standard deviations Σ̂
    gives and left to adapt for 500 transitions — each run 200 transitions of burn-in and 800 kept at thinning 4 with acov_maxlag = 63 (a window of 252
    transitions).  Device time is klara_last_run_ms of the kept part: the transition kernels and the autocovariance updates behind them, the same for all.
Writes the measured block of profiles/mhcov.txt (or of the file given as second argument) and keeps that file's commentary from "Reading:" on.
usage: run_mhcov.py [nchains] [output file]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import amwg_cases as WC  # noqa: E402
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
import mhcov_cases as MC  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def price(label, target, x0, sigma, nsteps):
    d = target.ndims
    samplers = (("MH(σ)", dict(sampler=L.SAMPLER_MH, mh_sigma=sigma)), ("MH(diag σ)", MC.mhcov(np.diag(sigma))))
    eng, r = {}, {name: [] for name, _ in samplers}
    for name, kw in samplers:
        e = K.Engine(target=target, nchains=n, nsteps=10 ** 6, steps_per_launch=32, monitor=L.MON_SUMMARIES, **kw)
        e.set_state(x0)
        e.run(64)                                                        # warm-up (clocks, code objects)
        eng[name] = e
    for _ in range(5):                                                   # the two alternate: what else runs on the box meets both
        for name, _ in samplers:
            eng[name].run(nsteps)
            ms, nl = eng[name].last_run_ms()
            r[name].append(n * nsteps / (ms * 1e-3))
    rates, states = {}, {}
    for name, _ in samplers:
        e = eng[name]
        acc, tot = e.accept_counts()
        v, sc, lds = e.kernel_attributes(0, 32)
        rates[name] = float(np.median(r[name]))
        states[name] = e.state()[0]
        say(f"{label:18s} {name:10s} layout {e.layout()}: {rates[name]:.4g} transitions/s (median of 5 runs of {nsteps} transitions, {nl} launches each; "
            f"min {min(r[name]):.4g}, max {max(r[name]):.4g}), acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B")
        e.close()
    same = bool(np.array_equal(states["MH(σ)"], states["MH(diag σ)"]))
    say(f"{label:18s} MH(diag σ) / MH(σ) in transitions/s = {rates['MH(diag σ)'] / rates['MH(σ)']:.3f}   (D (D + 1) = {d * (d + 1)} FP64 instructions a transition; "
        f"final states bit-identical: {same})")


def ess_rate(label, name, target, x0, kw, adapt=0):
    burn, keep, thin = 200, 800, 4
    e = K.Engine(target=target, nchains=n, nsteps=adapt + burn + keep, burnin=adapt + burn, thinning=thin, steps_per_launch=32, monitor=L.MON_SUMMARIES,
                 acov_maxlag=63, seed=11, **kw)
    e.set_state(x0)
    e.run(adapt + burn)
    e.run(keep)
    ms, _ = e.last_run_ms()
    out = e.pooled_ess("streamed")
    acc, tot = e.accept_counts()
    ess = float(out["ess"].min())
    say(f"{label:18s} {name:28s} pooled ESS (min over D) {ess:.4g} of {n * (keep // thin)} kept draws, tau {out['tau'].max():.2f} kept draws, window exhausted in "
        f"{int(out['window_exhausted'].sum())} of {target.ndims}; {ms:.1f} ms for {keep} transitions: {ess / (ms * 1e-3):.4g} ESS/s; acceptance {acc.sum() / (n * tot):.3f}")
    e.close()
    return ess / (ms * 1e-3)


def purpose(label, target, x0, pilot_sigma):
    d = target.ndims
    pilot = K.Engine(target=target, nchains=n, nsteps=1000, burnin=500, sampler=L.SAMPLER_MH, mh_sigma=np.full(d, pilot_sigma), steps_per_launch=32,
                     monitor=L.MON_SUMMARIES | L.MON_COVARIANCE, seed=7)
    pilot.set_state(x0); pilot.run(1000)
    _, m2, ns, _ = pilot.pooled_covariance()
    cov = m2 / (ns - 1)
    x1 = pilot.state()[0]                                                # every contender starts where the pilot ended
    pilot.close()
    sd = np.sqrt(np.diag(cov))
    cond_var = 1.0 / np.diag(np.linalg.inv(cov))
    say(f"{label:18s} pilot MH(σ = {pilot_sigma}): marginal sd {sd.min():.3g} .. {sd.max():.3g}, largest |correlation| "
        f"{np.abs(cov / np.outer(sd, sd) - np.eye(d)).max():.3f}, condition number of Σ̂ {np.linalg.cond(cov):.3g}")
    r = {}
    r["cov"] = ess_rate(label, "MH(rwm_factor(Σ̂))", target, x1, MC.mhcov(K.rwm_factor(cov)))
    r["diag"] = ess_rate(label, "MH(2.38/sqrt(D) sd)", target, x1, dict(sampler=L.SAMPLER_MH, mh_sigma=2.38 / np.sqrt(d) * sd))
    r["amwg"] = ess_rate(label, "AMWG, 500 transitions adapted", target, x1,
                         dict(amwg_logsigma0=np.log(2.38 ** 2 * cond_var), **WC.amwg(targetrate=0.44, period=50)), adapt=500)
    say(f"{label:18s} ESS/s of MH(Σ) over MH(σ): {r['cov'] / r['diag']:.2f}; over AMWG: {r['cov'] / r['amwg']:.2f}")


rng = np.random.default_rng(0)
X, y = cases.swiss_data()
swiss = K.LogisticTarget(X, y, 100.0)
swiss_x0 = MC.SWISS_X0[None, :] + 0.1 * rng.standard_normal((n, 4))
say("(a) the mat-vec's price")
price("swiss D=4 (cfg 4)", swiss, swiss_x0, np.full(4, 0.1), 320)
for d in (8, 16, 32):
    P = WC.conditioned_precision(d, 50.0, seed=d)
    price(f"closure D={d}", WC.quad_target(0.5, P), 0.5 * np.random.default_rng(2).standard_normal((n, d)), np.full(d, 0.1), max(64, 320 // (d // 8)))
say("")
say("(b) pooled ESS per second of device time")
purpose("swiss D=4", swiss, swiss_x0, 0.1)
t16, S16 = MC.correlated_gaussian(16, 0.9)
purpose("gauss rho=0.9 D=16", t16, np.random.default_rng(3).standard_normal((n, 16)) @ np.linalg.cholesky(S16).T, 0.1)

HEADER = """MH(Σ) (KLARA_SAMPLER_MH_COV) against the MH and AMWG kernels of the same build — scripts/run_mhcov.py on one MI355X, one session, the samplers alternating on the same box
=====================================================================================================================================================================
%s chains, 32 transitions per launch, running sums on.  Transitions/s and device time from klara_last_run_ms; (a) median of five runs after a 64-transition warm-up.
The yardsticks are the unchanged MH and AMWG kernels of this commit.

"""
MARK = "\nReading:"          # everything from here on in the committed file is commentary: kept as it is
out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "mhcov.txt"
committed = (ROOT / "profiles" / "mhcov.txt").read_text() if (ROOT / "profiles" / "mhcov.txt").exists() else ""
tail = committed[committed.index(MARK):] if MARK in committed else "\n"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(HEADER % (f"{n:,}") + "\n".join(lines) + "\n" + tail)
