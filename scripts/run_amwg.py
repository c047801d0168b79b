#!/usr/bin/env python3
"""AMWG against the MH kernel of the same build, back to back on one GPU: the cfg 4 swiss job (the swiss logistic regression,
262,144 chains, 32 transitions per launch, running sums on) with MH(sigma = 0.1) and MuvAMWG(sigma = 0.1) under RobertsRosenthalMCTuner(0.44, 50), then a
D = 8 and a D = 32 closure (Gaussians with condition number 50) the same way.  The two samplers alternate, five rounds; transitions/s from the library's
own event timing (klara_last_run_ms), the median of the five; the kernels' registers and scratch from the loaded code objects.  An AMWG transition is D
coordinate updates, each one evaluation of the target plus a draw — what an MH transition is — so the figure to read is AMWG's time per coordinate
update over MH's time per transition.  Writes the measured block of profiles/amwg.txt (or of the file given as third argument) and keeps that file's
commentary from "Reading:" on.
usage: run_amwg.py [nchains] [transitions] [output file]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import amwg_cases as WC  # noqa: E402
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 320
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(label, target, x0, nsteps):
    d = target.ndims
    samplers = (("MH", dict(sampler=L.SAMPLER_MH, mh_sigma=np.full(d, 0.1))),
                ("AMWG", dict(amwg_logsigma0=np.full(d, 2.0 * np.log(0.1)), **WC.amwg(targetrate=0.44, period=50))))      # sqrt(exp(logσ)) = 0.1: MH's scale
    eng, r = {}, {name: [] for name, _ in samplers}
    for name, kw in samplers:
        e = K.Engine(target=target, nchains=n, nsteps=10 ** 6, steps_per_launch=32, monitor=L.MON_SUMMARIES, **kw)
        e.set_state(x0)
        e.run(64)                                                        # warm-up (clocks, code objects; one tuning event)
        eng[name] = e
    for _ in range(5):                                                   # the two alternate: what else runs on the box meets both
        for name, _ in samplers:
            eng[name].run(nsteps)
            ms, nl = eng[name].last_run_ms()
            r[name].append(n * nsteps / (ms * 1e-3))
    rates = {}
    for name, _ in samplers:
        e = eng[name]
        acc, tot = e.accept_counts()
        v, sc, lds = e.kernel_attributes(0, 32)
        rates[name] = float(np.median(r[name]))
        extra = ""
        if name == "AMWG":
            ls, _, nacc = e.amwg_state()
            extra = (f", coordinate updates/s {rates[name] * d:.4g}, acceptance per coordinate {nacc.sum() / (n * tot * d):.3f}, "
                     f"mean logσ {ls.mean():.3f} (start {2.0 * np.log(0.1):.3f})")
        say(f"{label:18s} {name:4s} layout {e.layout()}: {rates[name]:.4g} transitions/s (median of 5 runs of {nsteps} transitions, {nl} launches each; "
            f"min {min(r[name]):.4g}, max {max(r[name]):.4g}), acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B{extra}")
        e.close()
    say(f"{label:18s} time per AMWG coordinate update / time per MH transition = {rates['MH'] / (rates['AMWG'] * d):.3f}   "
        f"(AMWG / MH in transitions/s = {rates['AMWG'] / rates['MH']:.3f})")


X, y = cases.swiss_data()
measure("swiss D=4 (cfg 4)", K.LogisticTarget(X, y, 100.0), np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((n, 4)), steps)
for d in (8, 32):
    P = WC.conditioned_precision(d, 50.0, seed=d)
    measure(f"closure D={d}", WC.quad_target(0.5, P), 0.5 * np.random.default_rng(2).standard_normal((n, d)), max(32, steps // (d // 8)))
HEADER = """AMWG (KLARA_SAMPLER_AMWG, RobertsRosenthalMCTuner) against the MH kernel of the same build — scripts/run_amwg.py on one MI355X, the two samplers alternating on the same box
===========================================================================================================================================================================
%s chains, 32 transitions per launch, running sums on; MH sigma = 0.1, MuvAMWG(fill(0.1, D)) as logσ0 = 2 log 0.1 with targetrate 0.44, period 50.  Transitions/s from
klara_last_run_ms, median of five runs after a 64-transition warm-up.  The yardstick is the unchanged MH kernel of this commit.

"""
MARK = "\nReading:"          # everything from here on in the committed file is commentary: kept as it is
out = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "amwg.txt"
committed = (ROOT / "profiles" / "amwg.txt").read_text() if (ROOT / "profiles" / "amwg.txt").exists() else ""
tail = committed[committed.index(MARK):] if MARK in committed else "\n"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(HEADER % (f"{n:,}") + "\n".join(lines) + "\n" + tail)
