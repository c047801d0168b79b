#!/usr/bin/env python3
"""AM against the MH and RAM kernels of the same build, back to back on one GPU: the cfg 4 swiss job (the swiss logistic
regression, 262,144 chains, 32 transitions per launch, running sums on) with MH(sigma = 0.1), RAM(S0 = 0.1 I) and AM(C0 = 0.01 I), then a D = 8
closure (a Gaussian with condition number 50) the same way.  The three samplers alternate, five rounds; transitions/s from the library's own
event timing (klara_last_run_ms), the median of the five; the kernels' registers and scratch from the loaded code objects.  Writes the measured block
of profiles/am.txt (or of the file given as third argument) and keeps that file's commentary and the section on the kernels' registers, which
comes from the cross-compile and not from a run.
usage: run_am.py [nchains] [transitions] [output file]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
import smmala_cases as SC  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 320
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def measure(label, target, x0):
    d = target.ndims
    samplers = (("MH", dict(sampler=L.SAMPLER_MH, mh_sigma=np.full(d, 0.1))),
                ("RAM", dict(sampler=L.SAMPLER_RAM, ram_S0=0.1 * np.eye(d), ram_targetrate=0.234, ram_gamma=0.7)),
                ("AM", dict(sampler=L.SAMPLER_AM, am_C0=0.01 * np.eye(d), am_corescale=2.38 ** 2 / d, am_minorscale=0.01, am_c=0.05, am_t0=10)))
    eng, r = {}, {name: [] for name, _ in samplers}
    for name, kw in samplers:
        e = K.Engine(target=target, nchains=n, nsteps=10 ** 6, steps_per_launch=32, monitor=L.MON_SUMMARIES, **kw)
        e.set_state(x0)
        e.run(64)                                                        # warm-up (clocks, code objects; AM is past t0)
        eng[name] = e
    for _ in range(5):                                                   # the three alternate: what else runs on the box meets all of them
        for name, _ in samplers:
            eng[name].run(steps)
            ms, nl = eng[name].last_run_ms()
            r[name].append(n * steps / (ms * 1e-3))
    rates = {}
    for name, _ in samplers:
        e = eng[name]
        acc, tot = e.accept_counts()
        v, sc, lds = e.kernel_attributes(0, 32)
        extra = f", skipped updates {e.ram_factor()[1]}" if name == "RAM" else f", fallbacks {e.am_state()[3]}" if name == "AM" else ""
        rates[name] = float(np.median(r[name]))
        say(f"{label:18s} {name:3s} layout {e.layout()}: {rates[name]:.4g} transitions/s (median of 5 runs of {steps} transitions, {nl} launches each; "
            f"min {min(r[name]):.4g}, max {max(r[name]):.4g}), acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B{extra}")
        e.close()
    say(f"{label:18s} AM / MH = {rates['AM'] / rates['MH']:.3f}, AM / RAM = {rates['AM'] / rates['RAM']:.3f}, RAM / MH = {rates['RAM'] / rates['MH']:.3f}")


X, y = cases.swiss_data()
measure("swiss D=4 (cfg 4)", K.LogisticTarget(X, y, 100.0), np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((n, 4)))
P = SC.conditioned_precision(8, 50.0, seed=8)
measure("closure D=8", SC.quad_target(0.5, P, P), 0.5 * np.random.default_rng(2).standard_normal((n, 8)))
HEADER = """AM (KLARA_SAMPLER_AM) against the MH and RAM kernels of the same build — scripts/run_am.py on one MI355X, the three samplers alternating on the same box
=====================================================================================================================================================
%s chains, 32 transitions per launch, running sums on; MH sigma = 0.1, RAM S0 = 0.1 I (targetrate 0.234, gamma 0.7), AM C0 = 0.01 I (corescale 2.38^2 / D,
minorscale 0.01, c = 0.05, t0 = 10: every timed transition is an adaptive one).  Transitions/s from klara_last_run_ms, median of five runs of %s transitions
after a 64-transition warm-up.  The yardsticks are the unchanged MH and RAM kernels of this commit.

"""
MARK = "\nReading:"          # everything from here on in the committed file is commentary and the cross-compile's register table: kept as it is
out = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "am.txt"
committed = (ROOT / "profiles" / "am.txt").read_text() if (ROOT / "profiles" / "am.txt").exists() else ""
tail = committed[committed.index(MARK):] if MARK in committed else "\n"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(HEADER % (f"{n:,}", steps) + "\n".join(lines) + "\n" + tail)
