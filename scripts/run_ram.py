#!/usr/bin/env python3
"""RAM against the MH kernel of the same build, back to back on one GPU: the cfg 4 swiss job (the swiss logistic regression,
262,144 chains, 32 transitions per launch, running sums on) with MH(sigma = 0.1) and RAM(S0 = 0.1 I), then a D = 8 logistic job and a D = 3
closure the same way.  Transitions/s from the library's own event timing (klara_last_run_ms), the median of five runs; the kernels' registers and
scratch from the loaded code objects.  Writes the measured block of profiles/ram.txt (or of the file given as third argument) and keeps that file's
section on the kernels' registers, which comes from the cross-compile and not from a run.
usage: run_ram.py [nchains] [transitions] [output file]"""
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
    rates = {}
    for name, kw in (("MH", dict(sampler=L.SAMPLER_MH, mh_sigma=np.full(d, 0.1))),
                     ("RAM", dict(sampler=L.SAMPLER_RAM, ram_S0=0.1 * np.eye(d), ram_targetrate=0.234, ram_gamma=0.7))):
        e = K.Engine(target=target, nchains=n, nsteps=10 ** 6, steps_per_launch=32, monitor=L.MON_SUMMARIES, **kw)
        e.set_state(x0)
        e.run(64)                                                        # warm-up (clocks, code objects)
        r = []
        for _ in range(5):
            e.run(steps)
            ms, nl = e.last_run_ms()
            r.append(n * steps / (ms * 1e-3))
        acc, tot = e.accept_counts()
        v, sc, lds = e.kernel_attributes(0, 32)
        extra = ""
        if name == "RAM":
            extra = f", skipped updates {e.ram_factor()[1]}"
        rates[name] = float(np.median(r))
        say(f"{label:18s} {name:3s} layout {e.layout()}: {rates[name]:.4g} transitions/s (median of 5 runs of {steps} transitions, {nl} launches each; "
            f"min {min(r):.4g}, max {max(r):.4g}), acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B{extra}")
        e.close()
    say(f"{label:18s} RAM / MH = {rates['RAM'] / rates['MH']:.3f}")


X, y = cases.swiss_data()
measure("swiss D=4 (cfg 4)", K.LogisticTarget(X, y, 100.0), np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((n, 4)))
X8, y8 = cases.synthetic_logit(200, 8, seed=19)
measure("logistic D=8", K.LogisticTarget(X8, y8, 25.0), 0.3 * np.random.default_rng(1).standard_normal((n, 8)))
P = SC.conditioned_precision(3, 50.0, seed=3)
measure("closure D=3", SC.quad_target(0.5, P, P), 0.5 * np.random.default_rng(2).standard_normal((n, 3)))
HEADER = """RAM (KLARA_SAMPLER_RAM) against the MH kernel of the same build — scripts/run_ram.py on one MI355X, both samplers back to back on the same box
================================================================================================================================================
%s chains, 32 transitions per launch, running sums on, sigma = S0 = 0.1 I, RAM targetrate 0.234, gamma 0.7; transitions/s from klara_last_run_ms,
median of five runs of %s transitions after a 64-transition warm-up.  The yardstick is the unchanged MH kernel (k_transitions<MH, ...>) of this commit.

"""
MARK = "\nReading:"          # everything from here on in the committed file is commentary and the cross-compile's register table: kept as it is
out = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "ram.txt"
committed = (ROOT / "profiles" / "ram.txt").read_text() if (ROOT / "profiles" / "ram.txt").exists() else ""
tail = committed[committed.index(MARK):] if MARK in committed else "\n"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(HEADER % (f"{n:,}", steps) + "\n".join(lines) + "\n" + tail)
