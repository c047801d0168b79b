#!/usr/bin/env python3
"""SMMALA against MALA on the cfg 4 job: the swiss logistic regression, 262,144 chains on one GPU, the same steps_per_launch, running
sums on (MALA's step 0.1, SMMALA's 0.02 of doc/examples/swiss/SMMALA/analytical.jl); transitions/s from the library's own event timing (klara_last_run_ms) and the kernels' registers / scratch.
usage: run_smmala.py [nchains] [transitions]        (profiles/smmala_swiss.txt records a run with its rocprofv3 summary)"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cases  # noqa: E402
import klara_jl_amd as K  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 640
X, y = cases.swiss_data()
x0 = np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((n, 4))
rates = {}
for name, sampler, h in (("MALA", L.SAMPLER_MALA, 0.1), ("SMMALA", L.SAMPLER_SMMALA, 0.02)):
    e = K.Engine(sampler=sampler, target=K.LogisticTarget(X, y, 100.0), nchains=n, nsteps=10 ** 6, steps_per_launch=32,
                 monitor=L.MON_SUMMARIES, driftstep=h)
    e.set_state(x0)
    e.run(64)                                                        # warm-up (clocks, code objects)
    best = 0.0
    for _ in range(3):
        e.run(steps)
        ms, nl = e.last_run_ms()
        best = max(best, n * steps / (ms * 1e-3))
    acc, tot = e.accept_counts()
    v, sc, lds = e.kernel_attributes(0, 32)
    rates[name] = best
    print(f"{name:6s} layout {e.layout()}: {best:.4g} transitions/s (best of 3 runs of {steps} transitions, {nl} launches each), "
          f"acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B, static LDS {lds} B", flush=True)
    e.close()
print(f"SMMALA / MALA = {rates['SMMALA'] / rates['MALA']:.3f}")
