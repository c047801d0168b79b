#!/usr/bin/env python3
"""What the softabs transform of the SMMALA metric costs: SMMALA on the same user-defined quadratic targets (tests/smmala_cases.py SRC_QUAD_TENSOR,
N(0, P^-1), condition number 100) at D = 2, 4, 8 with the transform on the device (tensor = -P, smmala_softabs = 1000) and without it (tensor =
softabs(-P, 1000) formed on the host, so that the job can run): the same metric either way, same box, same process, alternating.  262,144 chains, 32
transitions per launch, transitions/s from the library's own event timing (klara_last_run_ms), median of 5; the kernels' registers / scratch / LDS;
the Jacobi sweeps a factorisation takes (host build of klara_softabs.h on the same matrix: the metric is constant, so every lane takes as many).
usage: run_softabs.py [nchains] [transitions]        (profiles/softabs.txt records a run)"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import klara_jl_amd as K  # noqa: E402
import smmala_cases as SC  # noqa: E402
import softabs_ref as SR  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402
from klara_jl_amd import stats  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 320
A = 1000.0
for d in (2, 4, 8):
    P = SC.conditioned_precision(d, 100.0, seed=d)
    x0 = np.random.default_rng(d).standard_normal((n, d)) * 0.3
    jobs = {"device softabs": (SC.quad_target(0.5, P, -P), A), "host-formed metric": (SC.quad_target(0.5, P, stats.softabs(-P, A)), 0.0)}
    eng, rates, info = {}, {}, {}
    for name, (target, a) in jobs.items():
        e = K.Engine(sampler=L.SAMPLER_SMMALA, target=target, nchains=n, nsteps=10 ** 6, steps_per_launch=32, monitor=L.MON_SUMMARIES,
                     driftstep=1.0, smmala_softabs=a)
        e.set_state(x0)
        e.run(64)                                                    # warm-up (clocks, code objects)
        eng[name], rates[name] = e, []
    for _ in range(5):                                               # alternating: A B A B ...
        for name, e in eng.items():
            e.run(steps)
            ms, nl = e.last_run_ms()
            rates[name].append(n * steps / (ms * 1e-3))
    for name, e in eng.items():
        acc, tot = e.accept_counts()
        v, sc, lds = e.kernel_attributes(0, 32)
        info[name] = float(np.median(rates[name]))
        print(f"D = {d} {name:18s} layout {e.layout()}: {info[name]:.4g} transitions/s (median of 5 runs of {steps} transitions; "
              f"min {min(rates[name]):.4g}, max {max(rates[name]):.4g}), acceptance {acc.sum() / (n * tot):.3f}, kernel VGPRs {v}, scratch {sc} B, "
              f"static LDS {lds} B", flush=True)
        e.close()
    sweeps = SR.softabs(-P, A)[1]
    print(f"D = {d}: device softabs / host-formed metric = {info['device softabs'] / info['host-formed metric']:.3f}; "
          f"Jacobi sweeps per factorisation: mean {sweeps}, max {sweeps}", flush=True)
