"""Regenerates the SMMALA golden vectors under tests/golden/ from the CPU reference (oracle/klara_oracle.c ko_smmala).

    python tests/golden/make_golden_smmala.py

smmala_swiss.npz: the swiss example (SMMALA(0.02), AcceptanceRateMCTuner(0.5), lambda = 100) on the row-split logistic kernels;
smmala_bivariate.npz: the BivariateNormal example (SMMALA(1.25) with the softabs metric formed on the host) on a user-defined target.
Each holds x0 and the reference's accept mask, final state, log-target, gradient and tuned steps; tests/test_smmala_host.py checks that the
reference still reproduces them, tests/test_gpu_smmala.py that the kernels do.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import smmala_cases as SC  # noqa: E402

GOLDEN = {"smmala_swiss": "swiss_example", "smmala_bivariate": "bivariate_example"}


def run_case(name):
    c = SC.make(name)
    job = SC.ref_job(c)
    assert job.set_state(c["x0"]) == 0
    assert job.run(c["nsteps"]) == 0
    return dict(x0=c["x0"], accept=job.accept, X=job.X, LT=job.LT, G=job.G, step=job.step.copy())


if __name__ == "__main__":
    for fname, case in GOLDEN.items():
        np.savez_compressed(Path(__file__).resolve().parent / f"{fname}.npz", **run_case(case))
        print("wrote", fname)
