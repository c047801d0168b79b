"""Regenerates the golden vectors of the SMMALA sampler with the softabs transform under tests/golden/ from the CPU reference
(oracle/klara_oracle.c ko_smmala).

    python tests/golden/make_golden_softabs.py

softabs_banana.npz: the banana through KLARA_USER_AUTODIFF 2, start states with an indefinite Hessian among them;
softabs_doublewell_d8.npz: the coupled double well at D = 8 (VanillaMCTuner(verbose=true));
softabs_diag_d4.npz: a diagonal tensor with a zero entry (no rotation, f(0) = 1 / a).
Each holds x0 and the reference's accept mask, final state, log-target, gradient and steps; tests/test_softabs_host.py checks that the
reference still reproduces them, tests/test_gpu_softabs.py that the kernels do.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import softabs_cases as SAC  # noqa: E402

GOLDEN = {"softabs_banana": "banana_ad2", "softabs_doublewell_d8": "doublewell_d8", "softabs_diag_d4": "diag_metric_d4"}


def run_case(name):
    c = SAC.make(name)
    job = SAC.ref_job(c)
    assert job.set_state(c["x0"]) == 0
    assert job.run(c["nsteps"]) == 0
    return dict(x0=c["x0"], accept=job.accept, X=job.X, LT=job.LT, G=job.G, step=job.step.copy())


if __name__ == "__main__":
    for fname, case in GOLDEN.items():
        np.savez_compressed(Path(__file__).resolve().parent / f"{fname}.npz", **run_case(case))
        print("wrote", fname)
