"""Regenerates the RAM golden vectors under tests/golden/ from the CPU reference (oracle/klara_oracle.c ko_ram).

    python tests/golden/make_golden_ram.py

ram_swiss.npz: the swiss example (RAM(ones(4)), lambda = 100) on the row-split logistic kernels; ram_gauss_d3.npz: a correlated Gaussian as a
user-defined closure with a non-diagonal initial factor.  Each holds x0 and the reference's accept mask, final state, log-target and factors;
tests/test_ram_host.py checks that the reference still reproduces them, tests/test_gpu_ram.py that the kernels do.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import ram_cases as RC  # noqa: E402

GOLDEN = {"ram_swiss": "swiss_example", "ram_gauss_d3": "gauss_d3"}


def run_case(name):
    c = RC.make(name)
    job = RC.ref_job(c)
    assert job.set_state(c["x0"]) == 0
    assert job.run(c["nsteps"]) == 0
    return dict(x0=c["x0"], accept=job.accept, X=job.X, LT=job.LT, S=job.S, skipped=np.int64(job.skipped))


if __name__ == "__main__":
    for fname, case in GOLDEN.items():
        np.savez_compressed(Path(__file__).resolve().parent / f"{fname}.npz", **run_case(case))
        print("wrote", fname)
