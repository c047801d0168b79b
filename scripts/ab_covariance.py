#!/usr/bin/env python3
"""Cost of the pooled covariance monitor (KLARA_MON_COVARIANCE), same box, one process: job-level transitions/s with and without the bit, alternating,
median of 5 timed regions each, at the headline shape (MALA on -x.x, 65,536 x 100, 32 transitions per launch, thinning 1) and at the BASELINE cfg 3
shape (HMC L = 10 on the dense Gaussian, 65,536 x 100); and, as comparator, torch's x.T @ x over a buffer of the shape of one launch's 32 ring
columns (32 x 65,536 samples of 100 doubles) — the route tests/test_gpu_workloads.py takes for cfg 3's covariances.

  scripts/ab_covariance.py                 the A/B and the comparator (profiler off)
  scripts/ab_covariance.py --profile-job   the headline job with the bit alone, 512 transitions: run it under `rocprofv3 --kernel-trace --stats`
                                           in a run of its own; k_cov_update's mean time is the kernel time of one launch's update

Work of one update from shapes: 28 upper tiles x 256 elements x 2 flop per sample -> 14,336 flop per sample, 3.0e10 per launch of 32 x 65,536
samples (lower bound 0.38 ms at 78.6 TFLOP/s FP64 MFMA); 800 B read per sample, 1.68 GB per launch (0.27 ms at 6.3 TB/s achievable): compute binds."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import klara_jl_amd as K  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

N, D = 65536, 100
FLOP_PER_LAUNCH = 28 * 256 * 2 * 32 * N
BYTES_PER_LAUNCH = 32 * N * D * 8
PEAK_TF, PEAK_BW = 78.6, 6.3e12


def make(shape, cov):
    if shape == "headline":
        kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.9, monitor=L.MON_SUMMARIES | (L.MON_COVARIANCE if cov else 0))
    else:
        kw = dict(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget.compound_symmetric(D, 0.5), leapstep=0.1, nleaps=10, monitor=L.MON_COVARIANCE if cov else 0)
    e = K.Engine(nchains=N, nsteps=10 ** 7, burnin=0, seed=20260927, **kw)
    e.init_state_normal()
    return e


def region(e, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run(steps)                                   # (synchronous on return)
    return N * steps / (time.perf_counter() - t0)


def ab(shape, steps, warm):
    eng = {False: make(shape, False), True: make(shape, True)}
    for e in eng.values():
        e.run(warm)
    rates = {False: [], True: []}
    for _ in range(5):
        for cov in (False, True):
            rates[cov].append(region(eng[cov], steps))
    for e in eng.values():
        e.close()
    a, b = statistics.median(rates[False]), statistics.median(rates[True])
    spread = lambda r: (max(r) - min(r)) / statistics.median(r)
    print(f"{shape}: {steps} transitions per region, 65,536 x 100: without the bit {a:.4g} transitions/s (spread {spread(rates[False]):.1%}), "
          f"with it {b:.4g} (spread {spread(rates[True]):.1%}): x{b / a:.3f}; per launch of 32: {32 * N / a * 1e3:.3f} ms -> {32 * N / b * 1e3:.3f} ms "
          f"(+{(32 * N / b - 32 * N / a) * 1e3:.3f} ms)")


def comparator():
    x = torch.randn(32 * N, D, dtype=torch.float64, device="cuda")
    for _ in range(3):
        g = x.T @ x
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            g = x.T @ x
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 10)
    t = statistics.median(ts)
    print(f"torch x.T @ x, x = (32 x 65,536) x 100 f64: {t * 1e3:.3f} ms per product ({2 * 32 * N * D * D / t / 1e12:.1f} TFLOP/s of its 2 n D^2; "
          f"the full square, no shift, no sums)  [{float(g[0, 0]):.3g}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile-job", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs the GPU")
    if args.profile_job:
        e = make("headline", True)
        e.run(512)
        mean, M, ns, nc = e.pooled_covariance()
        print(f"profile job: {ns} samples, trace(M) / (n - 1) = {np.trace(M) / (ns - 1):.6g}")
        e.close()
        return
    print(f"one update from shapes: {FLOP_PER_LAUNCH:.3g} flop -> {FLOP_PER_LAUNCH / PEAK_TF / 1e9:.3f} ms at {PEAK_TF} TFLOP/s; "
          f"{BYTES_PER_LAUNCH / 1e9:.2f} GB -> {BYTES_PER_LAUNCH / PEAK_BW * 1e3:.3f} ms at {PEAK_BW / 1e12} TB/s")
    ab("headline", 8192, 2048)
    ab("cfg3", 1024, 256)
    comparator()


if __name__ == "__main__":
    main()
