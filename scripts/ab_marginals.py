#!/usr/bin/env python3
"""Cost of the pooled marginal histograms (klara_desc.marg_nbins > 0; klara.jl_amd/csrc/klara_marg.hip), same box, same session: job-level
transitions/s with and without marginals at thinning 1 and 10, median of 5 timed regions each, at the headline shape (MALA on -x.x, 65,536 x 100,
running sums on) and at the BASELINE cfg 3 shape (HMC L = 10 on the dense Gaussian, 65,536 x 100).  Every set of figures comes from a child process of
its own — this tree without marginals, this tree with them (64 and 1,024 bins), and, with --parent-root, the parent commit's tree (its own binding
and library: the descriptor grew, so one binding cannot drive both libraries).

  scripts/ab_marginals.py [--parent-root DIR]     the A/B (profiler off); DIR holds a built checkout of the parent commit
  scripts/ab_marginals.py --profile-job NBINS     the headline job with KLARA_MON_COVARIANCE and marginals of NBINS bins, 512 transitions: run it
                                                  under `rocprofv3 --kernel-trace --stats` in a run of its own; the mean times of k_marg_update and
                                                  k_cov_update are the kernel times of one launch's update, on the same box in the same session

One update from shapes: 32 saved steps x 65,536 chains x 100 dimensions = 2.1e8 samples, 8 B read per sample, 1.68 GB per launch: 0.266 ms at the
6.3 TB/s of achievable HBM bandwidth — the bound the update is expected to sit on: it reads the ring once and does one LDS add per sample."""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
N, D = 65536, 100
BYTES_PER_LAUNCH = 32 * N * D * 8
PEAK_BW = 6.3e12

_CHILD = r'''
import json, statistics, sys, time
root, nbins = sys.argv[1], int(sys.argv[2])
sys.path.insert(0, root)
import torch
import klara_jl_amd as K
from klara_jl_amd import _lib as L
N, D = 65536, 100

def make(shape, thinning):
    extra = dict(marginals=K.Marginals(nbins, -4.0, 4.0)) if nbins > 0 else {}
    if shape == "headline":
        kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.9, monitor=L.MON_SUMMARIES)
    else:
        kw = dict(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget.compound_symmetric(D, 0.5), leapstep=0.1, nleaps=10, monitor=0)
    e = K.Engine(nchains=N, nsteps=10 ** 7, burnin=0, thinning=thinning, seed=20260927, **kw, **extra)
    e.init_state_normal()
    return e

def region(e, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.run(steps)                                   # (synchronous on return)
    return N * steps / (time.perf_counter() - t0)

for shape, steps, warm in (("headline", 4096, 1024), ("cfg3", 512, 128)):
    for thinning in (1, 10):
        e = make(shape, thinning)
        e.run(warm)
        r = [region(e, steps) for _ in range(5)]
        e.close()
        print(json.dumps(dict(shape=shape, thinning=thinning, nbins=nbins, steps=steps, rate=statistics.median(r),
                              spread=(max(r) - min(r)) / statistics.median(r))), flush=True)
'''


def child(root, nbins):
    r = subprocess.run([sys.executable, "-c", _CHILD, str(root), str(nbins)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"child ({root}, nbins {nbins}) failed:\n{r.stderr[-3000:]}")
    return {(d["shape"], d["thinning"]): d for d in map(json.loads, r.stdout.strip().splitlines())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--profile-job", type=int, default=0, metavar="NBINS")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs the GPU")
    if args.profile_job:
        import numpy as np
        import klara_jl_amd as K
        from klara_jl_amd import _lib as L
        e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.9, monitor=L.MON_SUMMARIES | L.MON_COVARIANCE, nchains=N,
                     nsteps=10 ** 7, burnin=0, seed=20260927, marginals=K.Marginals(args.profile_job, -4.0, 4.0))
        e.init_state_normal()
        e.run(512)
        counts, _, ns, _ = e.pooled_histogram()
        _, M, _, _ = e.pooled_covariance()
        print(f"profile job, {args.profile_job} bins: {ns} samples per dimension, outer counts {int(counts[:, 0].sum())} / {int(counts[:, -1].sum())}, "
              f"trace(M) / (n - 1) = {np.trace(M) / (ns - 1):.6g}")
        e.close()
        return
    print(f"one update from shapes: {BYTES_PER_LAUNCH / 1e9:.2f} GB read once -> {BYTES_PER_LAUNCH / PEAK_BW * 1e3:.3f} ms at {PEAK_BW / 1e12} TB/s")
    sets = [("this, without", child(ROOT, 0))]
    if args.parent_root:
        sets.insert(0, ("parent, without", child(args.parent_root, 0)))
    sets += [("this, 64 bins", child(ROOT, 64)), ("this, 1024 bins", child(ROOT, 1024))]
    if args.parent_root:
        sets.append(("parent, without (again)", child(args.parent_root, 0)))
    base = sets[0][1]
    for key in (("headline", 1), ("headline", 10), ("cfg3", 1), ("cfg3", 10)):
        print(f"{key[0]}, thinning {key[1]}, 65,536 x 100, {base[key]['steps']} transitions per region, median of 5:")
        for name, res in sets:
            d = res[key]
            per = 32 * N / d["rate"] * 1e3
            print(f"    {name:24s} {d['rate']:.4g} transitions/s (spread {d['spread']:.1%})  x{d['rate'] / base[key]['rate']:.3f}   32 transitions: {per:.3f} ms")


if __name__ == "__main__":
    main()
