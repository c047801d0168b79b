"""Times the zero-variance control variates on the device (klara_get_chain_zv) and today's host route for the same estimator.

  python scripts/zv_bench.py --shape a|b [--reps 5] [--host-chains 256]      (--host-chains 0: device only, e.g. under rocprofv3)

  (a) swiss logistic regression   D = 4,   N = 65,536, n = 1,000 saved steps, lzv and qzv, per chain and pooled
  (b) dense Gaussian              D = 100, N = 8,192,  n = 512,               lzv, per chain

Per configuration: the whole call (the job's stream between two HIP events, and the host clock around the call — it ends in a
synchronise and includes the read-back of the results), the least traffic the call's passes need (both histories read once per pass) as a
share of the 8.0 TB/s HBM peak, the Gram stage's useful FP64 operations against the 78.6 TFLOP/s MFMA peak — both over the WHOLE call, so
they are end-to-end figures, not a kernel's share of peak —, and the host route: klara_get_chain + klara_get_chain_fields per chain, then
stats.lzv / stats.qzv, for --host-chains chains on 16 threads.  Needs a GPU; prints one line per configuration."""
import argparse
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

HBM_PEAK = 8.0e12
MFMA_F64_PEAK = 78.6e12


def counts(d, n, nchains, order, pooled):
    """(bytes of least traffic, passes, useful Gram FLOP) of one call: per chain the histories are read by the mean pass, the Gram pass and
    the pass that applies the coefficients; the pooled form reads them once more (the chains' means are formed again after the solve)."""
    k = d if order == 1 else d * (d + 3) // 2
    passes = 4 if pooled else 3
    traffic = passes * 2 * nchains * n * d * 8
    flop = nchains * n * (k * (k + 1) + 2 * k * d)          # upper triangle of S_ff (k (k + 1) / 2 products) and S_fx (k d), 2 FLOP each
    return traffic, passes, flop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["a", "b"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-chains", type=int, default=256)
    ap.add_argument("--nchains", type=int, default=0, help="number of chains instead of the shape's (0: the shape's own)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("zv_bench.py measures on a GPU: torch.cuda.is_available() is False")
    import klara_jl_amd as K
    from klara_jl_amd import _lib as L
    from klara_jl_amd import stats as S
    import cases

    mon = L.MON_HISTORY | L.MON_HIST_GRAD
    stream = torch.cuda.Stream()
    if args.shape == "a":
        X, y = cases.swiss_data()
        nch, n, d = args.nchains or 65536, 1000, 4
        eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), nchains=nch, nsteps=n + 200, burnin=200, driftstep=0.1,
                       monitor=mon, stream=stream.cuda_stream)
        eng.set_state(np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(1).standard_normal((nch, d)))
        configs = [(1, False), (1, True), (2, False), (2, True)]
        label = "(a) swiss"
    else:
        nch, n, d = args.nchains or 8192, 512, 100
        eng = K.Engine(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(cases.compound_symmetric_precision(d)), nchains=nch, nsteps=n + 20, burnin=20,
                       leapstep=0.1, nleaps=8, monitor=mon, stream=stream.cuda_stream)
        eng.init_state_normal()
        configs = [(1, False)]
        label = "(b) dense Gaussian"
    eng.run(eng.nsteps)
    print(f"{label}: D = {d}, N = {nch}, n = {eng.saved_steps()}, layout {eng.layout()}", flush=True)
    for order, pooled in configs:
        eng.chain_zv(order, pooled)                                  # warm-up: code objects, the LDS limits of the kernels
        ev, host = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            coef, zm, zv, info, _ = eng.chain_zv(order, pooled)
            host.append(time.perf_counter() - t0)
            e1.record(stream)
            e1.synchronize()
            ev.append(e0.elapsed_time(e1) * 1e-3)
        traffic, passes, flop = counts(d, n, nch, order, pooled)
        t = float(np.median(ev))
        print(f"  {'qzv' if order == 2 else 'lzv'} {'pooled   ' if pooled else 'per chain'}: call {t * 1e3:9.2f} ms by HIP events (min {min(ev) * 1e3:.2f}, max {max(ev) * 1e3:.2f}; "
              f"host clock median {np.median(host) * 1e3:.2f} ms; {args.reps} calls) | least traffic {traffic / 1e9:.2f} GB in {passes} passes = "
              f"{traffic / t / HBM_PEAK * 100:.1f} % of HBM peak | Gram {flop / 1e9:.1f} GFLOP = {flop / t / MFMA_F64_PEAK * 100:.2f} % of the FP64 MFMA peak | "
              f"info != 0: {int((info != 0).sum())}", flush=True)
    # today's route: both histories to the host chain by chain, then the NumPy restatement, 16 threads
    m = min(args.host_chains, nch)
    for order in sorted({o for o, _ in configs}) if m > 0 else ():
        fn = S.lzv if order == 1 else S.qzv

        def one(c):
            v = eng.chain(c).T
            g = eng.chain_fields(c, False, True)[1].T
            return fn(v, g)[0].mean(axis=0)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(one, range(m)))
        dt = time.perf_counter() - t0
        print(f"  host route {'qzv' if order == 2 else 'lzv'}: {m} chains in {dt * 1e3:.1f} ms on 16 threads = {dt / m * 1e3:.3f} ms per chain "
              f"(x {nch} chains = {dt / m * nch:.1f} s)", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
