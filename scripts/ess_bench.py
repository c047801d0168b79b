"""Times klara_gather_ess (profiles/ess.txt).  (a) Streamed mode at 65,536 chains x D = 100 and 262,144 x 4, acov_maxlag = 31: time per call, the streamed
state's bytes over the HBM peak, against klara_get_chain_acov_mcvar on the same handle (which reads the same arrays once).  (b) History and split modes
at 4,096 chains x 1,000 saved steps x D = 100, maxlag = 127, against klara_get_chain_mcvar on the same handle and against reading the histories back and
stats.pooled_ess on the host (timed on 256 of the chains and scaled); the temporary memory.  (c) The cfg 4 swiss job at its mixing drift step and from a
dispersed start cut short: pooled ESS per second, pooled ESS against the sum of the per-chain ESS, R-hat.  Medians of repeated timed calls after warm-up;
every call ends with its own device-to-host copy and synchronisation.
    python scripts/ess_bench.py [--out profiles/ess.txt] [--skip-host]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import klara_jl_amd as K                                                    # noqa: E402
from klara_jl_amd import _lib as L                                          # noqa: E402

HBM_PEAK = 8.0e12                                                           # bytes / s, MI355X specification


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def fmt(t, unit=1e3, name="ms"):
    return f"{t[0] * unit:9.3f} {name}  ({t[1] * unit:.3f} .. {t[2] * unit:.3f})"


def streamed(lines, N, D, maxlag=31):
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=10 ** 6, driftstep=0.05, monitor=L.MON_SUMMARIES,
                   acov_maxlag=maxlag, steps_per_launch=32, seed=5)
    eng.init_state_normal(); eng.run(128)
    te = timed(lambda: eng.pooled_ess("streamed"), 5, 40)
    ta = timed(lambda: eng.chain_acov_mcvar(want=("imse",)), 3, 15)
    out = eng.pooled_ess("streamed")
    nbytes = (3 * (maxlag + 1) + 1) * N * D * 8
    lines += [f"(a) streamed, {N} chains x D = {D}, acov_maxlag = {maxlag}, 128 saved steps; S | head | tail | total = {nbytes / 1e9:.3f} GB read once",
              f"  klara_gather_ess(streamed)        {fmt(te)}   40 timed calls after 5",
              f"  state bytes / time                {nbytes / te[0] / 1e12:9.2f} TB/s = {100 * nbytes / te[0] / HBM_PEAK:.0f} % of the 8.0 TB/s HBM peak",
              f"  klara_get_chain_acov_mcvar(imse)  {fmt(ta)}   15 timed calls after 3 (returns {N * D * 8 / 1e6:.1f} MB to the host)",
              f"  ratio ess / acov_mcvar            {te[0] / ta[0]:9.2f}",
              f"  pooled ESS over the dimensions {out['ess'].min():.4g} .. {out['ess'].max():.4g} of {N * 128} draws; window exhausted in "
              f"{int(out['window_exhausted'].sum())} of {D}", ""]
    eng.close()


def history(lines, skip_host):
    N, D, nsaved, maxlag = 4096, 100, 1000, 127
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=nsaved, driftstep=0.05,
                   monitor=L.MON_SUMMARIES | L.MON_HISTORY, seed=5)
    eng.init_state_normal(); eng.run(nsaved)
    th = timed(lambda: eng.pooled_ess("history", maxlag), 2, 10)
    ts = timed(lambda: eng.pooled_ess("split", maxlag), 2, 10)
    tm = timed(lambda: eng.chain_mcvar(maxlag=maxlag, want=("imse",)), 2, 10)
    out, outs = eng.pooled_ess("history", maxlag), eng.pooled_ess("split", maxlag)
    tmp = 3 * (maxlag + 1) * N * D * 8 + (32 + 1) * N * D * 8
    lines += [f"(b) history and split, {N} chains x {nsaved} saved steps x D = {D}, maxlag = {maxlag} ({N * D * nsaved * 8 / 1e9:.2f} GB of history), 10 timed calls after 2",
              f"  klara_gather_ess(history)         {fmt(th)}",
              f"  klara_gather_ess(split)           {fmt(ts)}",
              f"  klara_get_chain_mcvar(imse, maxlag = {maxlag}) on the same handle {fmt(tm)}   ratio history / mcvar {th[0] / tm[0]:.2f}",
              f"  temporary device memory: {tmp / 1e9:.2f} GB (history), {2 * tmp / 1e9:.2f} GB (split) — 3 (maxlag + 1) + 33 doubles per series and state",
              f"  pooled ESS {out['ess'].min():.4g} .. {out['ess'].max():.4g} (split {outs['ess'].min():.4g} .. {outs['ess'].max():.4g}) of {N * nsaved} draws; "
              f"window exhausted in {int(out['window_exhausted'].sum())} of {D}"]
    if not skip_host:
        sub = 256
        t0 = time.perf_counter()
        v = np.empty((nsaved, sub, D))
        for c in range(sub):
            v[:, c, :] = eng.chain(c).T
        t1 = time.perf_counter()
        K.stats.pooled_ess(v, maxlag)
        t2 = time.perf_counter()
        f = N / sub
        lines += [f"  the alternative, timed on {sub} chains and scaled by {f:.0f}: Engine.chain {f * (t1 - t0):.1f} s + stats.pooled_ess on the host {f * (t2 - t1):.1f} s"
                  f" = {f * (t2 - t0):.1f} s  ({f * (t2 - t0) / th[0]:.0f} x the device call)"]
    lines += [""]
    eng.close()


def swiss(lines):
    import cases
    X, y = cases.swiss_data()
    N, steps = 32768, 640
    for label, drift, x0, run in (("mixing drift step 0.1, start near the mode", 0.1, np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((N, 4)), steps),
                                  ("dispersed start (sd 3 around the mode), cut short", 0.1, np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 3.0 * np.random.default_rng(0).standard_normal((N, 4)), 64)):
        eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), nchains=N, nsteps=10 ** 6, driftstep=drift, monitor=L.MON_SUMMARIES,
                       acov_maxlag=63, steps_per_launch=32, seed=5)
        eng.set_state(x0)
        eng.run(run)
        dt = eng.last_run_ms()[0] * 1e-3                                     # the device's own time for the launches of this run
        out = eng.pooled_ess("streamed")
        imse, _, n = eng.chain_acov_mcvar(want=("imse",))
        s, q, _ = eng.chain_sums()
        var = (q - s * s / n) / (n - 1)
        with np.errstate(all="ignore"):
            per = np.nansum(var / imse, axis=0)                              # a chain's ess = n mcvar_iid / mcvar_imse = var / mcvar_imse
        r = eng.rhat()["rhat"]
        lines += [f"(c) cfg 4 swiss MALA, {N} chains, {run} saved steps, {label}: {dt * 1e3:.1f} ms on the device",
                  f"  pooled ESS {np.array2string(out['ess'], precision=4)}  = {out['ess'].min() / dt:.4g} .. {out['ess'].max() / dt:.4g} per second; window exhausted {out['window_exhausted'].tolist()}",
                  f"  pooled ESS / sum of the per-chain ESS (imse, maxlag 63) {np.array2string(out['ess'] / per, precision=3)};  R-hat {np.array2string(r, precision=4)}"]
        eng.close()
    lines += [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ess.txt"))
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    lines = ["The pooled effective sample size on the device (scripts/ess_bench.py): wall time per call, host side, each call with its device-to-host copy and",
             "synchronisation; median (min .. max) of the timed calls after warm-up, one process, one MI355X, all figures from the same run.", ""]
    streamed(lines, 65536, 100)
    streamed(lines, 262144, 4)
    history(lines, a.skip_host)
    swiss(lines)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
