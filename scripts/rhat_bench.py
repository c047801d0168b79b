"""Times klara_gather_rhat (profiles/rhat.txt).  Unsplit: 65,536 chains x D = 100 against klara_gather_moments on the same handle.  Split: 4,096 chains x
D = 100 x 1,000 saved steps (3.3 GB of history) — bytes read over the HBM peak — against the read-back alternative, Engine.chain for every chain and
stats.rhat on the host.  Medians of repeated timed calls after warm-up; every call ends with its own device-to-host copy and synchronisation.
    python scripts/rhat_bench.py [--out profiles/rhat.txt] [--skip-readback]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rhat.txt"))
    ap.add_argument("--skip-readback", action="store_true")
    a = ap.parse_args()
    lines = ["R-hat on the device (scripts/rhat_bench.py): wall time per call, host side, each call with its device-to-host copy and synchronisation;",
             "median (min .. max) of the timed calls after warm-up, one process, one MI355X, all figures from the same run.", ""]

    D = 100
    N = 65536
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=120, burnin=20, driftstep=0.05, monitor=L.MON_SUMMARIES,
                   seed=5)
    eng.init_state_normal(); eng.run(120)
    tm = timed(eng.pooled_moments, 30, 300)
    tr = timed(eng.rhat, 30, 300)
    r = eng.rhat()
    lines += [f"unsplit, {N} chains x D = {D}, 100 saved steps (from the running sums, no history), 300 timed calls after 30",
              f"  klara_gather_moments   {tm[0] * 1e6:8.1f} us  ({tm[1] * 1e6:.1f} .. {tm[2] * 1e6:.1f})",
              f"  klara_gather_rhat      {tr[0] * 1e6:8.1f} us  ({tr[1] * 1e6:.1f} .. {tr[2] * 1e6:.1f})",
              f"  ratio rhat / moments   {tr[0] / tm[0]:8.2f}",
              f"  R-hat over the dimensions: {r['rhat'].min():.4f} .. {r['rhat'].max():.4f}", ""]
    eng.close()

    N, nsaved = 4096, 1000
    eng = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), nchains=N, nsteps=nsaved + 20, burnin=20, driftstep=0.05,
                   monitor=L.MON_SUMMARIES | L.MON_HISTORY, seed=5)
    eng.init_state_normal(); eng.run(nsaved + 20)
    ts = timed(lambda: eng.rhat(split=True), 5, 40)
    tu = timed(eng.rhat, 5, 40)
    rs = eng.rhat(split=True)
    nbytes = N * D * (2 * (nsaved // 2)) * 8
    lines += [f"split, {N} chains x D = {D} x {nsaved} saved steps ({nbytes / 1e9:.2f} GB of history read once), 40 timed calls after 5",
              f"  klara_gather_rhat(split) {ts[0] * 1e3:8.3f} ms  ({ts[1] * 1e3:.3f} .. {ts[2] * 1e3:.3f})",
              f"  history bytes / time     {nbytes / ts[0] / 1e12:8.2f} TB/s = {100 * nbytes / ts[0] / HBM_PEAK:.0f} % of the 8.0 TB/s HBM peak",
              f"  klara_gather_rhat(unsplit) on the same handle {tu[0] * 1e6:.1f} us",
              f"  split R-hat over the dimensions: {rs['rhat'].min():.4f} .. {rs['rhat'].max():.4f}"]
    if not a.skip_readback:
        t0 = time.perf_counter()
        v = np.empty((N, nsaved, D))
        for c in range(N):
            v[c] = eng.chain(c).T
        t1 = time.perf_counter()
        ref = K.stats.rhat(v, split=True)
        t2 = time.perf_counter()
        lines += [f"  the alternative: Engine.chain for all {N} chains {t1 - t0:.2f} s + stats.rhat on the host {t2 - t1:.2f} s = {t2 - t0:.2f} s"
                  f"  ({(t2 - t0) / ts[0]:.0f} x the device call); largest |device - host| / host {np.max(np.abs(rs['rhat'] - ref) / ref):.2e}"]
    eng.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
