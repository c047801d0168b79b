#!/usr/bin/env python3
"""Cost of the derived quantities (klara_desc.derived_nout > 0; klara.jl_amd/csrc/klara_derived.h), one GPU, one process, one session.  Three blocks:

1. One update of 32 x 65,536 samples at D = 100 (1.68 GB of the value ring read once).  Jobs that differ only in what consumes the ring run back to back,
   alternating, five rounds of 512 transitions = 16 launches of 32; the per-launch time is the library's own event timing (klara_last_run_ms) over the
   launches, the median of the five; a consumer's update is its job's time minus that of the job that only stores the ring.  Consumers: the marginals at
   64 bins (k_marg_update), closure (a) and closure (b) at K = 2, each without and with 64-bin histograms of the outputs.  Beside them the time to read
   the 1.68 GB once at this box's copy rate, measured in the same run (a device-to-device copy of that many bytes: bytes read + bytes written over time).
2. The headline job (MALA on -x.x, 65,536 x 100, running sums on) at thinning 1 and 10: transitions/s without a consumer, with the marginals alone (64
   bins), with closure (a), with closure (a) and its histograms; the same alternation, wall-clock regions of 4,096 transitions.
3. The swiss logistic regression (BASELINE cfg 4's per-GPU share: 32,768 chains, MALA h = 0.1, 50 transitions per launch, running sums on) without and
   with closure (c), the predictive probability at a covariate row, with 64-bin histograms over [0, 1].
The kernel's registers and scratch in profiles/derived.txt come from cross-compiling the same translation unit, not from this run.

4. With --parent-root DIR (a built checkout of the parent commit): the headline job without the feature in this tree and in the parent's, a process each.

usage: run_derived.py [output file] [--parent-root DIR]"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import cases  # noqa: E402
import derived_cases as DC  # noqa: E402
import klara_jl_amd as K  # noqa: E402
import torch  # noqa: E402
from klara_jl_amd import _lib as L  # noqa: E402

N, D = 65536, 100
BYTES = 32 * N * D * 8
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def copy_rate():
    """bytes moved per second by a device-to-device copy of one update's bytes: median of 7 after 2 warm-up copies"""
    a = torch.empty(BYTES // 8, dtype=torch.float64, device="cuda").normal_()
    b = torch.empty_like(a)
    t = []
    for i in range(9):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    del a, b
    return 2 * BYTES / statistics.median(t[2:])


def consumers(with_plain):
    hist64 = K.Marginals(64, -4.0, 4.0)
    c = [("marginals, 64 bins", dict(marginals=hist64)),
         ("closure (a), K = 2", dict(derived=K.Derived(DC.K_A, DC.SRC_A))),
         ("closure (a) + 64-bin histograms", dict(derived=K.Derived(DC.K_A, DC.SRC_A, marginals=K.Marginals(64, -6.0, 6.0)))),
         ("closure (b), K = 2", dict(derived=K.Derived(DC.K_B, DC.SRC_B))),
         ("closure (b) + 64-bin histograms", dict(derived=K.Derived(DC.K_B, DC.SRC_B, marginals=K.Marginals(64, [-40.0, 0.0], [40.0, 120.0]))))]
    return ([("no consumer", dict())] if with_plain else []) + c


def headline(thinning, monitor, **kw):
    e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.9, monitor=monitor, nchains=N, nsteps=10 ** 7, burnin=0,
                 thinning=thinning, seed=20260927, **kw)
    e.init_state_normal()
    return e


def block_update(bw):
    say(f"1. one update: 32 saved steps x {N} chains x {D} dimensions = {BYTES / 1e9:.2f} GB read once; at this box's copy rate of {bw / 1e12:.2f} TB/s "
        f"(bytes read + written of a device-to-device copy of that size): {BYTES / bw * 1e3:.3f} ms")
    jobs = [("ring only", dict(monitor=L.MON_SUMMARIES | L.MON_HISTORY, hist_ring_cols=32, nstreams=1))] + \
           [(name, dict(monitor=L.MON_SUMMARIES, **kw)) for name, kw in consumers(False)]
    eng = {name: headline(1, **kw) for name, kw in jobs}
    per = {name: [] for name, _ in jobs}
    for e in eng.values():
        e.run(256)
    for _ in range(5):
        for name, _ in jobs:
            eng[name].run(512)
            ms, nl = eng[name].last_run_ms()
            per[name].append(ms / nl)
    base = statistics.median(per["ring only"])
    say(f"   per launch of 32 transitions (median of 5 runs of 16 launches; event time): the MALA kernel storing its values to the ring alone {base:.3f} ms")
    marg = None
    for name, _ in jobs[1:]:
        m = statistics.median(per[name]); upd = m - base
        marg = upd if marg is None else marg
        say(f"   {name:34s} {m:.3f} ms (min {min(per[name]):.3f}, max {max(per[name]):.3f})  update {upd:.3f} ms = {upd / (BYTES / bw * 1e3):.2f} x the read, "
            f"{upd / marg:.2f} x k_marg_update at 64 bins")
    for e in eng.values():
        e.close()


def block_headline():
    say("2. headline job (MALA, -x.x, 65,536 x 100, running sums on), transitions/s, median of 5 wall-clock regions of 4,096 transitions, jobs alternating:")
    for thinning in (1, 10):
        jobs = consumers(True)[:4]
        eng = {name: headline(thinning, L.MON_SUMMARIES, **kw) for name, kw in jobs}
        r = {name: [] for name, _ in jobs}
        for e in eng.values():
            e.run(1024)
        for _ in range(5):
            for name, _ in jobs:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                eng[name].run(4096)
                r[name].append(N * 4096 / (time.perf_counter() - t0))
        base = statistics.median(r["no consumer"])
        for name, _ in jobs:
            m = statistics.median(r[name])
            say(f"   thinning {thinning:2d}  {name:34s} {m:.4g} (spread {(max(r[name]) - min(r[name])) / m:.1%})  x{m / base:.3f}")
        for e in eng.values():
            e.close()


def block_swiss():
    X, y = cases.swiss_data()
    nc = 32768
    x0 = np.array([5.1, -0.9, 8.2, -4.5])[None, :] + 0.1 * np.random.default_rng(0).standard_normal((nc, 4))
    der = K.Derived(DC.K_C, DC.SRC_C, data=X[3], marginals=K.Marginals(64, 0.0, 1.0))
    jobs = [("no consumer", dict()), ("closure (c) + 64-bin histograms", dict(derived=der))]
    eng, r = {}, {name: [] for name, _ in jobs}
    for name, kw in jobs:
        e = K.Engine(sampler=L.SAMPLER_MALA, target=K.LogisticTarget(X, y, 100.0), nchains=nc, nsteps=10 ** 6, burnin=1000, driftstep=0.1, steps_per_launch=50,
                     monitor=L.MON_SUMMARIES, **kw)
        e.set_state(x0); e.run(1000)
        eng[name] = e
    for _ in range(5):
        for name, _ in jobs:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            eng[name].run(1000)
            r[name].append(nc * 1000 / (time.perf_counter() - t0))
    say("3. swiss logistic regression (cfg 4's per-GPU share: 32,768 chains, MALA, 50 transitions per launch, running sums on), transitions/s, median of 5 regions of 1,000:")
    base = statistics.median(r["no consumer"])
    for name, _ in jobs:
        m = statistics.median(r[name])
        say(f"   {name:34s} {m:.4g} (spread {(max(r[name]) - min(r[name])) / m:.1%})  x{m / base:.3f}")
    mean, m2, ns, _ = eng[jobs[1][0]].derived_moments()
    q = K.histogram_quantiles(eng[jobs[1][0]].derived_histogram()[0], 64, 0.0, 1.0, [0.025, 0.975])
    say(f"   predicted probability at covariate row 3: posterior mean {mean[0]:.4f}, sd {np.sqrt(m2[0] / ns):.4f}, 95 % interval [{q[0, 0]:.3f}, {q[0, 1]:.3f}] from {ns} samples")
    for e in eng.values():
        e.close()


_PARENT_CHILD = r"""
import json, statistics, sys, time
sys.path.insert(0, sys.argv[1])
import torch
import klara_jl_amd as K
from klara_jl_amd import _lib as L
N, D = 65536, 100
e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(D), driftstep=0.9, monitor=L.MON_SUMMARIES, nchains=N, nsteps=10 ** 7, burnin=0, seed=20260927)
e.init_state_normal(); e.run(1024)
r = []
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    e.run(4096)
    r.append(N * 4096 / (time.perf_counter() - t0))
e.close()
print(json.dumps(dict(rate=statistics.median(r), spread=(max(r) - min(r)) / statistics.median(r))))
"""


def block_parent(parent_root):
    """the headline job without the feature, this tree against a built checkout of the parent commit: a process of its own per line (the descriptor grew, so
    one binding cannot drive both libraries), parent and this tree alternating, twice each"""
    import json
    import subprocess
    say("4. headline job without the feature, this tree against the parent commit's (a process each, alternating; median of 5 regions of 4,096 transitions):")
    rates = {"parent": [], "this": []}
    for name, root in (("parent", parent_root), ("this", ROOT), ("parent", parent_root), ("this", ROOT)):
        r = subprocess.run([sys.executable, "-c", _PARENT_CHILD, str(root)], capture_output=True, text=True, timeout=600, cwd=str(root))
        if r.returncode != 0:
            sys.exit(f"child ({root}) failed:\n{r.stderr[-3000:]}")
        d = json.loads(r.stdout.strip().splitlines()[-1])
        rates[name].append(d["rate"])
        say(f"   {name:6s} {d['rate']:.4g} transitions/s (spread {d['spread']:.1%})")
    say(f"   this / parent = {statistics.mean(rates['this']) / statistics.mean(rates['parent']):.3f} (means of the two lines each)")


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("output", nargs="?", default=None, help="file the measured block is written to")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: adds block 4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs the GPU")
    say(f"derived quantities on {torch.cuda.get_device_name(0)}: scripts/run_derived.py")
    block_update(copy_rate())
    block_headline()
    block_swiss()
    if args.parent_root:
        block_parent(Path(args.parent_root).resolve())
    if args.output:
        Path(args.output).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
