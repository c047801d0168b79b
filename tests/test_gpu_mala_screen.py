"""GPU tests (-m gpu) of the screened rejections of the 4-lane MALA table kernel (klara.jl_amd/csrc/klara_diagt.h diagt_mala_screen,
klara_mala_screen.h).

k_diagt<MALA, 13, 4, .., SCTAB> first draws a transition's normals into the proposal's registers, adds up sum x z and sum z^2 and asks the screen
whether every chain of the wavefront certainly rejects; if so the transition ends there, otherwise the literal arithmetic runs over the stored
normals.  The estimate must never reach a result, so small jobs are held to the oracle bit for bit — states, log-targets, gradients, accept masks
and counts, running sums (and the value history) — where a stale sum x^2 after a commit, a wavefront that skips a chain that accepts, normals
overwritten before the second pass, or a padding chain that is not "certain" would move bits or stall:

D: 97 (odd: half a last pair), 100, 102 (with the padding pair: the accept draw is the last pair's), 103, 104 (no padding pair: the screen compares
   against the guard below which the kernel does not draw).
chains: 1, 17 (a partial wavefront of 16 + 1), 81 (more than one workgroup's four groups).
40 transitions as launches of 32 + 8 and as five launches of 8, all on the table kernel (sparse_moves = 1: the 4-lane kernels at any acceptance).
driftstep 0.9: nearly every wavefront-transition is screened; 0.3: about every second proposal is accepted, the second pass runs in nearly every
   transition and the commit re-forms sum x^2 again and again; 0.02: every proposal is accepted; 2.5: outside the step range the bound is proven
   for — the launch screens nothing and every transition takes the second pass."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cases
import oracle_ffi as O
import klara_jl_amd as K
from klara_jl_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]

ROOT = Path(__file__).resolve().parent.parent
SUMS = L.MON_ACCEPT | L.MON_SUMMARIES
NSTEPS = 40


def _run_engine(d, h, sparse, nchains, spl, nstreams=1, monitor=SUMS, burnin=0, thinning=1):
    """the job on the device: every output as arrays, and the launches counted by kernel family"""
    kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(d), driftstep=h)
    if sparse:
        kw["sparse_moves"] = sparse
    case = dict(burnin=burnin, thinning=thinning, **kw, nchains=nchains, nsteps=NSTEPS, x0=None, seed=20261020,
                name=f"mala_d{d}_h{h}_{sparse}_{nchains}_{spl}_{nstreams}_{burnin}")
    eng = K.Engine(**cases.engine_kwargs(case, monitor=monitor, steps_per_launch=spl, nstreams=nstreams))
    layout = eng.layout()
    assert layout[:2] == (3, 8), layout
    eng.init_state_normal()
    eng.run(NSTEPS)
    out = {"accept": eng.accept_mask()}
    out["x"], out["lt"], out["g"] = eng.state()
    out["naccept"], nst = eng.accept_counts()
    assert nst == NSTEPS
    out["sum"], out["sumsq"], nsaved = eng.chain_sums()
    assert nsaved == len(range(burnin + 1, NSTEPS + 1, thinning))
    if monitor & L.MON_HISTORY:
        out["hist"] = np.stack([np.ascontiguousarray(eng.chain(c)) for c in range(nchains)])       # (chain, D, saved)
    cnt = [int(c) for c in eng.launch_modes()[0]]
    eng.close()
    return case, layout, out, cnt


def _job(d, h, sparse, nchains, spl, **kw):
    case, layout, out, cnt = _run_engine(d, h, sparse, nchains, spl, **kw)
    name = case["name"]
    nlaunch = -(-NSTEPS // spl)
    assert sum(cnt) == nlaunch and (sparse != 1 or cnt[0] == nlaunch) and (sparse != 2 or cnt[0] == 0), (name, cnt)
    hist = "hist" in out
    job = O.OracleJob(**cases.oracle_kwargs(case, layout=layout), want_hist=hist)
    assert job.init_state_normal() == 0
    assert job.run(NSTEPS) == 0
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    assert np.array_equal(out["accept"], job.accept), f"{name}: accept mask differs at {np.argwhere(out['accept'] != job.accept)[:5]}"
    assert same(out["x"], job.X), f"{name}: values differ"
    assert same(out["lt"], job.LT), f"{name}: log-target differs"
    assert same(out["g"], job.G), f"{name}: gradient differs"
    assert np.array_equal(out["naccept"], job.naccept), f"{name}: accept counts differ"
    assert same(out["sum"], job.sum), f"{name}: running sums differ"
    assert same(out["sumsq"], job.sumsq), f"{name}: running sums of squares differ"
    if hist:
        for c in range(nchains):
            assert same(out["hist"][c], job.hist[:, c, :].T), f"{name}: value history of chain {c} differs"
    return int(out["accept"].sum()), int(out["accept"].size)


@pytest.mark.parametrize("d", [97, 100, 102, 103, 104])
def test_screened_kernel_bit_for_bit_against_the_oracle(d):
    for nchains in (1, 17, 81):
        for spl in (32, 8):
            for h in (0.9, 0.3, 0.02, 2.5):
                acc, size = _job(d, h, 1, nchains, spl)
                print(f"d{d} n{nchains} {spl} per launch h{h}: accepted {acc} of {size} ({acc / size:.4f})")
                if h == 0.02:
                    assert acc > 0.9 * size
                if h == 0.3 and nchains == 81:      # both paths of the second pass, and wavefronts on either side of the vote
                    assert 0.1 * size < acc < 0.9 * size
                if h == 0.9 and nchains == 81:      # the screened path and the fallback both ran
                    assert 0 < acc < 0.5 * size


def test_history_and_burnin():
    acc, size = _job(100, 0.3, 1, 81, 32, monitor=SUMS | L.MON_HISTORY, burnin=7)
    assert 0 < acc < size
    acc, size = _job(97, 0.9, 1, 81, 8, monitor=SUMS | L.MON_HISTORY, burnin=7)
    assert 0 < acc < size


def test_two_streams():
    for h in (0.9, 0.3):
        acc, size = _job(100, h, 1, 81, 32, nstreams=2)
        assert 0 < acc < size


@pytest.mark.parametrize("sparse", [0, 2])
def test_kernel_choice_moves_no_bit(sparse):
    """the device's own choice (0) and the 8-lane kernels (2) against the same oracle job as the screened 4-lane kernel (1)"""
    for h in (0.9, 0.3):
        _job(100, h, sparse, 81, 32)
        _job(103, h, sparse, 17, 8)


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_mala_screen as T
res = {{}}
for d, h, n, spl in {jobs!r}:
    _, _, out, cnt = T._run_engine(d, h, 1, n, spl)
    assert cnt[0] == -(-T.NSTEPS // spl), cnt
    for k, v in out.items():
        res[f"{{d}}_{{h}}_{{n}}_{{spl}}_{{k}}"] = np.ascontiguousarray(v)
np.savez({dest!r}, **res)
"""


def _library_without_the_screen():
    """klara.jl_amd/lib/libklara_hip_noscreen.so: the default build with -DKLARA_MALA_SCREEN=0 in the 4-lane MALA unit (scripts/build_variant.sh)"""
    default = Path(L.LIB_PATH)
    lib = default.with_name("libklara_hip_noscreen.so")
    if lib.exists() and lib.stat().st_mtime >= default.stat().st_mtime:
        return lib
    script = ROOT / "scripts" / "build_variant.sh"
    if not (script.exists() and (ROOT / "build" / "csrc" / "klara_diagt_mala_q4.o").exists() and shutil.which("make") and shutil.which("bash")):
        pytest.skip("no variant build: scripts/build_variant.sh needs the default build's objects and make")
    r = subprocess.run(["bash", str(script), "noscreen", "-DKLARA_MALA_SCREEN=0"], env=dict(os.environ, KLARA_VARIANT_TUS="klara_diagt_mala_q4"),
                       capture_output=True, text=True)
    if r.returncode != 0 or not lib.exists():
        pytest.skip("scripts/build_variant.sh did not produce the variant:\n" + r.stderr[-1500:])
    return lib


def test_screen_compiled_out_gives_the_same_bytes(tmp_path):
    lib = _library_without_the_screen()
    jobs = [(100, 0.9, 81, 32), (100, 0.3, 81, 8), (103, 0.9, 17, 32), (97, 0.02, 17, 8)]
    dest = str(tmp_path / "noscreen.npz")
    code = _CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), jobs=jobs, dest=dest)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KLARA_HIP_LIB=str(lib)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    other = np.load(dest)
    for d, h, n, spl in jobs:
        _, _, out, cnt = _run_engine(d, h, 1, n, spl)
        for k, v in out.items():
            w = other[f"{d}_{h}_{n}_{spl}_{k}"]
            assert v.shape == w.shape and np.ascontiguousarray(v).tobytes() == w.tobytes(), f"d{d} h{h} n{n} {spl} per launch: {k} differs without the screen"
