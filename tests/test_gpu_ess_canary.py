"""The pooled effective sample size between canaries (KLARA_DEBUG_CANARY=1: 4 KiB of a signalling-NaN pattern before and after every device array,
tests/test_gpu_canary.py): the self-test path on the shapes whose indexing is the least regular — a clipped window, a window of 128 lags with its
checkpoints, the split form's two states, D = 1024 on three chains, more unit-series than lanes — and the job path; klara_selftest_ess returns
KLARA_ERR_HIP and Engine.close raises when a kernel stored outside one of their arrays, and a stray load would bring a NaN into the compared bits."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_required")]
ROOT = Path(__file__).resolve().parent.parent

_PROBE = r'''
import ctypes as C, sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import numpy as np
import klara_jl_amd as K
from klara_jl_amd import _lib as L
import ess_ref as E
lib = L.load()
na, nc = C.c_int64(0), C.c_int64(0)
L.check(lib.klara_selftest_canary(0, C.byref(na), C.byref(nc)), "klara_selftest_canary")       # (KLARA_ERR_STATE unless the canaries are on)
for N, D, ml, ncols, kind, bounds in ((3, 3, 33, 20, "ragged", [0, 1, 3]), (5, 4, 127, 200, "ragged", [0, 2, 5]), (3, 1024, 8, 9, "one", [0, 1, 2, 3]),
                                      (1400, 100, 7, 9, "32s", [0, 1, 1400])):
    hist = E.make_hist(N, D, ncols, 1e4, 0)
    st, res = E.selftest(lib, hist, ml, E.launch_splits(ncols, kind), bounds)
    assert st == 0, (N, D, ml, ncols, st)
    for split, path in ((False, "streamed"), (False, "history"), (True, "split")):
        mir = E.mirror(hist, ml, split)
        for k in ("csum", "wsum", "mean", "bsum", "rho", "tau", "ess"):
            assert np.array_equal(res[(path, False)][k], mir[k], equal_nan=True), (N, D, path, k)
e = K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(7), nchains=301, nsteps=70, driftstep=0.5, acov_maxlag=40,
             monitor=L.MON_SUMMARIES | L.MON_ACCEPT | L.MON_HISTORY, steps_per_launch=32)
e.init_state_normal(); e.run(70)
a, b, c = e.pooled_ess("streamed"), e.pooled_ess("history", 127), e.pooled_ess("split", 33)
assert a["lags"] == 40 and b["lags"] == 69 and c["lags"] == 33 and np.all(np.isfinite(a["ess"]))
L.check(lib.klara_selftest_canary(0, C.byref(na), C.byref(nc)), "klara_selftest_canary")
assert nc.value == 0, nc.value
e.close()                                                     # raises when a canary of the handle's arrays was damaged
print("INTACT")
'''


def test_ess_kernels_between_canaries():
    env = dict(os.environ, KLARA_DEBUG_CANARY="1")
    r = subprocess.run([sys.executable, "-c", _PROBE.replace("ROOT", str(ROOT))], capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("INTACT"), r.stdout
