"""CPU side of the Gelman–Rubin diagnostic (klara_gather_rhat): tests/rhat_ref.py's mirror is held to exact rational arithmetic within the derived bound on
every shape tests/test_gpu_rhat.py runs on the device — which is where those inputs are shown to be admissible (every bound under pooled_ref.CAP) —, the
literal NumPy form klara_jl_amd.stats.rhat to the same exact values, the split form to its reason for existing, and the new surface (header, binding,
Julia, argument checks, the torch.distributed merge) to what it declares."""
import ctypes as C
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch.multiprocessing as mp

import klara_jl_amd as K
import pooled_ref as P
import rhat_ref as R
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------- the shapes and inputs shared with the GPU test
def sums_case(N, D, nsaved, offset):
    """(inp, exact) of the unsplit path: pooled_ref.make_inputs at the first admissible seed for every rank count of rhat_ref.rank_bounds(N)"""
    cols = R.cols_for(D)

    def make(seed):
        inp = P.make_inputs(N, D, nsaved, offset, seed)
        return inp, R.exact(inp=inp, cols=cols)
    inp, ex, _ = R.first_admissible(make, R.rank_bounds(N).keys())
    return inp, ex


def hist_case(N, D, ncols, offset, still="some"):
    cols = R.cols_for(D)

    def make(seed):
        h = R.make_hist(N, D, ncols, offset, seed, still)
        return h, R.exact(hist=h, cols=cols)
    h, ex, _ = R.first_admissible(make, R.rank_bounds(N).keys())
    return h, ex


def sums_shapes(N):
    return [(D, ns, off) for ns in R.NSAVED for off in R.OFFSETS for D in R.dims_for(N, ns)]


def hist_shapes(N):
    return [(D, nc, off) for nc in R.NCOLS for off in R.OFFSETS for D in R.dims_for(N, nc)]


def sums_of_hist(hist):
    """the running sums a job that saved the history `hist` (on GRID: every sum is exact) would hold, as pooled_ref inputs"""
    ncols, N, D = hist.shape
    return {"sum": hist.sum(axis=0), "sumsq": (hist * hist).sum(axis=0), "X": hist[-1].copy(), "held": np.zeros(N, dtype=np.int64),
            "naccept": np.zeros(N, dtype=np.uint64), "nsaved": ncols}


def selftest(inp=None, hist=None, bounds=None, status=False, **over):
    """klara_selftest_rhat: dict of "out", "ranks", "split", "split_ranks" -> dict as Engine.rhat returns (status=True: the status alone); `over` replaces
    single arguments for the argument checks"""
    klib = L.load()
    src = inp["sum"] if inp is not None else hist[0]
    a = {"N": src.shape[0], "D": src.shape[1], "nsaved": inp["nsaved"] if inp is not None else 0, "ncols": hist.shape[0] if hist is not None else 0,
         "sum": None, "sumsq": None, "X": None, "held": None, "hist": hist}
    if inp is not None:
        a.update({k: inp[k] for k in ("sum", "sumsq", "X", "held")})
    a.update(over)
    b = np.asarray([0, a["N"]] if bounds is None else bounds, dtype=np.int64)
    D = a["D"] if 1 <= a["D"] <= 1024 else 1
    outs = [np.full(4 * D, -12345.5) for _ in range(4)]
    cnt = np.zeros(8, dtype=np.uint64)
    ptr = lambda v: None if v is None else v.ctypes.data
    st = klib.klara_selftest_rhat(0, a["N"], a["D"], a["nsaved"], ptr(a["sum"]), ptr(a["sumsq"]), ptr(a["X"]), ptr(a["held"]), a["ncols"], ptr(a["hist"]),
                                  b.size - 1, ptr(b), *[ptr(o) for o in outs], ptr(cnt))
    if status:
        return st
    L.check(st, "klara_selftest_rhat")
    res = {}
    for i, name in enumerate(("out", "ranks", "split", "split_ranks")):
        o = outs[i]
        res[name] = {"rhat": o[:D], "mean": o[D:2 * D], "wsum": o[2 * D:3 * D], "bsum": o[3 * D:], "nchains": int(cnt[2 * i]), "nper": int(cnt[2 * i + 1])}
    return res


# ---------------------------------------------------------------- mirror against exact, on every shape of the GPU test
@pytest.mark.parametrize("N", R.NS)
def test_mirror_of_the_sums_path_is_within_the_bound_of_exact(N):
    worst = 0.0
    for D, ns, off in sums_shapes(N):
        inp, ex = sums_case(N, D, ns, off)
        what = f"sums N={N} D={D} nsaved={ns} offset={off}"
        worst = max(worst, R.check(R.mirror(inp=inp), None, ex, 1, what))
        for r, b in R.rank_bounds(N).items():
            worst = max(worst, R.check(R.mirror_ranks(b, inp=inp), None, ex, r, what + f" ranks={r}"))
    print(f"rhat mirror, sums, N={N}: largest error / bound {worst:.3g}")


@pytest.mark.parametrize("N", R.NS)
def test_mirror_of_the_split_path_is_within_the_bound_of_exact(N):
    worst = 0.0
    for D, nc, off in hist_shapes(N):
        h, ex = hist_case(N, D, nc, off)
        what = f"split N={N} D={D} ncols={nc} offset={off}"
        worst = max(worst, R.check(R.mirror(hist=h), None, ex, 1, what))
        for r, b in R.rank_bounds(N).items():
            worst = max(worst, R.check(R.mirror_ranks(b, hist=h), None, ex, r, what + f" ranks={r}"))
    print(f"rhat mirror, split, N={N}: largest error / bound {worst:.3g}")


def test_split_sums_are_exact_on_the_grid():
    """What bound() assumes of the split kernel's inputs: x - x_first, its sum and the sum of its squares round nowhere on make_hist's grid, at every offset"""
    for off in R.OFFSETS:
        h = R.make_hist(257, 3, 200, off)
        n = 100
        for first in (0, 100):
            z = h[first:first + n] - h[first]
            s = np.zeros(z.shape[1:]); q = np.zeros(z.shape[1:])
            for t in range(n):
                s = s + z[t]; q = q + z[t] * z[t]
            zi = np.rint(z / R.GRID).astype(np.int64)
            assert np.array_equal(zi * R.GRID, z)
            assert np.array_equal(s, zi.sum(axis=0) * R.GRID) and np.array_equal(q, (zi * zi).sum(axis=0) * R.GRID ** 2)


def test_still_chains_give_zero_inf_and_nan_exactly():
    """Chains that never moved: wsum is exactly 0; R-hat is +inf where their states differ and NaN where all stand at one state — in the mirror as in exact"""
    for off in R.OFFSETS:
        for same in (False, True):
            inp = R.still_inputs(257, 3, 200, off, same=same)
            ex = R.exact(inp=inp)
            m = R.mirror(inp=inp)
            assert np.all(ex["wsum_zero"]) and np.all(ex["bsum_zero"] == same) and np.all(m["wsum"] == 0.0)
            assert np.all(np.isnan(m["rhat"])) if same else np.all(m["rhat"] == np.inf)
            R.check(m, None, ex, 1, f"still sums same={same}")
            R.check(R.mirror_ranks([0, 1, 100, 257], inp=inp), None, ex, 3, f"still sums ranks same={same}")
            h = R.make_hist(257, 3, 200, off, still="same" if same else "all")
            ex = R.exact(hist=h)
            m = R.mirror(hist=h)
            assert np.all(ex["wsum_zero"]) and np.all(ex["bsum_zero"] == same)
            assert np.all(np.isnan(m["rhat"])) if same else np.all(m["rhat"] == np.inf)
            R.check(m, None, ex, 1, f"still hist same={same}")
            R.check(R.mirror_ranks([0, 1, 100, 257], hist=h), None, ex, 3, f"still hist ranks same={same}")


# ---------------------------------------------------------------- the literal NumPy form
@pytest.mark.parametrize("N,D,ncols", [(2, 1, 4), (3, 3, 7), (257, 3, 200), (1025, 3, 5)])
def test_stats_rhat_agrees_with_exact(N, D, ncols):
    """klara_jl_amd.stats.rhat — two passes in NumPy's own order — against exact within the device's bound, at offsets 0 and 242 sd.  (At 1e6 sd NumPy's
    chain means round at n u |mean|, which is no part of the device's bound: the statistical reference is not asked to be the accurate one.)"""
    for off in (0.0, 242.0):
        h, ex = hist_case(N, D, ncols, off)
        v = h.transpose(1, 0, 2)                                             # (chains, samples, D)
        got = K.stats.rhat(v, split=True)
        _, _, rel = R.bound(ex)
        for i, j in enumerate(ex["cols"]):
            want = np.sqrt(ex["rhat2"][i])
            assert (np.isnan(want) and np.isnan(got[j])) or abs(got[j] - want) <= rel[i] * want, (off, j, got[j], want, rel[i])
        inp = sums_of_hist(h)
        ex = R.exact(inp=inp, cols=R.cols_for(D))
        got = K.stats.rhat(v)
        _, _, rel = R.bound(ex)
        for i, j in enumerate(ex["cols"]):
            want = np.sqrt(ex["rhat2"][i])
            assert (np.isnan(want) and np.isnan(got[j])) or abs(got[j] - want) <= rel[i] * want, (off, j, got[j], want, rel[i])
    assert np.all(np.isnan(K.stats.rhat(np.zeros((1, 10, 2))))) and np.all(np.isnan(K.stats.rhat(np.zeros((4, 3, 2)), split=True)))


def test_split_rhat_sees_a_common_trend_that_rhat_does_not():
    """Every chain carries the same linear trend: the chains agree with each other at every step, so the unsplit R-hat stays near 1, while each chain's two
    halves disagree — the exact split R-hat exceeds the exact unsplit one.  This is why the split form exists."""
    rng = np.random.default_rng(7)
    N, D, n = 64, 2, 100
    t = np.arange(n)[:, None, None]
    h = np.rint((R.SD * rng.standard_normal((n, N, D)) + 0.125 * t) / R.GRID) * R.GRID
    split = R.exact(hist=h)
    whole = R.exact(inp=sums_of_hist(h))
    assert np.all(split["rhat2"] > whole["rhat2"]) and np.all(np.sqrt(split["rhat2"]) > 1.5) and np.all(np.sqrt(whole["rhat2"]) < 1.05), (split["rhat2"], whole["rhat2"])
    v = h.transpose(1, 0, 2)
    assert np.all(K.stats.rhat(v, split=True) > K.stats.rhat(v))


# ---------------------------------------------------------------- the surface
def test_header_and_binding_declare_the_new_symbols(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    for name in ("klara_gather_rhat", "klara_selftest_rhat"):
        assert name in L.EXPORTS and hasattr(klib, name) and re.search(r"klara_status " + name + r"\(", hdr), name
    assert klib.klara_abi_version() == 6
    assert klib.klara_gather_rhat(None, None, 0, None, None, None, None, None, None) == L.ERR_INVALID_ARG


def test_julia_exports_and_defines_rhat_and_gather_rhat():
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    exported = set(re.split(r"[,\s]+", re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jl, re.M).group(1)))
    assert {"rhat", "gather_rhat"} <= exported
    assert re.search(r"^function rhat\(job::HIPMCJob; split::Bool=false\)", jl, re.M)
    assert re.search(r"^function gather_rhat\(job::HIPMCJob, comm::HIPComm; split::Bool=false\)", jl, re.M)
    assert jl.count("(:klara_gather_rhat, lib)") == 2
    klara = (ROOT / "tests" / "golden" / "klara_exports.txt").read_text().split()
    assert "rhat" not in klara and "gather_rhat" not in klara


def test_selftest_refuses_bad_arguments_before_any_launch():
    """No device here: every refusal below has to come before the first HIP call"""
    inp = P.make_inputs(5, 3, 4)
    h = R.make_hist(5, 3, 4)
    bad = [dict(inp=None, hist=None, N=5, D=3), dict(inp=inp, N=0), dict(inp=inp, D=0), dict(inp=inp, D=1025), dict(inp=inp, nsaved=0),
           dict(inp=inp, sumsq=None), dict(inp=inp, held=None), dict(hist=h, ncols=1), dict(inp=inp, bounds=[0, 3, 3, 5]), dict(inp=inp, bounds=[1, 5]),
           dict(inp=inp, bounds=[0, 4]), dict(hist=h, bounds=[0, 6])]
    for kw in bad:
        kw = dict(kw)
        i, hh = kw.pop("inp", None), kw.pop("hist", None)
        if i is None and hh is None:
            klib = L.load()
            b = np.array([0, 5], dtype=np.int64)
            assert klib.klara_selftest_rhat(0, 5, 3, 4, None, None, None, None, 4, None, 1, b.ctypes.data, None, None, None, None, None) == L.ERR_INVALID_ARG
            continue
        assert selftest(inp=i, hist=hh, status=True, **kw) == L.ERR_INVALID_ARG, kw


# ---------------------------------------------------------------- the merge through torch.distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import sys
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    import torch.distributed as dist
    import klara_jl_amd as K
    import pooled_ref as P
    import rhat_ref as R
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    inp = P.make_inputs(301, 3, 50, 242.0)
    b = [0, 100, 301]
    out = K.allreduce_rhat(R.mirror(inp=P.slice_inputs(inp, b[rank], b[rank + 1])))
    uneven = R.mirror(inp=P.slice_inputs(inp, b[rank], b[rank + 1]))
    uneven["nper"] += rank                                                   # the ranks disagree on the saved steps: every rank has to refuse
    try:
        K.allreduce_rhat(uneven)
        refused = False
    except ValueError:
        refused = True
    q.put((rank, {k: np.asarray(v) for k, v in out.items()}, refused))
    dist.destroy_process_group()


def test_allreduce_rhat_world2_reproduces_mirror_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = R.mirror_ranks([0, 100, 301], inp=P.make_inputs(301, 3, 50, 242.0))
    for _, out, refused in res:
        assert refused
        for k in ("rhat", "mean", "wsum", "bsum"):
            assert np.array_equal(out[k], want[k]), k
        assert int(out["nchains"]) == 301 and int(out["nper"]) == 50
    one = K.allreduce_rhat(R.mirror(inp=P.make_inputs(301, 3, 50, 242.0)))   # no process group: this rank alone
    assert np.array_equal(one["rhat"], R.mirror_ranks([0, 301], inp=P.make_inputs(301, 3, 50, 242.0))["rhat"])
