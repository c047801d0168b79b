"""CPU side of the pooled posterior covariance (KLARA_MON_COVARIANCE, klara_gather_covariance): tests/cov_ref.py's mirror is held to exact rational
arithmetic within the derived bound on every synthetic input tests/test_gpu_cov.py feeds the device (the histories of its small jobs exist on the
device only and are checked there the same way), so that a failure there points at the kernel; the mirror's own fma is exact; the library surface —
header, binding, exports, statuses that need no device, launch planning, the torch.distributed merge, the Julia names — is consistent."""
import ctypes as C
import os
import re
import socket
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import cov_ref as R
import klara_jl_amd as K
import pooled_ref as P
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
OFFSET_SHAPE = (R.CH + 1, 3, 200)            # N, D, saved steps of the offset cases
RANK_SHAPE = (2 * R.CH + 5, 17, 40)          # ... of the shard cases


def check_against_exact(hist, what, splits=None, bounds=None):
    """mirror (and, with bounds, the merged shards) against exact within the bound; prints the figures first.  Returns the mirror's (mean, M)."""
    mean, M = R.mirror(hist, splits)
    ex = R.exact(hist)
    E, Em = R.bound(hist)
    rm, rmean = R.errors(mean, M, ex, E, Em)
    print(f"cov mirror {what}: |M - exact| / bound {rm:.3g}, |mean - exact| / bound {rmean:.3g}")
    assert rm <= 1.0 and rmean <= 1.0, what
    assert np.array_equal(M, M.T)
    if bounds is not None:
        gmean, gM, cnt, _ = R.mirror_ranks(hist, bounds, splits)
        Er, Emr = R.bound_ranks(hist, bounds)
        qm, qmean = R.errors(gmean, gM, ex, Er, Emr)
        print(f"cov mirror {what}, {len(bounds) - 1} shards: |M - exact| / bound {qm:.3g}, |mean - exact| / bound {qmean:.3g}")
        assert qm <= 1.0 and qmean <= 1.0 and cnt == (ex["n"], hist.shape[1]), what
        assert np.array_equal(gM, gM.T)
    return mean, M


# ---------------------------------------------------------------- the mirror
def test_fma_is_exact():
    """cov_ref.fma against a * b + c in rational arithmetic rounded once: random magnitudes, sums that cancel to the last bits of the product (the
    product's rounding error decides), addends far above and far below the product, zeros."""
    rng = np.random.default_rng(1)
    n = 12000
    a = rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n)); b = rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n))
    c = rng.standard_normal(n) * np.exp(rng.uniform(-10, 10, n))
    c[:4000] = -(a[:4000] * b[:4000]) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -52)
    c[4000:6000] = (a[4000:6000] * b[4000:6000]) * 2.0 ** rng.integers(40, 60, 2000)
    c[6000:7000] = (a[6000:7000] * b[6000:7000]) * 2.0 ** -rng.integers(40, 60, 1000).astype(np.float64)
    c[7000:7500] = 0.0; a[7500:8000] = 0.0
    got = R.fma(a, b, c)
    ref = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    assert R.bits_differ(got, ref) == 0
    assert R.bits_differ(got, a * b + c) > 100              # (and it is not the two-rounding form)


def test_slab_is_a_function_of_the_shape_alone():
    assert R.CH == 64 and R.slab(65536, 100) == 64 and R.slab(65536, 256) == 64
    assert R.slab(10 ** 6, 256) == 1024 and R.slab(10 ** 6, 100) == 128         # the workspace cap doubles it
    for N, D in ((65536, 100), (10 ** 6, 256), (10 ** 7, 3)):
        mt = (D + 15) // 16
        assert -(-N // R.slab(N, D)) * (mt * (mt + 1) // 2 * 256 + 16 * mt) * 8 <= R.WORKSPACE_BYTES


@pytest.mark.parametrize("N", R.CHAINS)
def test_mirror_within_bound_every_chain_count(N):
    check_against_exact(R.make_hist(N, 3, 200), f"N={N}", R.splits_of(200))


@pytest.mark.parametrize("D", R.DIMS)
def test_mirror_within_bound_every_width(D):
    check_against_exact(R.make_hist(37, D, 9), f"D={D}", [9])


def test_mirror_is_invariant_to_the_splits():
    hist = R.make_hist(R.N_SPLIT, R.D_SPLIT, 70)
    res = {k: check_against_exact(hist, f"splits {k}", s) for k, s in R.SPLITS70.items()}
    first = res["32+32+6"]
    for k, (mean, M) in res.items():
        assert R.bits_differ(mean, first[0]) == 0 and R.bits_differ(M, first[1]) == 0, k
    m40, M40 = R.mirror(hist, [40, 30])                                          # (a launch of more than 32 saved steps goes in pieces)
    assert R.bits_differ(m40, first[0]) == 0 and R.bits_differ(M40, first[1]) == 0


@pytest.mark.parametrize("offset", P.OFFSETS)
def test_mirror_within_bound_offsets(offset):
    N, D, nc = OFFSET_SHAPE
    hist = R.make_hist(N, D, nc, offset)
    check_against_exact(hist, f"offset={offset:g}sd", R.splits_of(nc))
    E, Em = R.bound(hist)
    print(f"cov bound at {offset:g} sd: M {E.max():.3g}, mean {Em.max():.3g}")      # (M's does not grow with the offset: z does not carry it)


def test_mirror_constant_chains_are_exact():
    hist, v = R.const_hist(R.CH + 6, 5, 9)
    mean, M = R.mirror(hist, [4, 5])
    assert np.all(M == 0.0) and np.array_equal(mean, v)


@pytest.mark.parametrize("nshards", [2, 3])
def test_mirror_shards_within_bound(nshards):
    N, D, nc = RANK_SHAPE
    hist = R.make_hist(N, D, nc, 1e4)
    hist[:, N // 2:] += 3.0 * R.SD                                               # the shards' means differ: the between-rank term is far from zero
    check_against_exact(hist, f"{nshards} shards", R.splits_of(nc), P.shard_bounds(N, nshards))


# ---------------------------------------------------------------- the library surface
def test_header_binding_and_exports_agree(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    assert int(re.search(r"#define KLARA_MON_COVARIANCE (0x[0-9a-f]+)u", hdr).group(1), 16) == L.MON_COVARIANCE == 0x40
    assert int(re.search(r"#define KLARA_COV_MAX_DIMS (\d+)", hdr).group(1)) == L.COV_MAX_DIMS == 256
    assert "#define KLARA_ABI_VERSION 6 " in hdr
    mons = [int(v, 16) for v in re.findall(r"#define KLARA_MON_[A-Z_]+\s+(0x[0-9a-f]+)u", hdr)]
    assert len(mons) == len(set(mons)) == 7 and all(m & (m - 1) == 0 for m in mons)
    for name in ("klara_gather_covariance", "klara_selftest_covariance"):
        assert name in L.EXPORTS and hasattr(klib, name) and re.search(r"klara_status " + name + r"\(", hdr), name
    covh = (ROOT / "klara.jl_amd" / "csrc" / "klara_cov.h").read_text()
    for macro, val in (("KLARA_COV_SLAB_MIN", R.SLAB_MIN), ("KLARA_COV_MAX_COLS", R.MAX_COLS)):
        assert int(re.search(r"#define " + macro + r" (\d+)", covh).group(1)) == val
    assert "((size_t)480 << 20)" in covh and R.WORKSPACE_BYTES == 480 << 20
    for name in ("pooled_cov", "pooled_cor", "allreduce_covariance", "gather_engine_covariance_klara"):
        assert hasattr(K, name), name
    assert hasattr(K.Engine, "pooled_covariance") and hasattr(K.stats, "pooled_cov")


def test_statuses_that_need_no_device(klib):
    assert klib.klara_gather_covariance(None, None, None, None, None, None) == L.ERR_INVALID_ARG
    hist = R.make_hist(3, 3, 4)
    spl, b = np.array([4], np.int64), np.array([0, 3], np.int64)

    def st(N=3, D=3, ncols=4, h=hist, s=spl, ns=1, nr=1, bb=b):
        p = lambda v: None if v is None else v.ctypes.data
        return klib.klara_selftest_covariance(0, N, D, ncols, p(h), ns, p(s), nr, p(bb), None, None, None, None, None)
    for kw in (dict(h=None), dict(s=None), dict(bb=None), dict(N=0), dict(D=0), dict(D=257), dict(ncols=0), dict(ns=0), dict(nr=0),
               dict(s=np.array([33], np.int64), ncols=33), dict(s=np.array([-1, 5], np.int64), ns=2), dict(s=np.array([3], np.int64)),
               dict(bb=np.array([0, 2], np.int64)), dict(bb=np.array([1, 3], np.int64)), dict(bb=np.array([0, 2, 2, 3], np.int64), nr=3),
               dict(bb=np.array([0, 4], np.int64))):
        assert st(**kw) == L.ERR_INVALID_ARG, kw


def _plan(klib, runs, **kw):
    d = L.KlaraDesc()
    d.struct_size = C.sizeof(L.KlaraDesc); d.abi_version = L.KLARA_ABI_VERSION
    d.sampler, d.target, d.nchains, d.ndims = L.SAMPLER_MALA, L.TARGET_GAUSS_DIAG, 256, 100
    d.driftstep, d.period, d.thinning, d.nsteps = 0.5, 100, 1, sum(runs)
    for key, v in kw.items():
        setattr(d, key, v)
    cap = int(sum(runs)) + 8
    k = np.zeros(cap, np.int64); col = np.zeros(cap, np.int64); ph = np.zeros(cap, np.int32); fl = np.zeros(cap, np.int32)
    n = C.c_int64(0)
    st = klib.klara_selftest_plan(C.byref(d), len(runs), np.asarray(runs, np.int64).ctypes.data, cap, k.ctypes.data, col.ctypes.data, ph.ctypes.data,
                                  fl.ctypes.data, C.byref(n))
    assert st == L.OK, st
    n = int(n.value)
    return [a[:n].tolist() for a in (k, col, ph, fl)]


def test_launch_plan_with_the_bit_is_the_plan_of_a_streaming_consumer(klib):
    """KLARA_MON_COVARIANCE plans its launches exactly as acov_maxlag > 0 does: the 32-column ring of its own ends launches where it would wrap
    (a job with neither is not cut there), a ring or a full history the caller asked for is kept."""
    for kw in (dict(), dict(burnin=10, thinning=3), dict(steps_per_launch=48), dict(burnin=7, steps_per_launch=20, thinning=2),
               dict(hist_ring_cols=8), dict(hist_ring_cols=40, steps_per_launch=64)):
        for base in (0, L.MON_HISTORY, L.MON_SUMMARIES | L.MON_ACCEPT):
            runs = [150, 37, 13]
            cov = _plan(klib, runs, monitor=base | L.MON_COVARIANCE, **kw)
            acov = _plan(klib, runs, monitor=base, acov_maxlag=5, **kw)
            assert cov == acov, (kw, base)
    plain = _plan(klib, [200], monitor=L.MON_SUMMARIES, steps_per_launch=48)
    cov = _plan(klib, [200], monitor=L.MON_SUMMARIES | L.MON_COVARIANCE, steps_per_launch=48)
    assert plain[0] != cov[0] and max(cov[0]) <= 32 and max(plain[0]) == 48
    full = _plan(klib, [200], monitor=L.MON_HISTORY | L.MON_COVARIANCE, steps_per_launch=48)
    assert full[0] == plain[0]                                                   # a full history has no ring to wrap


# ---------------------------------------------------------------- torch.distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import sys
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    import torch.distributed as dist
    import cov_ref as R
    import klara_jl_amd as K
    import pooled_ref as P
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    N, D, nc = RANK_SHAPE
    hist = R.make_hist(N, D, nc, 242.0)
    b = P.shard_bounds(N, world)
    mine = np.ascontiguousarray(hist[:, b[rank]:b[rank + 1]])
    mean, M = R.mirror(mine)                                                     # what Engine.pooled_covariance() hands a rank
    out = K.allreduce_covariance({"mean": mean, "m2": M, "nsamples": mine.shape[0] * mine.shape[1], "nchains": mine.shape[1]})
    q.put((rank, out["mean"], out["m2"], out["nsamples"], out["nchains"], out["cov"]))
    dist.destroy_process_group()


def test_allreduce_covariance_world2_is_the_single_rank_result_within_bound():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60); assert p.exitcode == 0
    N, D, nc = RANK_SHAPE
    hist = R.make_hist(N, D, nc, 242.0)
    one_mean, one_M = R.mirror(hist)
    wm, wM, cnt, _ = R.mirror_ranks(hist, P.shard_bounds(N, 2))
    E1, Em1 = R.bound(hist)
    E2, Em2 = R.bound_ranks(hist, P.shard_bounds(N, 2))
    ex = R.exact(hist)
    for _, mean, M, ns, nch, cov in res:
        assert (ns, nch) == (nc * N, N) and np.array_equal(M, M.T)
        assert R.bits_differ(mean, wm) == 0 and R.bits_differ(M, wM) == 0        # the same three sums, in rank order
        assert np.all(np.abs(M - one_M) <= E1 + E2) and np.all(np.abs(mean - one_mean) <= Em1 + Em2)
        rm, rmean = R.errors(mean, M, ex, E2, Em2)
        print(f"allreduce_covariance world 2: |M - exact| / bound {rm:.3g}, |mean - exact| / bound {rmean:.3g}")
        assert rm <= 1.0 and rmean <= 1.0
        assert np.array_equal(cov, M / (ns - 1))
    # ... and the literal NumPy form agrees to rounding
    lit = K.stats.pooled_cov(np.transpose(hist, (1, 2, 0)))
    assert np.allclose(lit, one_M / (nc * N - 1), rtol=1e-10, atol=1e-12)


def test_allreduce_covariance_single_process():
    hist = R.make_hist(5, 4, 6)
    mean, M = R.mirror(hist)
    out = K.allreduce_covariance({"mean": mean, "m2": M, "nsamples": 30, "nchains": 5})
    assert out["nsamples"] == 30 and out["nchains"] == 5 and np.array_equal(out["cov"], out["m2"] / 29)
    assert np.allclose(out["m2"], M, rtol=1e-14, atol=1e-14) and np.allclose(out["mean"], mean, rtol=1e-15)


# ---------------------------------------------------------------- Julia
def test_julia_names_are_present_and_do_not_collide():
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    txt = (ROOT / "tests" / "golden" / "klara_exports.txt").read_text().splitlines()
    klara = {t for t in txt if t and not t.startswith("[")}
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jl, re.M).group(1)
    exported = {t for t in re.split(r"[,\s]+", export) if t}
    for name in ("pooledcovariance", "gather_covariance"):
        assert name in exported and name not in klara and re.search(r"^function " + name + r"\(job::HIPMCJob", jl, re.M), name
    assert "covariance!" in klara and "covariance!" not in exported
    assert re.search(r"const MON_COVARIANCE = 0x40\b", jl) and "covariance::Bool=false" in jl and "mon |= MON_COVARIANCE" in jl
    assert jl.count("(:klara_gather_covariance, lib)") == 2
    md = (ROOT / "INTEGRATION.md").read_text()
    assert "pooledcovariance(job)" in md and "covariance=true" in md
