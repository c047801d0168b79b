"""CPU side of the pooled marginal histograms (klara_desc.marg_nbins, klara_gather_histogram, klara_histogram_quantiles): the library surface — header,
binding, Julia stub, exports, every status that needs no device, launch planning — is consistent; ranks whose bins differ are found by the agreement step klara_gather_histogram runs, over simulated ranks; the host-only quantile call equals its NumPy
restatement bit for bit and lies within a derived bound of the exact order statistic; the torch.distributed merge is the unsharded table; and the
quantile code runs clean under the host sanitizers as a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import socket
import subprocess
from pathlib import Path

import numpy as np
import pytest

import klara_jl_amd as K
import marg_ref as R
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
NEW_FIELDS = [("marg_lo", "const double*"), ("marg_hi", "const double*"), ("marg_nbins", "int64_t")]
NEW_FUNCS = ["klara_gather_histogram", "klara_histogram_quantiles", "klara_selftest_marginals", "klara_selftest_histogram_ranks"]


# ---------------------------------------------------------------- the library surface
def test_header_binding_julia_and_exports_agree(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    body = re.search(r"typedef struct klara_desc \{(.*?)\} klara_desc;", hdr, re.S).group(1)
    cfields = re.findall(r"^\s{4}((?:const\s+)?\w+\*?)\s+(\w+);", body, re.M)
    names = [n for _, n in cfields]
    i = names.index("ram_gamma")
    assert [(n, t.replace("const ", "const ").replace("  ", " ")) for t, n in cfields[i + 1:i + 4]] == NEW_FIELDS
    assert names[i + 4] == "seed" and names[-1] == "stream"
    pyf = [n for n, _ in L.KlaraDesc._fields_]
    assert pyf == names                                                          # the same order in the binding ...
    types = dict(L.KlaraDesc._fields_)
    assert types["marg_lo"] is types["marg_hi"] is types["ram_S0"] and types["marg_nbins"] is C.c_int64
    # ... no implicit padding: the three fields are 8 bytes each and the struct grew by exactly 24 over the fields before them
    assert L.KlaraDesc.marg_lo.offset == L.KlaraDesc.ram_gamma.offset + 8 and L.KlaraDesc.marg_nbins.offset == L.KlaraDesc.marg_lo.offset + 16
    assert L.KlaraDesc.seed.offset == L.KlaraDesc.marg_nbins.offset + 8
    assert sum(C.sizeof(t) for _, t in L.KlaraDesc._fields_) == C.sizeof(L.KlaraDesc)
    jstruct = re.search(r"struct KlaraDesc\n(.*?)\nend", jl, re.S).group(1)
    jfields = re.findall(r"(\w+)::([\w{}]+)", jstruct)
    assert [n for n, _ in jfields] == names
    jt = dict(jfields)
    assert jt["marg_lo"] == jt["marg_hi"] == "Ptr{Float64}" and jt["marg_nbins"] == "Int64"
    call = re.search(r"KlaraDesc\(UInt32\(sizeof\(KlaraDesc\)\), KLARA_ABI_VERSION,(.*?)\)\nend", jl, re.S).group(1)
    assert [t for t in re.split(r"[,\s]+", call) if t] == names[2:]              # klara_desc(; ...) passes them in struct order
    assert "marg_lo=Ptr{Float64}(C_NULL), marg_hi=Ptr{Float64}(C_NULL), marg_nbins=0" in jl
    # still 7 monitor bits, still ABI version 6: the feature is switched on by descriptor fields
    mons = [int(v, 16) for v in re.findall(r"#define KLARA_MON_[A-Z_]+\s+(0x[0-9a-f]+)u", hdr)]
    assert len(mons) == len(set(mons)) == 7
    assert "#define KLARA_ABI_VERSION 6 " in hdr and L.KLARA_ABI_VERSION == 6 and int(klib.klara_abi_version()) == 6
    assert "const KLARA_ABI_VERSION = UInt32(6)" in jl
    assert int(re.search(r"#define KLARA_MARG_MAX_BINS (\d+)", hdr).group(1)) == L.MARG_MAX_BINS == 1024
    assert re.search(r"const MARG_MAX_BINS = 1024\b", jl)
    for name in NEW_FUNCS:
        assert name in L.EXPORTS and hasattr(klib, name) and re.search(r"klara_status " + name + r"\(", hdr), name
    assert jl.count("(:klara_gather_histogram, lib)") == 1 and jl.count("(:klara_histogram_quantiles, lib)") == 1
    for name in ("Marginals", "pooled_hist", "pooled_quantiles", "allreduce_histogram", "histogram_quantiles"):
        assert hasattr(K, name), name
    assert hasattr(K.Engine, "pooled_histogram") and hasattr(K.stats, "pooled_hist") and hasattr(K.stats, "hist_quantiles")


def test_julia_names_are_present_and_do_not_collide():
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    txt = (ROOT / "tests" / "golden" / "klara_exports.txt").read_text().splitlines()
    klara = {t for t in txt if t and not t.startswith("[")}
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jl, re.M).group(1)
    exported = {t for t in re.split(r"[,\s]+", export) if t}
    for name in ("pooledhistogram", "pooledquantiles", "gather_histogram"):
        assert name in exported and name not in klara and re.search(r"^(function )?" + name + r"\(job::HIPMCJob", jl, re.M), name
    assert "marginals=nothing" in jl and "kw[:marg_nbins] = Int64(nb)" in jl


def test_geometry_is_a_function_of_the_shape_alone():
    """klara_marg.h: slab, dimensions per workgroup and LDS bytes from (N, D, nbins); a workgroup's 32-bit counter cannot overflow in one launch"""
    assert (R.THREADS, R.MAX_DB, R.SLAB_UNIT, R.MAX_COLS) == (256, 64, 256, 32)
    assert R.slab(1) == R.slab(64) == R.slab(254) == 256 and R.slab(255) == 512 and R.slab(1024) == 1280
    assert R.dims_per_block(100, 64) == 64 and R.dims_per_block(3, 64) == 3 and R.dims_per_block(100, 1024) == 14 and R.dims_per_block(1024, 237) == 64
    for nbins in range(1, L.MARG_MAX_BINS + 1):
        db = R.dims_per_block(1024, nbins)
        assert db >= 1 and 4 * db * ((nbins + 2) | 1) <= R.LDS_BYTES and R.slab(nbins) * R.MAX_COLS < 2 ** 32
        assert R.THREADS // db >= 4


def _desc(**kw):
    d = L.KlaraDesc()
    d.struct_size = C.sizeof(L.KlaraDesc); d.abi_version = L.KLARA_ABI_VERSION
    d.sampler, d.target, d.nchains, d.ndims = L.SAMPLER_MALA, L.TARGET_GAUSS_DIAG, 256, 100
    d.driftstep, d.period, d.thinning, d.nsteps = 0.5, 100, 1, 200
    d.device = 1 << 20                                                           # (no such device: a descriptor that passes validation ends at KLARA_ERR_HIP)
    for key, v in kw.items():
        setattr(d, key, v)
    return d


def test_create_refuses_every_bad_argument_before_any_device_call(klib):
    D = 100
    lo = np.full(D, -1.0); hi = np.full(D, 1.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def create(nbins, lo_, hi_):
        d = _desc(marg_nbins=nbins)
        if lo_ is not None:
            d.marg_lo = dp(lo_)
        if hi_ is not None:
            d.marg_hi = dp(hi_)
        h = C.c_void_p()
        st = klib.klara_create(C.byref(d), C.byref(h))
        assert not h.value
        return st
    bad = lambda i, v, a: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    cases = [(-1, lo, hi), (1025, lo, hi), (8, None, hi), (8, lo, None), (8, None, None), (0, lo, None), (0, None, hi), (0, lo, hi),
             (8, bad(3, np.nan, lo), hi), (8, bad(99, -np.inf, lo), hi), (8, lo, bad(0, np.inf, hi)), (8, lo, bad(7, np.nan, hi)),
             (8, bad(5, 1.0, lo), hi), (8, bad(5, 2.0, lo), hi)]
    for nbins, a, b in cases:
        assert create(nbins, a, b) == L.ERR_INVALID_ARG, (nbins, None if a is None else a[:8], None if b is None else b[:8])
    for nbins in (1, 8, 1024):                                                   # valid: validation passes and the missing device is what stops it
        assert create(nbins, lo, hi) == L.ERR_HIP
    assert create(0, None, None) == L.ERR_HIP
    assert klib.klara_gather_histogram(None, None, None, None, None) == L.ERR_INVALID_ARG


def test_selftest_refuses_every_bad_argument_before_any_device_call():
    hist = np.zeros((4, 3, 2))
    lo, hi = np.array([-1.0, 0.0]), np.array([1.0, 2.0])
    st = lambda h=hist, s=(4,), nb=8, a=lo, b=hi: R.selftest(h, s, nb, a, b, status=True)
    for kw in (dict(s=(5,)), dict(s=(2, -1, 3)), dict(s=(3,)), dict(nb=0), dict(nb=1025), dict(a=np.array([-1.0, np.nan])), dict(b=np.array([np.inf, 2.0])),
               dict(a=np.array([1.0, 0.0])), dict(a=np.array([2.0, 0.0])), dict(h=np.zeros((33, 1, 2)), s=(33,))):
        assert st(**kw) == L.ERR_INVALID_ARG, kw
    klib = L.load()
    spl = np.array([4], np.int64); cnt = np.zeros((2, 10), np.uint64)
    p = lambda v: None if v is None else v.ctypes.data
    for N, D, nc, h, s, a, b, c in ((0, 2, 4, hist, spl, lo, hi, cnt), (3, 0, 4, hist, spl, lo, hi, cnt), (3, 1025, 4, hist, spl, lo, hi, cnt),
                                    (3, 2, 0, hist, spl, lo, hi, cnt), (3, 2, 4, None, spl, lo, hi, cnt), (3, 2, 4, hist, None, lo, hi, cnt),
                                    (3, 2, 4, hist, spl, None, hi, cnt), (3, 2, 4, hist, spl, lo, None, cnt), (3, 2, 4, hist, spl, lo, hi, None)):
        assert klib.klara_selftest_marginals(1 << 20, N, D, nc, p(h), 1, p(s), 8, p(a), p(b), p(c)) == L.ERR_INVALID_ARG, (N, D, nc)
    assert klib.klara_selftest_marginals(1 << 20, 3, 2, 4, p(hist), 0, p(spl), 8, p(lo), p(hi), p(cnt)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_marginals(1 << 20, 3, 2, 4, p(hist), 1, p(spl), 8, p(lo), p(hi), p(cnt)) == L.ERR_HIP       # valid: stopped by the device only


def _ranks(klib, nbins, lo, hi):
    nbins = np.asarray(nbins, np.int64); lo = np.ascontiguousarray(lo, np.float64); hi = np.ascontiguousarray(hi, np.float64)
    return klib.klara_selftest_histogram_ranks(nbins.size, lo.shape[1], nbins.ctypes.data, lo.ctypes.data, hi.ctypes.data)


def test_ranks_whose_bins_differ_all_get_err_state(klib):
    """klara_gather_histogram's agreement step over simulated ranks — the words every rank stages, the maximum all-reduce replaced by a host maximum, the
    verdict all ranks reach on the same reduced words: identical ranks go on; a differing nbins, one differing bit of one bound on one rank, a sign of zero,
    bounds swapped between dimensions all end in KLARA_ERR_STATE, whichever rank is the odd one"""
    D = 5
    lo = np.tile(np.array([-2.0, -1.0, 0.0, 1e6, -3.5]), (3, 1)); hi = np.tile(np.array([2.0, 1.5, 0.25, 1e6 + 1e-3, 3.5]), (3, 1))
    for world in (1, 2, 3):
        assert _ranks(klib, [64] * world, lo[:world], hi[:world]) == L.OK
    for odd in range(3):
        nb = [64, 64, 64]; nb[odd] = 65
        assert _ranks(klib, nb, lo, hi) == L.ERR_STATE
        nb[odd] = 1
        assert _ranks(klib, nb, lo, hi) == L.ERR_STATE
        for arr in (lo, hi):
            for d in range(D):
                for step in (np.inf, -np.inf):
                    a = arr.copy(); a[odd, d] = np.nextafter(a[odd, d], step)    # one bit of one bound on one rank
                    args = (a, hi) if arr is lo else (lo, a)
                    assert _ranks(klib, [64, 64, 64], *args) == L.ERR_STATE, (odd, d, step)
        a = lo.copy(); a[odd, 2] = -0.0
        assert _ranks(klib, [64, 64, 64], a, hi) == L.ERR_STATE                  # bit patterns, not values
        a = lo.copy(); a[odd, [0, 1]] = a[odd, [1, 0]]
        assert _ranks(klib, [64, 64, 64], a, hi) == L.ERR_STATE
    assert _ranks(klib, [64, 65], lo[:2], hi[:2]) == L.ERR_STATE and _ranks(klib, [1024, 1], lo[:2], hi[:2]) == L.ERR_STATE
    nb = np.array([8], np.int64)
    assert klib.klara_selftest_histogram_ranks(0, D, nb.ctypes.data, lo.ctypes.data, hi.ctypes.data) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_histogram_ranks(1, 0, nb.ctypes.data, lo.ctypes.data, hi.ctypes.data) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_histogram_ranks(1, 1025, nb.ctypes.data, lo.ctypes.data, hi.ctypes.data) == L.ERR_INVALID_ARG
    for i in range(3):
        a = [nb.ctypes.data, lo.ctypes.data, hi.ctypes.data]; a[i] = None
        assert klib.klara_selftest_histogram_ranks(1, D, *a) == L.ERR_INVALID_ARG


def _plan(klib, runs, marginals=False, **kw):
    d = _desc(nsteps=sum(runs), device=0, **kw)
    keep = (np.full(100, -3.0), np.full(100, 3.0))
    if marginals:
        d.marg_lo = keep[0].ctypes.data_as(C.POINTER(C.c_double)); d.marg_hi = keep[1].ctypes.data_as(C.POINTER(C.c_double)); d.marg_nbins = 8
    cap = int(sum(runs)) + 8
    k = np.zeros(cap, np.int64); col = np.zeros(cap, np.int64); ph = np.zeros(cap, np.int32); fl = np.zeros(cap, np.int32)
    n = C.c_int64(0)
    st = klib.klara_selftest_plan(C.byref(d), len(runs), np.asarray(runs, np.int64).ctypes.data, cap, k.ctypes.data, col.ctypes.data, ph.ctypes.data,
                                  fl.ctypes.data, C.byref(n))
    assert st == L.OK, st
    n = int(n.value)
    return [a[:n].tolist() for a in (k, col, ph, fl)]


def test_launch_plan_with_marginals_is_the_plan_of_a_streaming_consumer(klib):
    """marg_nbins = 8 plans its launches exactly as acov_maxlag = 5 does, over the grid of tests/test_cov_host.py's plan test: the 32-column ring of its own
    ends launches where it would wrap, a ring or a full history the caller asked for is kept"""
    for kw in (dict(), dict(burnin=10, thinning=3), dict(steps_per_launch=48), dict(burnin=7, steps_per_launch=20, thinning=2),
               dict(hist_ring_cols=8), dict(hist_ring_cols=40, steps_per_launch=64)):
        for base in (0, L.MON_HISTORY, L.MON_SUMMARIES | L.MON_ACCEPT):
            runs = [150, 37, 13]
            marg = _plan(klib, runs, True, monitor=base, **kw)
            acov = _plan(klib, runs, monitor=base, acov_maxlag=5, **kw)
            assert marg == acov, (kw, base)
    plain = _plan(klib, [200], monitor=L.MON_SUMMARIES, steps_per_launch=48)
    marg = _plan(klib, [200], True, monitor=L.MON_SUMMARIES, steps_per_launch=48)
    assert plain[0] != marg[0] and max(marg[0]) <= 32 and max(plain[0]) == 48
    full = _plan(klib, [200], True, monitor=L.MON_HISTORY, steps_per_launch=48)
    assert full[0] == plain[0]                                                   # a full history has no ring to wrap


# ---------------------------------------------------------------- the NumPy forms
def test_numpy_slots_follow_the_index_formula():
    """stats.hist_slots on values whose slot is known by construction: exact binary edges (lo = -2, hi = 2, nbins = 16: w = 1/4), the outer slots, NaN"""
    x = np.array([-2.0, -1.75, -1.750000001, 1.75, 1.9999999, 2.0, -2.0000001, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.25])[:, None]
    want = [1, 2, 1, 16, 16, 17, 0, 17, 0, 17, 9, 9, 10]
    assert K.stats.hist_slots(x, 16, -2.0, 2.0)[:, 0].tolist() == want
    c = K.stats.pooled_hist(x, 16, -2.0, 2.0)
    assert c.shape == (1, 18) and c.dtype == np.uint64 and int(c.sum()) == x.size and c[0, 17] == 3 and c[0, 0] == 2 and c[0, 9] == 2
    assert K.stats.hist_slots(np.array([[0.3]]), 1, 0.0, 1.0)[0, 0] == 1         # nbins = 1: one inner slot


def _random_counts(rng, D, nbins, empty_rows=()):
    c = rng.integers(0, 50, size=(D, nbins + 2)).astype(np.uint64)
    c[rng.random(c.shape) < 0.4] = 0                                             # runs of empty bins
    c[:, 0] = rng.integers(0, 3, D); c[:, -1] = rng.integers(0, 3, D)
    for d in empty_rows:
        c[d] = 0
    return c


PROBS = np.array([1e-9, 0.001, 0.025, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.975, 0.999, 1.0])


@pytest.mark.parametrize("nbins", R.BINS + [7, 100])
def test_c_quantiles_equal_the_numpy_restatement_bit_for_bit(nbins):
    rng = np.random.default_rng(nbins)
    D = 9
    lo = rng.uniform(-5, 0, D); hi = lo + rng.uniform(0.1, 7, D)
    lo[1], hi[1] = 1e6, 1e6 + 1e-3
    counts = _random_counts(rng, D, nbins, empty_rows=(4,))
    counts[5] = 0; counts[5, 0] = 7                                              # everything below the range
    counts[6] = 0; counts[6, -1] = 3                                             # ... and above it
    counts[7, 1:-1] = 0; counts[7, 0] = 5; counts[7, -1] = 5                     # half below, half above: no inner count at all
    got = R.quantiles_c(counts, nbins, lo, hi, PROBS)
    want = K.stats.hist_quantiles(counts, nbins, lo, hi, PROBS)
    assert R.bits_differ(got, want) == 0
    assert R.bits_differ(K.histogram_quantiles(counts, nbins, lo, hi, PROBS), want) == 0
    assert np.all(np.isnan(got[4]))                                              # an empty dimension
    assert np.all(got[5] == -np.inf) and np.all(got[6] == np.inf)
    assert np.all(got[7][PROBS <= 0.5] == -np.inf) and np.all(got[7][PROBS > 0.5] == np.inf)
    rows = got[[0, 1, 2, 3, 8]]
    assert np.all(rows[:, :-1] <= rows[:, 1:])                                   # non-decreasing in p


def test_quantiles_refuse_bad_arguments():
    c = np.ones((2, 6), np.uint64); lo = np.zeros(2); hi = np.ones(2)
    assert R.quantiles_c(c, 4, lo, hi, [0.5], status=True) == L.OK
    for p in ([0.0], [-0.1], [1.0000001], [np.nan], [0.5, 2.0]):
        assert R.quantiles_c(c, 4, lo, hi, p, status=True) == L.ERR_INVALID_ARG, p
        with pytest.raises(ValueError):
            K.stats.hist_quantiles(c, 4, lo, hi, p)
    klib = L.load()
    p = np.array([0.5]); out = np.zeros((2, 1))
    args = [c.ctypes.data, 2, 4, lo.ctypes.data, hi.ctypes.data, 1, p.ctypes.data, out.ctypes.data]
    for i in (0, 3, 4, 6, 7):
        a = list(args); a[i] = None
        assert klib.klara_histogram_quantiles(*a) == L.ERR_INVALID_ARG, i
    for i, v in ((1, 0), (2, 0), (2, 1025), (5, 0)):
        a = list(args); a[i] = v
        assert klib.klara_histogram_quantiles(*a) == L.ERR_INVALID_ARG, (i, v)


@pytest.mark.parametrize("nbins,kind", [(64, "per_dim"), (1024, "per_dim"), (2, "per_dim"), (64, "offset")])
def test_quantiles_within_one_bin_of_the_order_statistic(nbins, kind):
    """Against the exact order statistic x_(k), k = max(1, ceil(p n)) (np.quantile(..., method="inverted_cdf"), checked against a sort), where x_(k) lies
    in an inner slot.  The bound, derived, with u = 2^-53, w = (hi - lo) / nbins and A = |lo| + |hi| >= hi - lo:
      - the result is left_b + w (k - cum) / c_b with 0 < (k - cum) / c_b <= 1: it lies in (left_b, left_b + w] up to the roundings of left_b = lo + (b - 1) w
        (w: 2 u relative, the product one more, the sum u max(|lo|, |hi|): at most 3 u (hi - lo) + u A) and of the last product, quotient and sum (3 u A);
      - x_(k) was put into slot b by floor((x - lo) * inv_w) = b - 1: x - lo is exact to u relative, inv_w to 2 u, the product to u, so the slot's true
        extent [lo + (b - 1) w, lo + b w) is met up to 4 u nbins w = 4 u (hi - lo) at either end;
      hence |result - x_(k)| <= w + (3 + 4) u (hi - lo) + 4 u A <= w + 16 u A — one bin width plus the rounding of the edges."""
    N, D, nc = 50, 5, 40
    hist = R.make_hist(nc, N, D, kind)
    lo, hi = R.bounds(D, kind)
    counts = K.stats.pooled_hist(hist, nbins, lo, hi)
    got = R.quantiles_c(counts, nbins, lo, hi, PROBS)
    flat = hist.reshape(-1, D)
    n = flat.shape[0]
    order = np.quantile(flat, PROBS, axis=0, method="inverted_cdf").T           # (D, nprobs)
    srt = np.sort(flat, axis=0)
    k = np.maximum(1, np.ceil(PROBS * n)).astype(int)
    assert np.array_equal(order, srt[k - 1].T)
    w = (hi - lo) / nbins
    bound = (w + 16 * 2.0 ** -53 * (np.abs(lo) + np.abs(hi)))[:, None]
    below = order < lo[:, None]; above = ~(order < hi[:, None]); inner = ~below & ~above
    err = np.abs(got - order)
    print(f"marg quantiles nbins={nbins} {kind}: largest |q - x_(k)| / bound {np.max(err[inner] / np.broadcast_to(bound, err.shape)[inner]):.3g} over {inner.sum()} "
          f"inner, {below.sum()} below, {above.sum()} above")
    assert inner.sum() > 0 and below.sum() > 0 and above.sum() > 0
    assert np.all(err[inner] <= np.broadcast_to(bound, err.shape)[inner])
    assert np.all(got[below] == -np.inf) and np.all(got[above] == np.inf)       # the k-th sample lies in an outer slot: infinities, never a clipped number


# ---------------------------------------------------------------- torch.distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


SHARD_SHAPE = (9, 2 * 64 + 5, 17)


def _worker(rank, world, port, q):
    import sys
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    import torch.distributed as dist
    import klara_jl_amd as K
    import marg_ref as R
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nc, N, D = SHARD_SHAPE
    hist = R.make_hist(nc, N, D)
    lo, hi = R.bounds(D)
    b = [0, N // 3, N]
    mine = K.stats.pooled_hist(hist[:, b[rank]:b[rank + 1]], 64, lo, hi)        # what Engine.pooled_histogram() hands a rank
    q.put((rank, K.allreduce_histogram(mine)))
    dist.destroy_process_group()


def test_allreduce_histogram_world2_is_the_unsharded_table():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60); assert p.exitcode == 0
    nc, N, D = SHARD_SHAPE
    want = K.stats.pooled_hist(R.make_hist(nc, N, D), 64, *R.bounds(D))
    for _, got in res:
        assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert int(want.sum()) == nc * N * D
    one = K.allreduce_histogram(want)                                            # no process group: the table itself
    assert np.array_equal(one, want) and one is not want


# ---------------------------------------------------------------- the host code under the sanitizers
_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "klara_marg_host.h"
// klara_marg_quantiles on tables of every shape the tests use: full, sparse, empty, everything in one outer slot; bad arguments
int main()
{
    unsigned long long s = 88172645463325252ull;
    int bad = 0;
    const long long bins[] = {1, 2, 7, 64, 1024};
    for (long long nbins : bins)
        for (int D : {1, 3, 17}) {
            std::vector<uint64_t> c((size_t)D * (nbins + 2));
            for (auto& v : c) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = (s & 3) ? (s >> 40) % 50 : 0; }
            if (D > 1) for (long long i = 0; i < nbins + 2; ++i) c[(size_t)(nbins + 2) + i] = 0;            // an empty dimension
            if (D > 2) { for (long long i = 0; i < nbins + 2; ++i) c[(size_t)2 * (nbins + 2) + i] = 0; c[(size_t)3 * (nbins + 2) - 1] = 9; }
            std::vector<double> lo(D, -1.5), hi(D, 2.25), p = {1e-12, 0.025, 0.5, 0.975, 1.0}, out((size_t)D * p.size(), -1.0);
            if (klara_marg_quantiles(c.data(), D, nbins, lo.data(), hi.data(), (int)p.size(), p.data(), out.data()) != 0) ++bad;
            for (size_t j = 0; j + 1 < p.size(); ++j) if (out[j] > out[j + 1]) ++bad;                      // non-decreasing in p
            if (D > 1 && out[p.size()] == out[p.size()]) ++bad;                                             // NaN for the empty dimension
            if (D > 2 && !(out[2 * p.size()] > 1e300)) ++bad;                                               // +inf: everything above the range
            const double pb[] = {0.0};
            if (klara_marg_quantiles(c.data(), D, nbins, lo.data(), hi.data(), 1, pb, out.data()) != 1) ++bad;
            if (klara_marg_quantiles(nullptr, D, nbins, lo.data(), hi.data(), 1, p.data(), out.data()) != 1) ++bad;
        }
    // the ranks' agreement words: two ranks reduced by hand (maximum), identical and differing in nbins / in one bound
    for (int D : {1, 7}) {
        const size_t NV = 2 * (size_t)D + 1;
        std::vector<double> lo(D, -1.5), hi(D, 2.25), lo2(lo);
        lo2[D - 1] = -1.25;
        std::vector<uint64_t> a(2 * NV), b(2 * NV), r(2 * NV);
        const auto reduced = [&](long long nb2, const std::vector<double>& l2) {
            klara_marg_agreement_words(64, lo.data(), hi.data(), D, a.data());
            klara_marg_agreement_words(nb2, l2.data(), hi.data(), D, b.data());
            for (size_t i = 0; i < 2 * NV; ++i) r[i] = a[i] > b[i] ? a[i] : b[i];
            return klara_marg_words_agree(r.data(), NV);
        };
        if (reduced(64, lo) != 1) ++bad;
        if (reduced(65, lo) != 0) ++bad;
        if (reduced(64, lo2) != 0) ++bad;
    }
    printf(bad ? "BAD %d\n" : "CLEAN\n", bad);
    return bad != 0;
}
'''


def test_quantile_code_runs_clean_under_the_host_sanitizers(tmp_path):
    """klara_marg_host.h — all of klara_histogram_quantiles but its extern "C" line, and the ranks' agreement words — with a small main of its own, built with
    -fsanitize=address,undefined and run once as a stand-alone program (nothing loaded into Python runs under a sanitizer)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    src = tmp_path / "marg_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "marg_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(ROOT / "klara.jl_amd" / "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "CLEAN", (r.stdout[-2000:], r.stderr[-3000:])
