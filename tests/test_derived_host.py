"""CPU side of the derived quantities (klara_desc.derived_src ..., klara_get_derived_sums, klara_gather_derived_*): the library surface — header, binding,
Julia stub, exports — is consistent; klara_create refuses every bad descriptor without a device; the closures of tests/derived_cases.py compile for gfx950
here and a bad text is reported with its name and line; the kernel's geometry is the stated function of (N, D, K); the NumPy form of the sums is exact on
inputs whose partial sums are exact; and the gcc build of the predictive-probability closure is its NumPy evaluation with the project's kd_exp."""
import ctypes as C
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import derived_cases as DC
import derived_ref as R
import klara_jl_amd as K
import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
NEW_FIELDS = [("derived_src", "const char*"), ("derived_data", "const double*"), ("derived_ndata", "int64_t"), ("derived_nout", "int64_t"),
              ("derived_nbins", "int64_t"), ("derived_lo", "const double*"), ("derived_hi", "const double*")]
NEW_FUNCS = ["klara_get_derived_sums", "klara_gather_derived_moments", "klara_gather_derived_rhat", "klara_gather_derived_histogram", "klara_check_derived",
             "klara_selftest_derived_plan", "klara_selftest_derived"]


# ---------------------------------------------------------------- the library surface
def test_header_binding_julia_and_exports_agree(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    body = re.search(r"typedef struct klara_desc \{(.*?)\} klara_desc;", hdr, re.S).group(1)
    cfields = re.findall(r"^\s{4}((?:const\s+)?\w+\*?)\s+(\w+);", body, re.M)
    names = [n for _, n in cfields]
    i = names.index("steps_per_launch")
    assert [(n, " ".join(t.split())) for t, n in cfields[i + 1:i + 8]] == NEW_FIELDS          # directly behind steps_per_launch, in the stated order ...
    assert names[i + 8] == "stream" and names[-1] == "stream"                                # ... and directly before stream, which stays last
    pyf = [n for n, _ in L.KlaraDesc._fields_]
    assert pyf == names
    types = dict(L.KlaraDesc._fields_)
    assert types["derived_src"] is C.c_char_p and types["derived_data"] is types["derived_lo"] is types["derived_hi"] is types["marg_lo"]
    assert types["derived_ndata"] is types["derived_nout"] is types["derived_nbins"] is C.c_int64
    # seven 8-byte fields, no padding: the struct grew by exactly 56
    assert L.KlaraDesc.derived_src.offset == L.KlaraDesc.steps_per_launch.offset + 4
    for k, (n, _) in enumerate(NEW_FIELDS):
        assert getattr(L.KlaraDesc, n).offset == L.KlaraDesc.derived_src.offset + 8 * k and getattr(L.KlaraDesc, n).size == 8
    assert L.KlaraDesc.stream.offset == L.KlaraDesc.derived_src.offset + 56
    assert sum(C.sizeof(t) for _, t in L.KlaraDesc._fields_) == C.sizeof(L.KlaraDesc)
    jstruct = re.search(r"struct KlaraDesc\n(.*?)\nend", jl, re.S).group(1)
    jfields = re.findall(r"(\w+)::([\w{}]+)", jstruct)
    assert [n for n, _ in jfields] == names
    jt = dict(jfields)
    assert jt["derived_src"] == "Cstring" and jt["derived_data"] == jt["derived_lo"] == jt["derived_hi"] == "Ptr{Float64}"
    assert jt["derived_ndata"] == jt["derived_nout"] == jt["derived_nbins"] == "Int64"
    call = re.search(r"KlaraDesc\(UInt32\(sizeof\(KlaraDesc\)\), KLARA_ABI_VERSION,(.*?)\)\nend", jl, re.S).group(1)
    assert [t for t in re.split(r"[,\s]+", call) if t] == names[2:]
    # still 7 monitor bits and ABI version 6: the feature is switched on by descriptor fields
    mons = [int(v, 16) for v in re.findall(r"#define KLARA_MON_[A-Z_]+\s+(0x[0-9a-f]+)u", hdr)]
    assert len(mons) == len(set(mons)) == 7
    assert "#define KLARA_ABI_VERSION 6 " in hdr and L.KLARA_ABI_VERSION == 6 and int(klib.klara_abi_version()) == 6
    assert int(re.search(r"#define KLARA_DERIVED_MAX_OUT (\d+)", hdr).group(1)) == L.DERIVED_MAX_OUT == 64
    assert re.search(r"const DERIVED_MAX_OUT = 64\b", jl)
    for name in NEW_FUNCS:
        proto = re.search(r"klara_status " + name + r"\((.*?)\);", hdr, re.S)
        assert name in L.EXPORTS and hasattr(klib, name) and proto, name
        nargs = proto.group(1).count(",") + 1
        assert len(getattr(klib, name).argtypes) == nargs, name                  # the binding's signature has the prototype's argument count ...
        for m in re.finditer(r"ccall\(\(:" + name + r", lib\), Cint,\s*\((.*?)\),\n?\s*", jl, re.S):     # ... and so has every Julia ccall of it
            assert len([t for t in re.split(r",\s*", m.group(1).strip()) if t]) == nargs, (name, m.group(1))
    for name in NEW_FUNCS[:5]:
        assert jl.count("(:" + name + ", lib)") == 1, name
    for name in ("Derived", "check_derived", "derived_mean", "derived_var", "derived_rhat", "derived_quantiles"):
        assert hasattr(K, name), name
    for name in ("derived_sums", "derived_moments", "derived_rhat", "derived_histogram"):
        assert hasattr(K.Engine, name), name
    assert hasattr(K.stats, "derived_sums")


def test_julia_names_are_present_and_do_not_collide():
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    txt = (ROOT / "tests" / "golden" / "klara_exports.txt").read_text().splitlines()
    klara = {t for t in txt if t and not t.startswith("[")}
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jl, re.M).group(1)
    exported = {t for t in re.split(r"[,\s]+", export) if t}
    for name in ("derivedsums", "derivedmoments", "derivedrhat", "derivedhistogram", "derivedquantiles", "gather_derived_moments", "gather_derived_rhat",
                 "gather_derived_histogram"):
        assert name in exported and name not in klara and re.search(r"^(function )?" + name + r"\(job::HIPMCJob", jl, re.M), name
    assert "Derived" in exported and "Derived" not in klara and "check_derived" in exported and "check_derived" not in klara
    assert "derived=nothing" in jl and "kw[:derived_nout] = Int64(derived.nout)" in jl


# ---------------------------------------------------------------- validation without a device
def _desc(**kw):
    d = L.KlaraDesc()
    d.struct_size = C.sizeof(L.KlaraDesc); d.abi_version = L.KLARA_ABI_VERSION
    d.sampler, d.target, d.nchains, d.ndims = L.SAMPLER_MALA, L.TARGET_GAUSS_DIAG, 256, 100
    d.driftstep, d.period, d.thinning, d.nsteps = 0.5, 100, 1, 200
    d.device = 1 << 20                                                           # (no such device: a descriptor that passes validation ends at KLARA_ERR_HIP)
    for key, v in kw.items():
        setattr(d, key, v)
    return d


def test_create_refuses_every_bad_descriptor_before_any_device_call(klib):
    src = DC.SRC_A.encode()
    data = np.arange(5.0); lo = np.array([-1.0, -2.0]); hi = np.array([1.0, 3.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    bad = lambda i, v, a: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    keep = []

    def create(**kw):
        for k, v in list(kw.items()):
            if isinstance(v, np.ndarray):
                keep.append(v); kw[k] = dp(v)
        h = C.c_void_p()
        st = klib.klara_create(C.byref(_desc(**kw)), C.byref(h))
        assert not h.value
        return st
    ok = dict(derived_src=src, derived_nout=2)
    hist = dict(ok, derived_nbins=8, derived_lo=lo, derived_hi=hi)
    refused = [
        dict(derived_src=src, derived_nout=-1), dict(derived_src=src, derived_nout=65),                      # nout outside 0 .. 64
        dict(derived_src=src), dict(derived_nout=2),                                                         # a source without nout, nout without a source
        dict(ok, derived_ndata=-1), dict(ok, derived_ndata=-1, derived_data=data), dict(ok, derived_data=data),      # a negative length, data without a length
        dict(ok, derived_ndata=5), dict(derived_data=data, derived_ndata=5),                                 # a length without data, data without a closure
        dict(hist, derived_nbins=-1), dict(hist, derived_nbins=1025),                                        # nbins outside its range
        dict(derived_nbins=8, derived_lo=lo, derived_hi=hi),                                                 # bins without nout
        dict(ok, derived_nbins=8), dict(ok, derived_nbins=8, derived_lo=lo), dict(ok, derived_nbins=8, derived_hi=hi),     # bounds NULL
        dict(hist, derived_lo=bad(0, np.nan, lo)), dict(hist, derived_lo=bad(1, -np.inf, lo)), dict(hist, derived_hi=bad(0, np.inf, hi)),
        dict(hist, derived_hi=bad(1, np.nan, hi)),                                                           # not finite
        dict(hist, derived_lo=bad(1, 3.0, lo)), dict(hist, derived_lo=bad(0, 2.0, lo)),                      # lo = hi, lo > hi
        dict(ok, derived_lo=lo), dict(ok, derived_hi=hi), dict(ok, derived_lo=lo, derived_hi=hi),            # bounds with nbins = 0
    ]
    for kw in refused:
        assert create(**kw) == L.ERR_INVALID_ARG, sorted(kw)
    for kw in (ok, hist, dict(ok, derived_nout=64), dict(hist, derived_nbins=1024), dict(ok, derived_data=data, derived_ndata=5), dict(hist, derived_nbins=1), {}):
        assert create(**kw) == L.ERR_HIP, sorted(kw)                             # valid: validation passes and the missing device is what stops it
    for fn, n in (("klara_get_derived_sums", 4), ("klara_gather_derived_moments", 6), ("klara_gather_derived_rhat", 8), ("klara_gather_derived_histogram", 5)):
        assert getattr(klib, fn)(*([None] * n)) == L.ERR_INVALID_ARG, fn


def test_selftest_refuses_every_bad_argument_before_any_device_call(klib):
    hist = np.zeros((4, 3, 2)); spl = np.array([4], np.int64); s = np.zeros((3, 2)); q = np.zeros((3, 2)); data = np.zeros(2)
    src = DC.SRC_A.encode()
    p = lambda v: None if v is None else v.ctypes.data

    def call(N=3, D=2, nc=4, h=hist, ns=1, sp=spl, text=src, K=2, d=None, nd=0, a=s, b=q):
        return klib.klara_selftest_derived(1 << 20, N, D, nc, p(h), ns, p(sp), text, K, p(d), nd, p(a), p(b), None)
    for kw in (dict(N=0), dict(D=0), dict(D=1025), dict(nc=0), dict(h=None), dict(sp=None), dict(text=None), dict(K=0), dict(K=65), dict(a=None), dict(b=None),
               dict(ns=0), dict(nd=-1), dict(nd=2), dict(d=data), dict(sp=np.array([5], np.int64)), dict(sp=np.array([3], np.int64)),
               dict(ns=2, sp=np.array([5, -1], np.int64))):
        assert call(**kw) == L.ERR_INVALID_ARG, sorted(kw)
    assert call() == L.ERR_HIP and call(d=data, nd=2) == L.ERR_HIP               # valid: stopped by the device only, before anything is compiled
    for N, D, Kk in ((0, 2, 2), (3, 0, 2), (3, 1025, 2), (3, 2, 0), (3, 2, 65)):
        assert R.plan(N, D, Kk, status=True) == L.ERR_INVALID_ARG


# ---------------------------------------------------------------- the run-time compiler, without a GPU
@pytest.mark.parametrize("name, D, nout", [("A", 3, DC.K_A), ("B", 100, DC.K_B), ("C", 5, DC.K_C), ("D", 3, DC.K_D)])
def test_the_closures_compile_for_gfx950(klib, name, D, nout):
    assert klib.klara_check_derived(getattr(DC, "SRC_" + name).encode(), D, nout) == L.OK, klib.klara_compile_log().decode(errors="replace")
    assert K.check_derived(getattr(DC, "SRC_" + name), D, nout) is True


def test_a_bad_text_is_reported_with_its_name_and_line(klib):
    assert klib.klara_check_derived(DC.SRC_NO_FUNCTION.encode(), 3, 1) == L.ERR_COMPILE
    assert "klara_user_derived" in klib.klara_compile_log().decode(errors="replace")
    assert klib.klara_check_derived(DC.SRC_SYNTAX_ERROR.encode(), 3, 2) == L.ERR_COMPILE
    log = klib.klara_compile_log().decode(errors="replace")
    assert re.search(r"klara_user_derived:%d:\d+: error" % DC.SYNTAX_ERROR_LINE, log), log
    with pytest.raises(K.KlaraError) as e:
        K.check_derived(DC.SRC_SYNTAX_ERROR, 3, 2)
    assert e.value.status == L.ERR_COMPILE and "klara_user_derived:%d" % DC.SYNTAX_ERROR_LINE in e.value.log
    for D, nout in ((0, 1), (1025, 1), (3, 0), (3, 65)):
        assert klib.klara_check_derived(DC.SRC_A.encode(), D, nout) == L.ERR_INVALID_ARG
    assert klib.klara_check_derived(None, 3, 1) == L.ERR_INVALID_ARG


# ---------------------------------------------------------------- geometry
def test_geometry_is_the_stated_function_of_the_shape():
    assert (R.LDS_BYTES, R.MAX_CH, R.MAX_COLS) == (61440, 256, 32)
    assert R.geometry(1, 29, 1)[0] == 256 and R.geometry(1, 100, 1)[0] == 76 and R.geometry(1, 1024, 1)[0] == 7
    for D in (1, 2, 29, 30, 100, 479, 480, 1024):
        ch, stride, thr, _, lds = R.geometry(1, D, 2)
        assert stride == D | 1 and stride % 2 == 1 and ch == min(256, 61440 // (8 * stride)) and thr == 64 * -(-ch // 64) and ch <= thr <= 256
        assert lds == 8 * ch * stride <= 61440 and 1 <= ch
        for mult in (1, 3):
            for N in (mult * ch - 1, mult * ch, mult * ch + 1):
                if N < 1:
                    continue
                for Kk in (1, 64):
                    got = R.plan(N, D, Kk)
                    assert got == R.geometry(N, D, Kk), (N, D, Kk)
                    assert got[3] == -(-N // ch) and (got[3] - 1) * ch < N <= got[3] * ch          # every chain has one owner


# ---------------------------------------------------------------- the NumPy form of the sums
def test_numpy_sums_are_exact_where_every_partial_sum_is():
    """small integers: every y, every product and every partial sum is an integer far below 2^53, so the float sums must equal the rational ones"""
    rng = np.random.default_rng(7)
    v = rng.integers(-9, 10, size=(11, 5, 3)).astype(np.float64)
    f = lambda x: (x[0] - x[1], x[0] * x[1], x[2])
    s, q = K.stats.derived_sums(v, f)
    assert s.shape == q.shape == (5, 3)
    for c in range(5):
        ys = [[Fraction(int(a)) for a in (x[0] - x[1], x[0] * x[1], x[2])] for x in v[:, c]]
        for k in range(3):
            assert Fraction(s[c, k]) == sum(y[k] for y in ys) and Fraction(q[c, k]) == sum(y[k] * y[k] for y in ys)
    # ... and it is the reference's order of operations on any input
    h = DC.history(6, 4, 3)
    s2, q2 = K.stats.derived_sums(h, lambda x: (x[0] - x[1], x[0] * x[1]))
    rs, rq, _ = R.reference(DC.SRC_A, DC.K_A, h)
    assert R.bits_differ(s2, rs) == 0 and R.bits_differ(q2, rq) == 0
    with pytest.raises(ValueError):
        K.stats.derived_sums(np.zeros((3, 2)), f)


def test_gcc_build_of_the_predictive_probability_is_its_numpy_evaluation():
    """closure (c) on twenty points: eta summed in ascending j, one rounded product and one addition per term; kd_exp from the project's oracle"""
    D = 5
    x = DC.history(1, 20, D, seed=3, scale=2.0)[0]
    row = DC.covariate_row(D)
    got = R.evaluate(DC.SRC_C, DC.K_C, x, row)[:, 0]
    eta = np.zeros(20)
    for j in range(D):
        eta = eta + row[j] * x[:, j]
    want = 1.0 / (1.0 + O.math_op(1, -eta))
    assert got.shape == (20,) and R.bits_differ(got, want) == 0 and np.all((got > 0.0) & (got < 1.0))
    assert np.max(np.abs(got - 1.0 / (1.0 + np.exp(-eta)))) < 1e-15


def test_reference_flows_nan_through_as_ieee():
    h = DC.half_negative_history(5, 6, 3, seed=1)
    s, q, y = R.reference(DC.SRC_D, DC.K_D, h)
    neg = (h[:, :, 0] < 0.0).any(axis=0)
    assert np.array_equal(neg, np.arange(6) % 2 == 1)
    assert np.array_equal(np.isnan(s[:, 0]), neg) and np.array_equal(np.isnan(q[:, 0]), neg) and np.array_equal(np.isnan(y[:, :, 0]), h[:, :, 0] < 0.0)
