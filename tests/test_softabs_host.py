"""The softabs transform of the SMMALA metric without a GPU: the host build of klara.jl_amd/csrc/klara_softabs.h against 60-digit arithmetic
(mpmath), the CPU reference (oracle/klara_oracle.c ko_smmala) against the independent NumPy restatement (tests/smmala_mirror.py with
stats.softabs), the descriptor mapping and refusals of the C ABI, the Python and Julia interfaces, the run-time compiled kernels'
resources, and the committed vectors."""
import importlib.util
import re
import shutil
import subprocess
from pathlib import Path

import mpmath as mp
import numpy as np
import pytest

import cases
import klara_jl_amd as K
import smmala_cases as SC
import smmala_mirror as SM
import softabs_cases as SAC
import softabs_ref as SR
from klara_jl_amd import _lib as L
from klara_jl_amd import stats

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -52

# ---------------------------------------------------------------- the scalar lambda / tanh(a lambda)
# The largest error the function shows is 2.4 ulps on the points below and 2.5 on a sample ten times as large (x86-64, gcc; the device computes the same bits).  Its parts, for |a lambda| >= 1/2:
# kd_exp's < 1 ulp times t / (1 + t) + t / (1 - t) <= 0.85, the rounding of a lambda carried through exp (<= 0.43), and four roundings
# (1 + t, 1 - t, the quotient, the product) of half an ulp each: 3.3 at most.  The cap is 4; a form that cancels
# near the crossover (70 ulps at 1e-3 for the exponential form alone) fails it.
F_CAP_ULPS = 4.0


def _f_true(lam, a):
    u = mp.mpf(a) * mp.mpf(lam)
    return 1 / mp.mpf(a) if u == 0 else mp.mpf(lam) / mp.tanh(u)


def _ulps(got, true):
    ulp = mp.mpf(2) ** (mp.floor(mp.log(abs(true), 2)) - 52)
    return float(abs(mp.mpf(got) - true) / ulp)


def test_scalar_against_60_digits():
    mp.mp.dps = 60
    cross = SR.limits()[2]
    rng = np.random.default_rng(1)
    us = np.concatenate([10.0 ** rng.uniform(-320, 4, 1500), 10.0 ** rng.uniform(-3, 1, 2500), rng.uniform(0.8 * cross, 1.2 * cross, 2000),
                         cross * (1.0 + rng.uniform(-1e-5, 1e-5, 300)), [cross, np.nextafter(cross, 0), np.nextafter(cross, 1), 1e-320, 1e4, 1e-3]])
    worst = 0.0
    for a in (1.0, 1000.0, 0.37):
        for u in us:
            for sign in (1.0, -1.0):
                lam = sign * u / a
                worst = max(worst, _ulps(SR.f(lam, a), _f_true(lam, a)))
    print(f"lambda / tanh(a lambda): largest error {worst:.3f} ulps (cap {F_CAP_ULPS})")
    assert worst <= F_CAP_ULPS


def test_scalar_limits():
    for a in (1.0, 1000.0, 0.37, 3.0):
        assert SR.f(0.0, a) == 1.0 / a and SR.f(-0.0, a) == 1.0 / a               # the limit, exactly (the reference: 0 / 0)
        assert SR.f(1e-320, a) == 1.0 / a
        for lam in (1e-9, 0.3, 0.5 / a, 2.0, 77.0, 1e6 / a, 1e300):
            assert SR.f(lam, a) == SR.f(-lam, a) > 0.0                              # even
        assert SR.f(1e6 / a, a) == 1e6 / a and SR.f(-1e6 / a, a) == 1e6 / a         # |lambda| for large |a lambda|: no overflow
        assert SR.f(1e306, a) == 1e306 and np.isfinite(SR.f(1e308 / max(a, 1.0), a))
    assert np.isnan(SR.f(float("nan"), 1.0))


# ---------------------------------------------------------------- the matrix transform
def _true_softabs(H, a):
    n = H.shape[0]
    E, Q = mp.eigsy(mp.matrix(H.tolist()))
    f = [_f_true(E[k], a) for k in range(n)]
    T = mp.zeros(n)
    for k in range(n):
        for i in range(n):
            for j in range(n):
                T[i, j] += f[k] * Q[i, k] * Q[j, k]
    return T


def _err(T, Tt):
    n = T.shape[0]
    nrm = mp.norm(Tt, 2) if n > 1 else abs(Tt[0, 0])
    return float(max(abs(mp.mpf(float(T[i, j])) - Tt[i, j]) for i in range(n) for j in range(n)) / (mp.mpf(EPS) * nrm))


def _matrices():
    rng = np.random.default_rng(20261017)
    out = []
    for d in (1, 2, 3, 5, 8):
        for spread in (1.0, 1e3, 1e6):
            for rep in range(3):
                Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
                lam = rng.choice([-1.0, 1.0], d) * (np.exp(rng.uniform(0.0, np.log(spread), d)) if spread > 1.0 else rng.uniform(0.5, 1.0, d))
                if rep == 2 and d > 1:
                    lam[0] = 1e-9                                                # one eigenvalue of order 1e-9
                H = (Q * lam) @ Q.T
                out.append((f"d{d}_spread{spread:g}_{rep}", 0.5 * (H + H.T)))
    Q3, _ = np.linalg.qr(rng.standard_normal((5, 5)))
    rep = (Q3 * np.array([2.0, 2.0, 2.0, -3.0, 0.5])) @ Q3.T
    out += [("diagonal", np.diag([3.0, -1e-4, 0.0, 7e5, -2.0])),
            ("repeated", 0.5 * (rep + rep.T)),
            ("theta0", np.array([[1.5, 0.25], [0.25, 1.5]])),
            ("tiny_off", np.diag([1.0, -2.0, 3.0, 0.5]) + 1e-200 * (np.ones((4, 4)) - np.eye(4))),
            ("tiny_off_equal_diag", np.array([[1.0, 1e-200], [1e-200, 1.0]]))]
    return out


def test_matrix_transform_against_60_digits():
    """cap: 4 x the largest error stats.softabs (LAPACK's eigh, the path Julia's eig takes) shows against the same truth on the same matrices.
    Measured here (x86-64, OpenBLAS): eigh 3.75, the Jacobi path 5.77 (units of eps ||T||_2), at most 6 sweeps."""
    mp.mp.dps = 60
    cap_sweeps = SR.limits()[0]
    worst_dev, worst_eigh, most = 0.0, 0.0, 0
    for name, H in _matrices():
        for a in (1.0, 1000.0):
            Tt = _true_softabs(H, a)
            T, sweeps = SR.softabs(H, a)
            assert 0 <= sweeps < cap_sweeps, (name, a, sweeps)                        # the sweep cap was not the reason for stopping
            assert np.array_equal(T, T.T) and np.all(np.isfinite(T)), (name, a)
            np.linalg.cholesky(T)                                                    # positive definite
            e_dev = _err(T, Tt)
            with np.errstate(invalid="ignore", divide="ignore"):
                Tn = stats.softabs(H, a)
            e_eigh = _err(Tn, Tt) if np.all(np.isfinite(Tn)) else 0.0                # (a zero eigenvalue: the reference's 0 / 0)
            worst_dev, worst_eigh, most = max(worst_dev, e_dev), max(worst_eigh, e_eigh), max(most, sweeps)
    print(f"softabs: klara_softabs.h {worst_dev:.2f}, eigh {worst_eigh:.2f} (eps ||T||_2), most sweeps {most}")
    assert worst_dev <= 4.0 * worst_eigh, (worst_dev, worst_eigh)


def test_matrix_transform_hand_made_cases():
    a = 3.0
    d = np.array([3.0, -1e-4, 0.0, 7e5, -2.0])
    T, sweeps = SR.softabs(np.diag(d), a)
    assert sweeps == 0                                                               # already diagonal: no rotation ...
    assert np.array_equal(T, np.diag([SR.f(v, a) for v in d]))                       # ... and exactly f of the diagonal
    T, sweeps = SR.softabs(np.array([[1.5, 0.25], [0.25, 1.5]]), a)                  # theta = 0
    assert sweeps == 1 and np.allclose(T, stats.softabs(np.array([[1.5, 0.25], [0.25, 1.5]]), a), rtol=1e-14)
    T, sweeps = SR.softabs(np.array([[1.0, 1e-200], [1e-200, 1.0]]), a)              # off-diagonals that underflow when squared
    assert sweeps == 0 and np.array_equal(T, np.diag([SR.f(1.0, a)] * 2))
    T, _ = SR.softabs(np.array([[-4.0]]), a)                                         # D = 1: T = f(g)
    assert T[0, 0] == SR.f(-4.0, a)
    # the padding does not enter: the same matrix held in 4 or 8 elements per lane
    H = np.array([[0.3, -1.0, 0.2], [-1.0, -2.0, 0.7], [0.2, 0.7, 1.1]])
    assert np.array_equal(SR.softabs(H, a, E=4)[0], SR.softabs(H, a, E=8)[0])
    # only the upper triangle is read (T3)
    Hl = H.copy(); Hl[2, 0] = 99.0
    assert np.array_equal(SR.softabs(Hl, a)[0], SR.softabs(H, a)[0])
    # a non-finite entry, or one whose square overflows, is not transformed (T4): the result carries a NaN
    for bad in (np.nan, np.inf, -np.inf, 1e200):
        Hb = H.copy(); Hb[0, 2] = Hb[2, 0] = bad
        T, sweeps = SR.softabs(Hb, a)
        assert sweeps == -1 and np.isnan(T[0, 0])


# ---------------------------------------------------------------- reference against mirror
@pytest.mark.parametrize("name", SAC.NAMES)
def test_reference_matches_numpy_restatement(name):
    case = SAC.make(name)
    n, nsteps = 8, case["nsteps"]
    pooled = case.get("tuner_mode", L.TUNE_PER_CHAIN) == L.TUNE_POOLED
    job = SAC.ref_job(case, nchains=n)
    assert job.set_state(case["x0"][:n]) == 0
    assert job.run(nsteps) == 0
    chains = SAC.mirror_chains(case, nchains=n)
    if pooled:
        rows = SM.run_pooled(chains, nsteps, tuner="rate", targetrate=case["targetrate"], period=case["period"], burnin=case.get("burnin", 0))
    else:
        for c in chains:
            c.run(nsteps)
        rows = np.array([c.accepts for c in chains], dtype=np.uint8).T
    assert np.array_equal(job.accept, rows), "accept masks differ between the C reference and the NumPy restatement"
    np.testing.assert_allclose(job.X, np.array([c.x for c in chains]), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.LT, [c.lt for c in chains], rtol=1e-10, atol=1e-10)
    steps = job.step if not pooled else np.full(n, job.step[0])
    np.testing.assert_allclose(steps, [c.step for c in chains], rtol=1e-12)
    assert 0.0 < job.accept.mean() < 1.0, "a case that never (or always) accepts tests nothing"
    nmetrics, _, most = SR.sweep_stats()
    assert nmetrics >= n * (1 + nsteps) and most < SR.limits()[0]


def test_banana_starts_where_the_hessian_is_indefinite():
    """what the feature is for: without the transform these start states are KLARA_ERR_NONFINITE_INIT (SMMALA deviation S5)"""
    import autodiff_ref
    case = SAC.make("banana_ad2")
    _, _, tensor = case["mirror"]
    indefinite = [np.linalg.eigvalsh(tensor(x)).min() < 0.0 for x in case["x0"]]
    assert 10 < sum(indefinite) < case["nchains"] - 10
    kw = cases.oracle_kwargs(SAC.engine_case(case)); kw.pop("layout"); kw.pop("smmala_softabs")
    plain = autodiff_ref.AdSmmalaRefJob(**kw)
    assert plain.set_state(case["x0"]) == L.ERR_NONFINITE_INIT
    assert SAC.ref_job(case).set_state(case["x0"]) == 0


def test_bivariate_device_route_agrees_with_the_host_formed_metric():
    """the existing golden smmala_bivariate.npz forms softabs(-2C) on the host; the reference with the transform on the raw -2C takes the same
    decisions over its 40 steps, none of them a near-tie (the GPU test compares the device with the same golden)"""
    g = np.load(ROOT / "tests" / "golden" / "smmala_bivariate.npz")
    case = SAC.make("bivariate_device")
    job = SAC.ref_job(case)
    assert job.set_state(g["x0"]) == 0 and job.run(case["nsteps"]) == 0
    assert np.array_equal(job.accept, g["accept"])
    np.testing.assert_allclose(job.X, g["X"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(job.LT, g["LT"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- host API
def _status(**over):
    kw = dict(sampler=L.SAMPLER_SMMALA, target=SC.quad_target(0.5, np.eye(3), -np.eye(3)), nchains=4, nsteps=10, driftstep=0.5, smmala_softabs=1000.0)
    kw.update(over)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


def _raw_status(target_kind=L.TARGET_LOGISTIC, **fields):
    """klara_create on a hand-filled descriptor (the Engine refuses the logistic combination before create)"""
    import ctypes as C
    X, y = cases.swiss_data()
    X, y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    d = L.KlaraDesc()
    d.struct_size = C.sizeof(L.KlaraDesc); d.abi_version = L.KLARA_ABI_VERSION
    d.sampler, d.target, d.nchains, d.ndims, d.nsteps, d.thinning, d.period, d.driftstep = L.SAMPLER_SMMALA, target_kind, 4, 4, 10, 1, 100, 0.1
    d.logit_X, d.logit_y = X.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double))
    d.logit_ndata, d.logit_lambda = X.shape[0], 100.0
    for k, v in fields.items():
        setattr(d, k, v)
    h = C.c_void_p()
    st = L.load().klara_create(C.byref(d), C.byref(h))
    if st == 0:
        L.load().klara_destroy(h)
    return st


def test_descriptor_field_and_refusals(klib):
    import ctypes as C
    names = [n for n, _ in L.KlaraDesc._fields_]
    assert names[names.index("sparse_moves") + 1] == "smmala_softabs" and names[-1] == "stream"
    assert L.KlaraDesc.smmala_softabs.size == 8 and L.KlaraDesc.mh_sigma.offset == 48
    assert klib.klara_abi_version() == 6
    assert _status() in (0, L.ERR_HIP)
    assert _status(smmala_softabs=0.0) in (0, L.ERR_HIP, L.ERR_NONFINITE_INIT)
    for d in (1, 2, 8):
        assert _status(target=SC.quad_target(0.5, np.eye(d), -np.eye(d))) in (0, L.ERR_HIP)
    assert _status(target=SAC.make("banana_ad2")["target"]) in (0, L.ERR_HIP)
    # negative or not finite
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert _status(smmala_softabs=bad) == L.ERR_INVALID_ARG, bad
    # above 0 with another sampler
    assert _status(sampler=L.SAMPLER_MALA) == L.ERR_INVALID_ARG
    assert _status(sampler=L.SAMPLER_HMC) == L.ERR_INVALID_ARG
    assert _status(sampler=L.SAMPLER_MH, mh_sigma=np.ones(3)) == L.ERR_INVALID_ARG
    # the logistic target: positive definite by construction, not transformed
    assert _raw_status(smmala_softabs=1000.0) == L.ERR_UNSUPPORTED
    assert _raw_status(smmala_softabs=0.0) in (0, L.ERR_HIP)
    assert _raw_status(smmala_softabs=-1.0) == L.ERR_INVALID_ARG
    # the existing refusals
    assert _status(target=SC.quad_target(0.5, np.eye(9), np.eye(9))) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget(4, "#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + SC.SRC_QUAD_TENSOR)) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget(4, "#define KLARA_USER_PAIR_TARGET 1\n" + SC.SRC_QUAD_TENSOR)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDiagTarget.negdot(4)) == L.ERR_UNSUPPORTED
    assert _status(driftstep=0.0) == L.ERR_INVALID_ARG
    X, y = cases.swiss_data()
    with pytest.raises(ValueError, match="positive definite by construction"):
        K.Engine(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=10, driftstep=0.1, smmala_softabs=1000.0)


def test_python_interface():
    s = K.SoftAbs()
    assert s.a == 1000.0 and K.SoftAbs(2.5).a == 2.5 and callable(s)
    H = np.array([[0.3, -1.0], [-1.0, -2.0]])
    assert np.array_equal(K.SoftAbs(7.0)(H), stats.softabs(H, 7.0))
    lam, Q = np.linalg.eigh(H)
    assert np.allclose(stats.softabs(H, 7.0), (Q * (lam / np.tanh(7.0 * lam))) @ Q.T, rtol=0, atol=0)      # metrics.jl:1-4, literally
    assert np.allclose(stats.softabs(H), stats.softabs(H, 1000.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            K.SoftAbs(bad)
    smp = K.SMMALA(1.25, K.SoftAbs(1000.0))                                          # BivariateNormal/SMMALA/analytical.jl:16
    assert smp.driftstep == 1.25 and smp.transform.a == 1000.0
    assert K.SMMALA().transform is None and K.SMMALA(0.5, None).transform is None
    with pytest.raises(NotImplementedError, match="SoftAbs"):
        K.SMMALA(1.25, lambda H: stats.softabs(H, 1000.0))                           # a closure cannot be recognised


def test_basic_mc_job_maps_the_transform(monkeypatch):
    import klara_jl_amd.api as A
    seen = {}

    class FakeEngine:
        def __init__(self, **kw):
            seen.clear(); seen.update(kw)

        def set_state(self, x):
            pass

    monkeypatch.setattr(A, "Engine", FakeEngine)
    case = SAC.make("banana_ad2")
    p = K.BasicContMuvParameter("p", logtarget=case["target"])
    K.BasicMCJob(K.likelihood_model(p), K.SMMALA(0.7, K.SoftAbs(3.0)), K.BasicMCRange(nsteps=50, burnin=10), {"p": np.zeros(2)})
    assert seen["sampler"] == L.SAMPLER_SMMALA and seen["driftstep"] == 0.7 and seen["smmala_softabs"] == 3.0
    K.BasicMCJob(K.likelihood_model(p), K.SMMALA(0.7), K.BasicMCRange(nsteps=50, burnin=10), {"p": np.zeros(2)})
    assert seen.get("smmala_softabs", 0.0) == 0.0
    X, y = cases.swiss_data()
    pl = K.BasicContMuvParameter("p", logtarget=K.LogisticTarget(X, y, 100.0))
    with pytest.raises(ValueError, match="positive definite by construction"):
        K.BasicMCJob(K.likelihood_model(pl), K.SMMALA(0.02, K.SoftAbs()), K.BasicMCRange(nsteps=50, burnin=10), {"p": SC.SWISS_X0})


def test_julia_binding():
    """mechanical check of julia/KlaraHIP (no Julia here)"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"^struct SoftAbs <: Function; a::Float64; end$", src, re.M)
    assert re.search(r"^\(s::SoftAbs\)\(H\) = Klara\.softabs\(H, s\.a\)$", src, re.M)
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    assert re.search(r"\bSoftAbs\b", export) and re.search(r"\bcheck_custom_target_softabs\b", export)
    body = re.search(r"isa\(sampler,\s*SMMALA\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S).group(1)
    assert "isa(tr, SoftAbs)" in body and "kw[:smmala_softabs] = tr === nothing ? 0.0 : tr.a" in body
    assert "SoftAbs" in re.search(r"error\(\"(SMMALA:[^\"]*)\"\)", body).group(1)          # the refusal of a closure names it
    assert re.search(r"ccall\(\(:klara_check_custom_target_softabs, lib\), Cint, \(Cstring, Cint\), src, ndims\)", src)
    assert "SMMALA(1.25, SoftAbs(1000.))" in (ROOT / "INTEGRATION.md").read_text()


def test_check_custom_target_softabs(klib):
    def check(src, d):
        return klib.klara_check_custom_target_softabs(src.encode(), d)
    for d in (1, 3, 8):
        assert check(SC.SRC_QUAD_TENSOR, d) == 0, klib.klara_compile_log().decode()
    assert check(SAC.make("doublewell_d5")["target"].source, 5) == 0, klib.klara_compile_log().decode()
    assert check(SC.SRC_QUAD_TENSOR, 9) == L.ERR_UNSUPPORTED
    assert check(cases.SRC_NEGDOT, 3) == L.ERR_COMPILE
    assert b"klara_user_tensorlogtarget" in klib.klara_compile_log()
    assert check("#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + SC.SRC_QUAD_TENSOR, 3) == L.ERR_UNSUPPORTED
    assert check(SC.SRC_QUAD_TENSOR, 0) == L.ERR_INVALID_ARG
    SC.quad_target(0.5, np.eye(3), -np.eye(3)).check_softabs()
    with pytest.raises(K.KlaraError) as ei:
        K.CustomTarget(3, cases.SRC_NEGDOT).check_softabs()
    assert ei.value.status == L.ERR_COMPILE


# ---------------------------------------------------------------- resources of the run-time compiled kernels
def _kernel_resources(tmp_path, src, d):
    """the translation unit klara_jit.hip hands the run-time compiler for an SMMALA job with the transform, compiled by hipcc with the Makefile's flags"""
    csrc = ROOT / "klara.jl_amd" / "csrc"
    mk = (csrc / "Makefile").read_text()
    flags = [f for f in re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split() if f != "-fPIC"]
    arch = re.search(r"^ARCH \?= (\S+)$", mk, re.M).group(1)
    assert arch == "gfx950" and "-O3" in flags and "-ffp-contract=off" in flags
    assert '#define KLARA_SMMALA_SOFTABS 1' in (csrc / "klara_jit.hip").read_text()
    e = SR.pad_of(d)
    tu = (f"#define KLARA_D {d}\n#define KLARA_SMMALA 1\n#define KLARA_SMMALA_SOFTABS 1\n#include \"klara_kernels.h\"\n"
          "#define KLARA_USER_FN static __device__ __forceinline__\n" + src + "\n#include \"klara_custom.h\"\n")
    for mode in (0, 1, 3, 7):
        tu += f"template __global__ void k_transitions<KLARA_SAMPLER_SMMALA, KLARA_TARGET_CUSTOM, {e}, 1, {mode}>(const KParams*, const KLaunch);\n"
    tu += f"template __global__ void k_init_smmala<KLARA_TARGET_CUSTOM, {e}, 1>(const KParams, int);\n"
    f = tmp_path / f"softabs_d{d}.hip"
    f.write_text(tu)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is what builds the library: it must be there"
    out = tmp_path / f"softabs_d{d}.s"
    r = subprocess.run([hipcc, f"--offload-arch={arch}", *flags, "-Rpass-analysis=kernel-resource-usage", "-I", str(csrc), "-I", str(ROOT / "include"),
                        "-S", "--cuda-device-only", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for blk in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), re.S):
        t = blk.group(0)
        meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", t).group(1)) for k in
                                                         ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")}
    assert len(meta) == 5, sorted(meta)
    return meta


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_kernels_use_no_scratch_up_to_four_dimensions(tmp_path, d):
    for name, m in sorted(_kernel_resources(tmp_path, SC.SRC_QUAD_TENSOR, d).items()):
        print(d, name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 8192, (name, m)                      # the math tables only: the eigenvectors are registers


def test_kernel_resources_at_eight_dimensions(tmp_path):
    """recorded, not gated (profiles/softabs.txt): the eigenvectors of D >= 5 live in LDS (D^2 doubles for each of 256 lanes beside the 8 KB of math tables)"""
    for name, m in sorted(_kernel_resources(tmp_path, SC.SRC_QUAD_TENSOR, 8).items()):
        print(8, name, m)
        assert 8192 + 8 * 8 * 256 * 8 <= m["group_segment_fixed_size"] <= 160 * 1024, (name, m)     # (the compiler may add a promoted array of its own)


# ---------------------------------------------------------------- goldens
@pytest.mark.parametrize("fname", ["softabs_banana", "softabs_doublewell_d8", "softabs_diag_d4"])
def test_reference_reproduces_the_goldens(fname):
    spec = importlib.util.spec_from_file_location("make_golden_softabs", ROOT / "tests" / "golden" / "make_golden_softabs.py")
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    g = np.load(ROOT / "tests" / "golden" / f"{fname}.npz")
    out = mg.run_case(mg.GOLDEN[fname])
    for k in ("x0", "accept", "X", "LT", "G", "step"):
        assert np.array_equal(out[k], g[k]), f"{fname}: {k} differs from the golden"
