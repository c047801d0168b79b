"""The AM sampler without a GPU: the CPU reference (oracle/klara_oracle.c ko_am) against the literal NumPy restatement of the Julia source
(tests/am_mirror.py), deviation A1 case by case, the fallback of A2 / A3, the descriptor mapping and refusals of the C ABI, the Python API, the
Julia binding's mapping, a run of the reference under the host sanitizers, and whether the sampler learns its target's covariance."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import am_cases as AC
import am_ref as AR
import cases
import klara_jl_amd as K
import oracle_ffi as O
import smmala_cases as SC
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent

# Relative bounds, max |a - a_ref| / max |a_ref| per chain, between oracle/klara_oracle.c ko_am and the literal restatement over the cases of AC.ALL, 8 chains each:
# twice the largest difference measured.  The covariance: 3.04e-14 measured (swiss_example: 30 adaptive transitions of a recursion whose every step
# rounds three rank-one updates in the same order on both sides, but from states that the two sides' factorisations and products L z have moved apart by
# an ulp or two); RAM's comparable figure is 2.4e-14.  The running means: 1.07e-14 measured (swiss_example).
C_RTOL = 6.0e-14
M_RTOL = 2.1e-14


def _rel(a, b):
    return max(np.max(np.abs(a[i] - b[i])) / np.max(np.abs(b[i])) for i in range(len(b)))


@pytest.mark.parametrize("name", AC.ALL)
def test_reference_matches_literal_restatement(name):
    """accept masks identical, X / LT to 1e-10, C to C_RTOL and the means to M_RTOL (measured maxima beside the bounds); the restatement's two proposal
    log-densities are the same bits at every transition beyond t0 (A1), and taking them into the ratio changes no accept flag"""
    case = AC.make(name)
    n = 8
    job = AC.ref_job(case, nchains=n)
    assert job.set_state(case["x0"][:n]) == 0
    assert job.run(case["nsteps"]) == 0
    chains = AC.mirror_chains(case, nchains=n)
    for c in chains:
        c.run(case["nsteps"])
    rows = np.array([c.accepts for c in chains], dtype=np.uint8).T
    assert np.array_equal(job.accept, rows), "accept masks differ between the C reference and the NumPy restatement"
    np.testing.assert_allclose(job.X, np.array([c.x for c in chains]), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.LT, [c.lt for c in chains], rtol=1e-10, atol=1e-10)
    assert 0 < job.accept.mean() < 1, "a case that never (or always) accepts tests nothing"
    assert case["nsteps"] > case["am_t0"] + 1 and case["am_t0"] >= 2, "transitions before, at and after t0"
    crel = _rel(job.C, np.array([c.C for c in chains]))
    mrel = max(_rel(job.lastmean, np.array([c.lastmean for c in chains])), _rel(job.secondlastmean, np.array([c.secondlastmean for c in chains])))
    print(f"{name}: covariance differs from the literal restatement by {crel:.3e}, the means by {mrel:.3e} (relative)")
    assert crel <= C_RTOL and mrel <= M_RTOL
    assert job.fallbacks == 0
    # A1: q(x -> x') and q(x' -> x) are one number ...
    for c in chains:
        assert len(c.q) == case["nsteps"] - case["am_t0"]
        assert all(a == b for a, b in c.q), "the two proposal log-densities differ"
        assert all(np.isfinite(a) for a, _ in c.q)
    # ... and (r - q) + q decides every accept test as r does (a flag that ever differs here is a tie within 4 ulp of |q|: show that, then change
    # that case's seed with a comment — never exclude it)
    plain = np.array([c.plain_accepts for c in chains], dtype=np.uint8).T
    assert int((plain != rows).sum()) == 0, f"A1 changes {(plain != rows).sum()} accept flags"


def test_selector_is_the_unused_half_of_the_accept_block():
    """the reference's selector (detmath.h: kd_uniform_zw of block slot ceil(D / 2)) is the restatement's (the oracle's ko_stream_block, words z and w),
    strictly inside (0, 1); c = 0 therefore always picks the core component (w1 = 1.0)"""
    import am_mirror as AMM
    lib = O.load()
    us = []
    for d in range(1, 9):
        for chain in (0, 5, 1 << 33):
            for t in (0, 1, 77):
                u = lib.ko_am_selector(20260927, chain, t, d)
                assert u == AMM.selector(20260927, chain, t, d)
                us.append(u)
    assert 0.0 < min(us) and max(us) < 1.0 and len(set(us)) == 4 * 9         # (D = 2 j - 1 and 2 j share block slot j)


def test_covariance_update_is_the_empirical_covariance_recursion():
    """ko_am_covariance on exact data: with C = cov(x_1 .. x_k) (k >= 2 samples, normalised by k - 1), lastmean and secondlastmean the means of k + 1 and k
    values as iterate/AM.jl keeps them, the update gives the reference's formula entry for entry (formed here in NumPy with the full matrix)"""
    lib = O.load()
    rng = np.random.default_rng(5)
    for d in (1, 3, 8):
        for k in (1, 2, 7):
            x, m, m2 = rng.standard_normal(d), rng.standard_normal(d), rng.standard_normal(d)
            A = rng.standard_normal((d, d)); C0 = A @ A.T
            P = AR.pack(C0[None])[0].copy()
            lib.ko_am_covariance(d, k, x.ctypes.data, m.ctypes.data, m2.ctypes.data, P.ctypes.data)
            want = ((k - 1) * C0 + np.outer(x, x) + np.outer(-(k + 1) * m, m) + np.outer(k * m2, m2)) / k
            got = AR.unpack(P[None], d)[0]
            assert np.array_equal(np.triu(got), np.triu(want)), (d, k)


def test_factor_is_the_cholesky_factor_or_refuses():
    lib = O.load()
    rng = np.random.default_rng(6)
    for d in (1, 2, 5, 8):
        A = rng.standard_normal((d, d)); Cm = A @ A.T + 0.1 * np.eye(d)
        out = np.zeros(d * (d + 1) // 2)
        assert lib.ko_am_factor(d, 1.7, AR.pack(Cm[None])[0].ctypes.data, out.ctypes.data) == 1
        Lf = np.tril(AR.unpack(out[None], d)[0])
        np.testing.assert_allclose(Lf, np.linalg.cholesky(1.7 * Cm), rtol=1e-12, atol=1e-14)
    for bad in (np.zeros((3, 3)), -np.eye(3), np.full((3, 3), np.nan), np.diag([1.0, np.inf, 1.0]), np.ones((3, 3))):
        out = np.zeros(6)
        assert lib.ko_am_factor(3, 1.0, AR.pack(bad[None])[0].ctypes.data, out.ctypes.data) == 0


def test_t0_2_falls_back_until_the_samples_span_the_space():
    """A2 / A3 on the t0 = 2, D = 3 case.  At its third transition k - 1 = 0 wipes C0 and C = (x1 - x2)(x1 - x2)' / 2 has rank <= 1.

    What holds exactly: no chain falls back before the third transition; a chain whose second transition was rejected has C = 0 bit for bit there
    (x x' - 2 m m' + m2 m2' with x = m = m2), falls back, and the restatement's factorisation raises at that transition; every other chain's C is the
    rank-one matrix to rounding.  The issue expected a fallback at the third transition for EVERY chain and the restatement to raise there; in floating
    point neither side does: the second and third pivots of a rank-one matrix formed from three rounded rank-one updates are rounding noise of either
    sign, and a chain whose noise happens to be positive factors.  Measured on this case: 92 of 100 chains fall back at the third transition on the
    reference; the restatement raises at the third transition for 92 chains, at the fourth for 6, at the fifth for 1 and never for 1.  A chain factors
    with two noise pivots positive, which no more than half the chains can be expected to: more than half must fall back.  The fallbacks go on
    afterwards (82, 76, 59, ... per transition), the last one is at transition 26 of 40, and every state and covariance stays finite."""
    case = AC.make(AC.FALLBACK)
    n, nsteps = case["nchains"], case["nsteps"]
    assert case["am_t0"] == 2 and case["target"].ndims == 3
    job = AC.ref_job(case)
    assert job.set_state(case["x0"]) == 0
    per_step, prev = [], 0
    states = [job.X.copy()]
    C3 = None
    for t in range(nsteps):
        before = job.C.copy()
        assert job.run(1) == 0
        per_step.append(job.fallbacks - prev); prev = job.fallbacks
        states.append(job.X.copy())
        if t == 2:
            C3 = job.C.copy()
        if t < 2:
            assert np.array_equal(job.C, before), "C moved before t0"
    per_step = np.array(per_step)
    print("fallbacks per transition:", per_step.tolist())
    assert per_step[0] == per_step[1] == 0
    stuck = np.all(states[1] == states[2], axis=1)                       # the second transition was rejected
    d = states[1] - states[2]
    want = 0.5 * d[:, :, None] * d[:, None, :]
    assert np.array_equal(C3[stuck], np.zeros((int(stuck.sum()), 3, 3))) and stuck.sum() > 0
    scale = np.max(np.abs(states[1]), axis=1) ** 2 + np.max(np.abs(states[2]), axis=1) ** 2
    assert np.max(np.abs(C3 - want) / scale[:, None, None]) < 1e-14
    assert n // 2 < per_step[2] <= n and per_step[2] >= stuck.sum()
    assert per_step[3:].sum() > 0, "no fallback after the third transition"
    last = int(np.max(np.nonzero(per_step)[0]))
    assert last < nsteps - 5, "the fallbacks did not stop within the run"
    assert np.all(np.isfinite(job.X)) and np.all(np.isfinite(job.C)) and np.all(np.isfinite(job.lastmean)) and np.all(np.isfinite(job.LT))
    assert np.all(np.linalg.eigvalsh(job.C) > 0), "a chain's covariance is not positive definite at the end of the run"
    assert 0 < job.accept.mean() < 1
    # the restatement: a chain with C = 0 raises at the third transition; no chain raises before it
    raised = []
    for c in AC.mirror_chains(case):
        try:
            c.run(nsteps); raised.append(0)
        except np.linalg.LinAlgError:
            raised.append(c.count)
    raised = np.array(raised)
    print("the restatement raises at transition:", {int(k): int((raised == k).sum()) for k in np.unique(raised)})
    assert np.all(raised[stuck] == 3) and np.all((raised == 0) | (raised >= 3)) and (raised == 3).sum() > n // 2


def _status(**over):
    X, y = cases.swiss_data()
    kw = dict(sampler=L.SAMPLER_AM, target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=20, am_C0=np.eye(4), am_corescale=1.0, am_minorscale=1.0, am_c=0.05, am_t0=10)
    kw.update(over)
    if "target" in over and "am_C0" not in over and kw["sampler"] == L.SAMPLER_AM:
        kw["am_C0"] = np.eye(kw["target"].ndims)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


NOT_AM = dict(am_C0=None, am_corescale=0.0, am_minorscale=0.0, am_c=0.0, am_t0=0)


def test_create_maps_and_refuses_like_the_issue_says(klib, monkeypatch):
    assert L.SAMPLER_AM == 8
    ok = (0, L.ERR_HIP)                                               # (without a GPU an accepted job gets as far as the device)
    assert _status() in ok
    assert _status(verbose=True, period=5) in ok
    assert _status(monitor=L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT) in ok
    assert _status(am_C0=np.array([[1.0, 0.5, 0.0, 0.0], [np.nan, 1.0, 0.1, 0.0], [np.nan, np.nan, 2.0, 0.3], [np.nan, np.nan, np.nan, 1.0]])) in ok     # (the upper triangle is read)
    for d, n in ((1, 50), (3, 50), (8, 200), (3, 40)):               # kinds 2 (row split) and 0
        X, y = cases.synthetic_logit(n, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) in ok
    # user-defined whole-vector closures, plain and likelihood + prior form; the autodiff marker is tolerated as for MH
    assert _status(target=SC.quad_target(0.5, np.eye(3), np.eye(3))) in ok
    assert _status(target=AC.make("likprior_d5")["target"]) in ok
    assert _status(target=K.CustomTarget(8, cases.SRC_NEGDOT)) in ok
    import autodiff_cases as ADC
    assert _status(target=ADC.target(ADC.AD_BANANA, 2, np.array([100.0]))) in ok
    # AM.jl:138-143, and A5: c in [0, 1)
    bad = np.eye(4); bad[1, 2] = np.inf
    assert _status(am_C0=bad) == L.ERR_INVALID_ARG
    assert _status(am_C0=None) == L.ERR_INVALID_ARG
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert _status(am_corescale=v) == L.ERR_INVALID_ARG
        assert _status(am_minorscale=v) == L.ERR_INVALID_ARG
    for v in (-0.01, 1.0, 1.5, float("nan")):
        assert _status(am_c=v) == L.ERR_INVALID_ARG
    assert _status(am_c=0.0) in ok and _status(am_c=0.999) in ok
    for v in (0, -3):
        assert _status(am_t0=v) == L.ERR_INVALID_ARG
    # A3: t0 = 1 makes k = 0; t0 = 2 is accepted
    assert _status(am_t0=1) == L.ERR_UNSUPPORTED
    assert _status(am_t0=2) in ok
    # the five fields belong to AM alone
    mh = dict(sampler=L.SAMPLER_MH, mh_sigma=np.ones(4))
    assert _status(**mh, **NOT_AM) in ok
    for k, v in (("am_C0", np.eye(4)), ("am_corescale", 1.0), ("am_minorscale", 1.0), ("am_c", 0.05), ("am_t0", 10)):
        assert _status(**mh, **{**NOT_AM, k: v}) == L.ERR_INVALID_ARG, k
    assert _status(sampler=L.SAMPLER_RAM, ram_S0=np.eye(4), ram_targetrate=0.234, ram_gamma=0.7, **{**NOT_AM, "am_t0": 10}) == L.ERR_INVALID_ARG
    # any tuner but VanillaMCTuner, and the pooled tuner mode
    assert _status(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5) == L.ERR_UNSUPPORTED
    assert _status(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.6, da_nadapt=10) == L.ERR_UNSUPPORTED
    assert _status(tuner_mode=L.TUNE_POOLED) == L.ERR_UNSUPPORTED
    # D >= 9 (also where the logistic job would go to the matrix cores), the Gaussian and hierarchical families, pair closures
    for d in (9, 16, 20):
        X, y = cases.synthetic_logit(60, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDiagTarget.negdot(4)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDenseTarget(np.eye(4))) == L.ERR_UNSUPPORTED
    assert _status(target=cases.rats_target()) == L.ERR_UNSUPPORTED
    assert _status(target=SC.quad_target(0.5, np.eye(9), np.eye(9))) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT)) == L.ERR_UNSUPPORTED
    # more than one lane per chain
    monkeypatch.setenv("KLARA_CUSTOM_LANES", "4")
    assert _status(target=SC.quad_target(0.5, np.eye(3), np.eye(3))) == L.ERR_UNSUPPORTED
    monkeypatch.delenv("KLARA_CUSTOM_LANES")
    # 5 and 7 stay reserved
    for s in (5, 7, 9):
        assert _status(sampler=s, **NOT_AM) == L.ERR_INVALID_ARG
    # the getter needs a handle
    assert klib.klara_get_am_state(None, None, None, None, None) == L.ERR_INVALID_ARG


def test_descriptor_layout_and_exports(klib):
    """the five fields sit between smmala_softabs and ram_S0, 8 bytes each; the header, the ctypes mirror and the Julia struct list them in one order;
    the ABI version and the frozen stream's known answers are as they were"""
    names = [f[0] for f in L.KlaraDesc._fields_]
    i = names.index("smmala_softabs")
    assert names[i + 1:i + 7] == ["am_C0", "am_corescale", "am_minorscale", "am_c", "am_t0", "ram_S0"]
    for k in names[i + 1:i + 6]:
        assert getattr(L.KlaraDesc, k).size == 8
    assert L.KlaraDesc.am_C0.offset == L.KlaraDesc.smmala_softabs.offset + 8 and L.KlaraDesc.ram_S0.offset == L.KlaraDesc.am_C0.offset + 40
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    body = hdr[hdr.index("typedef struct klara_desc"):hdr.index("} klara_desc;")]
    order = [m.start() for m in (re.search(rf"\b{k}\s*;", body) for k in ["smmala_softabs", "am_C0", "am_corescale", "am_minorscale", "am_c", "am_t0", "ram_S0"])]
    assert order == sorted(order)
    assert re.search(r"KLARA_SAMPLER_AM\s*=\s*8", hdr) and re.search(r"#define\s+KLARA_ABI_VERSION\s+6\b", hdr) and L.KLARA_ABI_VERSION == 6
    assert klib.klara_abi_version() == 6
    assert "klara_get_am_state" in L.EXPORTS and hasattr(klib, "klara_get_am_state")
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert "am_C0::Ptr{Float64}; am_corescale::Float64; am_minorscale::Float64; am_c::Float64; am_t0::Int64\n    ram_S0::Ptr{Float64}" in jl


def test_check_custom_target_for_am(klib):
    """klara_check_custom_target(src, KLARA_SAMPLER_AM, D) compiles the AM kernels of a user's target (no GPU needed)"""
    import ram_cases as RC

    def check(src, d, sampler=L.SAMPLER_AM):
        return klib.klara_check_custom_target(src.encode(), sampler, d)
    assert check(SC.SRC_QUAD_TENSOR, 3) == 0, klib.klara_compile_log()
    assert check(SC.SRC_QUAD_TENSOR, 8) == 0, klib.klara_compile_log()
    assert check(cases.SRC_BANANA_LT_ONLY, 2) == 0                    # no gradient closure is needed
    assert check(RC.SRC_HALFSPACE, 2) == 0, klib.klara_compile_log()
    assert check(AC.make("likprior_d5")["target"].source, 5) == 0, klib.klara_compile_log()
    assert check(SC.SRC_QUAD_TENSOR, 9) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT).source, 4) == L.ERR_UNSUPPORTED
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=7) == L.ERR_INVALID_ARG
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=9) == L.ERR_INVALID_ARG
    K.CustomTarget(3, SC.SRC_QUAD_TENSOR).check(L.SAMPLER_AM)


def test_python_api_mirrors_the_reference_constructors():
    s = K.AM(np.eye(2))                                               # AM(C0::Matrix; corescale=1., minorscale=1., c=0.05, t0=10)
    assert s.kind == L.SAMPLER_AM and np.array_equal(s.C0, np.eye(2)) and (s.corescale, s.minorscale, s.c, s.t0) == (1.0, 1.0, 0.05, 10)
    assert np.array_equal(K.AM(np.array([1.0, 2.0, 3.0])).C0, np.diag([1.0, 2.0, 3.0]))       # AM(C0::Vector): diagm(C0)
    assert np.array_equal(K.AM(0.5, 3).C0, 0.5 * np.eye(3)) and np.array_equal(K.AM(2.0).C0, [[2.0]])      # AM(C0::Real, d=1): fill(C0, d)
    M = np.array([[1.0, 0.3], [0.3, 2.0]])
    s = K.AM(M, corescale=2.0, minorscale=0.1, c=0.0, t0=1)           # (the reference's assertion is t0 > 0; the library refuses t0 = 1)
    assert np.array_equal(s.C0, M) and (s.corescale, s.minorscale, s.c, s.t0) == (2.0, 0.1, 0.0, 1)
    with pytest.raises(AssertionError, match=re.escape("Constant corescale must be positive, got 0.0")):
        K.AM(np.eye(2), corescale=0.0)
    with pytest.raises(AssertionError, match=re.escape("Constant minorscale must be positive, got -1.0")):
        K.AM(np.eye(2), minorscale=-1.0)
    with pytest.raises(AssertionError, match="Constant c must be non-negative"):
        K.AM(np.eye(2), c=-0.1)
    with pytest.raises(AssertionError, match="t0 is not positive"):
        K.AM(np.eye(2), t0=0)
    with pytest.raises(ValueError):
        K.AM(np.ones((2, 3)))


def test_basic_mc_job_maps_am_to_the_descriptor(monkeypatch):
    import klara_jl_amd.api as A
    seen = {}

    class FakeEngine:
        def __init__(self, **kw):
            seen.update(kw)

        def set_state(self, x):
            pass

    monkeypatch.setattr(A, "Engine", FakeEngine)
    X, y = cases.swiss_data()
    p = K.BasicContMuvParameter("p", logtarget=K.LogisticTarget(X, y, 100.0))
    K.BasicMCJob(K.likelihood_model(p), K.AM(np.ones(4), corescale=1.4, c=0.1, t0=20), K.BasicMCRange(nsteps=50, burnin=10), {"p": AC.SWISS_X0},
                 tuner=K.VanillaMCTuner(verbose=True))
    assert seen["sampler"] == L.SAMPLER_AM and np.array_equal(seen["am_C0"], np.eye(4))
    assert (seen["am_corescale"], seen["am_minorscale"], seen["am_c"], seen["am_t0"]) == (1.4, 1.0, 0.1, 20)
    assert seen["tuner"] == L.TUNER_VANILLA and seen["verbose"] and "mh_sigma" not in seen and "ram_S0" not in seen
    with pytest.raises(NotImplementedError):
        K.BasicMCJob(K.likelihood_model(p), K.AM(np.ones(4)), K.BasicMCRange(nsteps=50, burnin=10), {"p": AC.SWISS_X0}, tuner=K.AcceptanceRateMCTuner(0.3))


def test_julia_binding_maps_am():
    """mechanical check of julia/KlaraHIP: AM is Klara's own (imported, not exported), mapped to SAMPLER_AM with C0, corescale, minorscale, c and t0, and
    amstate is exported — a name Klara does not export"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"const\s+SAMPLER_AM\s*=\s*Int32\(8\)", src)
    assert re.search(r"import\s+Klara:[^\n]*\bAM\b", src)
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    names = {t for t in re.split(r"[,\s]+", export) if t}
    assert "amstate" in names and "AM" not in names
    klara = set((ROOT / "tests" / "golden" / "klara_exports.txt").read_text().split())
    assert "AM" in klara and "amstate" not in klara
    m = re.search(r"isa\(sampler,\s*AM\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S)
    assert m, "no AM branch in the sampler mapping"
    body = m.group(1)
    assert "samplers/AM.jl:131-136" in body
    for f in ("SAMPLER_AM", "sampler.C0", "sampler.corescale", "sampler.minorscale", "sampler.c", "sampler.t0"):
        assert f in body, f
    assert re.search(r"^function amstate\(job::HIPMCJob\)", src, re.M) and "klara_get_am_state" in src


def test_reference_runs_clean_under_the_host_sanitizers():
    """oracle/klara_oracle.c with the main of tests/am_sanitizer_main.c (one small t0 = 2 job, so that the fallback path runs), built with -fsanitize=address,undefined and run as a
    stand-alone program: no report, exit status 0"""
    exe = AR.sanitizer_program()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "am_ref main: status 0" in r.stdout and "finite 1" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr


# Relative Frobenius error of the chain-mean of C against the target's covariance, || mean_c C - Sigma ||_F / || Sigma ||_F: 2 x the 0.0130 measured on the
# reference with the job below (256 chains, 2,000 transitions).  At the start, C0 = I against this Sigma, it is 1.07.
LEARN_TOL = 0.026


def test_am_learns_the_target_covariance():
    """the reference on N(0, P^-1), D = 3, condition number 10, 256 chains started in equilibrium, AM(eye(3); corescale = 2.38^2 / 3, minorscale = 0.01,
    c = 0.05, t0 = 10), 2,000 transitions: the mean over the chains of C is the target's covariance to LEARN_TOL (measured 0.0130); no fallback.  The
    device is held to this reference bit for bit (tests/test_gpu_am.py), so this needs no GPU."""
    d, n, steps = 3, 256, 2000
    P = AC.conditioned_precision(d, 10.0, seed=3)
    Sigma = np.linalg.inv(P)
    x0 = np.random.default_rng(103).standard_normal((n, d)) @ np.linalg.cholesky(Sigma).T
    case = dict(target=AC.quad_target(0.5, P, P), nchains=n, nsteps=steps, am_C0=np.eye(d), x0=x0, seed=9003, **AC.am(d, 10))
    job = AC.ref_job(case)
    job.want_accept = False
    assert job.set_state(x0) == 0 and job.run(steps) == 0
    err = np.linalg.norm(job.C.mean(axis=0) - Sigma) / np.linalg.norm(Sigma)
    start = np.linalg.norm(np.eye(d) - Sigma) / np.linalg.norm(Sigma)
    rate = float(job.naccept.mean()) / steps
    print(f"chain-mean of C against Sigma: relative error {err:.4f} (start {start:.2f}), acceptance {rate:.3f}, fallbacks {job.fallbacks}")
    assert err <= LEARN_TOL and start > 1.0
    assert job.fallbacks == 0 and 0.1 < rate < 0.6
