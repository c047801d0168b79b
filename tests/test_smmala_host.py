"""The SMMALA sampler without a GPU: the CPU reference (oracle/klara_oracle.c ko_smmala) against the NumPy restatement of the Julia source
(tests/smmala_mirror.py), the factor C = L^-T against the reference's chol(inv(G))', the descriptor mapping and refusals of the C ABI,
and the Julia binding's mapping."""
import re
from pathlib import Path

import numpy as np
import pytest

import cases
import klara_jl_amd as K
import smmala_cases as SC
import smmala_mirror as SM
import smmala_ref as SR
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent


def _ref_vs_mirror(case, nchains, nsteps, pooled=False):
    job = SC.ref_job(case, nchains=nchains)
    assert job.set_state(case["x0"][:nchains]) == 0
    assert job.run(nsteps) == 0
    chains = SC.mirror_chains(case, nchains=nchains)
    if pooled:
        rows = SM.run_pooled(chains, nsteps, tuner="rate" if case.get("tuner") == L.TUNER_ACCEPT_RATE else "vanilla",
                             targetrate=case.get("targetrate"), period=case.get("period", 100), burnin=case.get("burnin", 0),
                             verbose=case.get("verbose", False))
    else:
        for c in chains:
            c.run(nsteps)
        rows = np.array([c.accepts for c in chains], dtype=np.uint8).T
    assert np.array_equal(job.accept, rows), "accept masks differ between the C reference and the NumPy restatement"
    xm = np.array([c.x for c in chains])
    np.testing.assert_allclose(job.X, xm, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.LT, [c.lt for c in chains], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.G, np.array([c.g for c in chains]), rtol=1e-10, atol=1e-9)
    steps = job.step if not pooled else np.full(nchains, job.step[0])
    np.testing.assert_allclose(steps, [c.step for c in chains], rtol=1e-12)
    return job


@pytest.mark.parametrize("name", ["swiss_example", "logit_d1", "logit_d3", "logit_d8", "logit_d3_unsplit", "logit_d8_verbose",
                                  "custom_gauss_d3", "custom_gauss_d3_rate", "bivariate_example"])
def test_reference_matches_numpy_restatement(name):
    case = SC.make(name)
    job = _ref_vs_mirror(case, nchains=8, nsteps=case["nsteps"])
    assert 0 < job.accept.mean() < 1, "a case that never (or always) accepts tests nothing"


@pytest.mark.parametrize("name", ["swiss_pooled", "custom_gauss_d6_pooled"])
def test_reference_matches_numpy_restatement_pooled(name):
    case = SC.make(name)
    _ref_vs_mirror(case, nchains=12, nsteps=case["nsteps"], pooled=True)


def test_reference_metric_is_the_example_tensor():
    """the metric the kernels accumulate row by row is ptensorlogtarget of swiss/SMMALA/analytical.jl:20-23"""
    case = SC.make("swiss_example")
    job = SC.ref_job(case, nchains=2)
    t = case["target"]
    for x in (SC.SWISS_X0, np.zeros(4), np.array([0.3, -1.2, 2.0, 0.1])):
        G = job.metric(x) + np.eye(4) / t.lam
        np.testing.assert_allclose(G, SM.logistic_tensor(t.X, t.lam)(x), rtol=1e-12, atol=1e-14)


def test_inverse_transposed_factor_is_a_root_of_the_inverse_metric():
    """SMMALA deviation 1: C = L^-T (G = L L') in place of the reference's chol(inv(G))' — the same C C' = inv(G)"""
    rng = np.random.default_rng(7)
    for k in range(100):
        d = 1 + k % 8
        A = rng.standard_normal((d, d))
        G = A @ A.T + (0.05 + rng.random()) * np.eye(d)
        C, ok = SR.inv_chol_t(G)
        assert ok
        assert np.allclose(np.triu(C), C), "L^-T is upper triangular"
        inv = np.linalg.inv(G)
        Kr = np.linalg.cholesky(inv)                         # chol(Hermitian(inv(G)))' of iterate/SMMALA.jl:171: lower
        scale = np.max(np.abs(inv))
        # 1e-12 relative to the largest entry of inv(G), widened by cond(G) / 100 where that exceeds 1: the triangular solves lose
        # ~log10(cond) digits (forward error ~ cond * eps), and so does numpy's own inverse the result is compared with — a bound that
        # ignored the conditioning would test numpy's rounding as much as the factor (cond reaches ~1e4 among these matrices)
        assert np.max(np.abs(C @ C.T - inv)) <= 1e-12 * scale * max(1.0, np.linalg.cond(G) / 1e2)
        assert np.max(np.abs(C @ C.T - Kr @ Kr.T)) <= 1e-12 * scale * max(1.0, np.linalg.cond(G) / 1e2)
    # a matrix that is not positive definite does not factor (deviation 4)
    _, ok = SR.inv_chol_t(np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert not ok


def test_reference_rejects_a_start_state_without_a_positive_definite_metric():
    """deviation 5: klara_set_state returns KLARA_ERR_NONFINITE_INIT; the reference does the same (a negative prior variance makes
    X' W X - I/|lambda| indefinite near the mode)"""
    X, y = cases.synthetic_logit(80, 3, seed=2)
    case = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 25.0), nchains=3, nsteps=5, driftstep=0.5, x0=np.zeros((3, 3)))
    job = SC.ref_job(case)
    assert job.set_state(case["x0"]) == 0
    bad = dict(case)
    job2 = SC.ref_job(bad)
    job2.desc.logit_lambda = -1e-3                                    # (not a valid descriptor: only to reach the metric check)
    assert job2.set_state(np.zeros((3, 3))) == L.ERR_NONFINITE_INIT


def _status(**over):
    X, y = cases.swiss_data()
    kw = dict(sampler=L.SAMPLER_SMMALA, target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=10, driftstep=0.1)
    kw.update(over)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


def test_create_maps_and_refuses_like_the_issue_says(klib):
    assert L.SAMPLER_SMMALA == 4
    assert _status() in (0, L.ERR_HIP)
    assert _status(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5) in (0, L.ERR_HIP)
    assert _status(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5, tuner_mode=L.TUNE_POOLED) in (0, L.ERR_HIP)
    assert _status(monitor=L.MON_HIST_GRAD | L.MON_HISTORY | L.MON_HIST_LT) in (0, L.ERR_HIP)
    for d in (1, 3, 8):
        X, y = cases.synthetic_logit(50, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) in (0, L.ERR_HIP)
    # SMMALA.jl:132 "Drift step is not positive"
    assert _status(driftstep=0.0) == L.ERR_INVALID_ARG
    assert _status(driftstep=-1.0) == L.ERR_INVALID_ARG
    # DualAveraging: the status MALA gets
    da = dict(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.6, da_nadapt=10)
    assert _status(**da) == L.ERR_UNSUPPORTED
    assert _status(sampler=L.SAMPLER_MALA, **da) == L.ERR_UNSUPPORTED
    # refused: D >= 9 (also the matrix-core layout beyond 16), the Gaussian / hierarchical / user-defined families
    for d in (9, 16, 20):
        X, y = cases.synthetic_logit(60, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDiagTarget.negdot(4)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDenseTarget(np.eye(4))) == L.ERR_UNSUPPORTED
    assert _status(target=cases.rats_target()) == L.ERR_UNSUPPORTED
    # a user-defined target: the plain whole-vector form with klara_user_tensorlogtarget; without the tensor the source does not compile
    # for SMMALA, the likelihood + prior form and pair closures are refused, and so is D >= 9
    assert _status(target=SC.quad_target(0.5, np.eye(3), np.eye(3))) in (0, L.ERR_HIP)
    assert _status(target=K.CustomTarget(2, cases.SRC_NEGDOT)) in (L.ERR_COMPILE, L.ERR_HIP)      # (compiled after the device check)
    assert _status(target=SC.quad_target(0.5, np.eye(9), np.eye(9))) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget(4, "#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + SC.SRC_QUAD_TENSOR)) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget(4, "#define KLARA_USER_PAIR_TARGET 1\n" + SC.SRC_QUAD_TENSOR)) == L.ERR_UNSUPPORTED
    # no new sampler beyond SMMALA
    assert _status(sampler=5) == L.ERR_INVALID_ARG


def test_python_api_mirrors_the_reference_constructor():
    s = K.SMMALA()
    assert s.driftstep == 1.0 and s.transform is None and s.kind == L.SAMPLER_SMMALA
    assert K.SMMALA(0.02).driftstep == 0.02
    with pytest.raises(AssertionError, match="Drift step is not positive"):
        K.SMMALA(0.0)
    with pytest.raises(NotImplementedError):
        K.SMMALA(1.25, lambda H: H)                                   # softabs & co. are not run on the device


def test_basic_mc_job_maps_smmala_to_the_descriptor(monkeypatch):
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
    K.BasicMCJob(K.likelihood_model(p), K.SMMALA(0.02), K.BasicMCRange(nsteps=50, burnin=10), {"p": SC.SWISS_X0},
                 tuner=K.AcceptanceRateMCTuner(0.5))
    assert seen["sampler"] == L.SAMPLER_SMMALA and seen["driftstep"] == 0.02
    assert seen["tuner"] == L.TUNER_ACCEPT_RATE and seen["targetrate"] == 0.5


def test_julia_binding_maps_smmala():
    """mechanical check of julia/KlaraHIP: SMMALA is imported from Klara, mapped to SAMPLER_SMMALA with its drift step, and a
    transform other than `nothing` is refused"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"const\s+SAMPLER_SMMALA\s*=\s*Int32\(4\)", src)
    assert re.search(r"import\s+Klara:.*\bSMMALA\b", src) or re.search(r"using\s+Klara:.*\bSMMALA\b", src)
    m = re.search(r"isa\(sampler,\s*SMMALA\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S)
    assert m, "no SMMALA branch in the sampler mapping"
    body = m.group(1)
    assert "SAMPLER_SMMALA" in body and "driftstep" in body and "transform" in body and "nothing" in body


def test_check_custom_target_for_smmala(klib):
    """klara_check_custom_target(src, KLARA_SAMPLER_SMMALA, D) compiles the SMMALA kernels of a user's target (no GPU needed) and rejects a
    source without klara_user_tensorlogtarget"""
    def check(src, d, sampler=L.SAMPLER_SMMALA):
        return klib.klara_check_custom_target(src.encode(), sampler, d)
    assert check(SC.SRC_QUAD_TENSOR, 3) == 0
    assert check(SC.SRC_QUAD_TENSOR, 8) == 0
    assert check(cases.SRC_NEGDOT, 3) == L.ERR_COMPILE
    assert b"klara_user_tensorlogtarget" in klib.klara_compile_log()
    assert check(SC.SRC_QUAD_TENSOR, 9) == L.ERR_UNSUPPORTED
    assert check("#define KLARA_USER_LIKELIHOOD_PRIOR 1\n" + SC.SRC_QUAD_TENSOR, 3) == L.ERR_UNSUPPORTED
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=5) == L.ERR_INVALID_ARG
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=L.SAMPLER_MALA) == 0          # (the other samplers ignore the tensor)
    t = K.CustomTarget(3, cases.SRC_NEGDOT)
    assert not t.has_tensor and SC.quad_target(0.5, np.eye(3), np.eye(3)).has_tensor
    with pytest.raises(K.KlaraError) as ei:
        t.check(L.SAMPLER_SMMALA)
    assert ei.value.status == L.ERR_COMPILE


@pytest.mark.parametrize("fname", ["smmala_swiss", "smmala_bivariate"])
def test_reference_reproduces_the_goldens(fname):
    """the committed vectors (tests/golden/make_golden_smmala.py) still come out of the CPU reference bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_smmala", ROOT / "tests" / "golden" / "make_golden_smmala.py")
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    g = np.load(ROOT / "tests" / "golden" / f"{fname}.npz")
    out = mg.run_case(mg.GOLDEN[fname])
    for k in ("x0", "accept", "X", "LT", "G", "step"):
        assert np.array_equal(out[k], g[k]), f"{fname}: {k} differs from the golden"
