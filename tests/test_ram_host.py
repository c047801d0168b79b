"""The RAM sampler without a GPU: the CPU reference (oracle/klara_oracle.c ko_ram) against the literal NumPy restatement of the Julia source
(tests/ram_mirror.py), the algebra of the factor update, the descriptor mapping and refusals of the C ABI, the Python API and the Julia
binding's mapping."""
import re
from pathlib import Path

import numpy as np
import pytest

import cases
import klara_jl_amd as K
import oracle_ffi as O
import ram_cases as RC
import ram_ref as RR
import smmala_cases as SC
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent

# Relative bound on a factor, max |S - S_ref| / max |S_ref| per chain: 100 x the largest difference measured between oracle/klara_oracle.c ko_ram (R1-R4) and the
# literal restatement over the cases below (2.4e-14, swiss_example: 40 transitions of a recursion whose every step rounds a 4 x 4 product and
# factorisation differently in the two); the margin covers R1 / R2's reordering, not an algorithmic difference
S_RTOL = 2.4e-12


def _srel(a, b):
    return max(np.max(np.abs(a[i] - b[i])) / np.max(np.abs(b[i])) for i in range(len(b)))


@pytest.mark.parametrize("name", RC.ALL)
def test_reference_matches_literal_restatement(name):
    """accept masks identical, X / LT to 1e-10, the factors to S_RTOL (measured: at most 2.4e-14 over these cases, 8 chains each)"""
    case = RC.make(name)
    n = 8
    job = RC.ref_job(case, nchains=n)
    assert job.set_state(case["x0"][:n]) == 0
    assert job.run(case["nsteps"]) == 0
    chains = RC.mirror_chains(case, nchains=n)
    for c in chains:
        c.run(case["nsteps"])
    rows = np.array([c.accepts for c in chains], dtype=np.uint8).T
    assert np.array_equal(job.accept, rows), "accept masks differ between the C reference and the NumPy restatement"
    np.testing.assert_allclose(job.X, np.array([c.x for c in chains]), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(job.LT, [c.lt for c in chains], rtol=1e-10, atol=1e-10)
    assert 0 < job.accept.mean() < 1, "a case that never (or always) accepts tests nothing"
    rel = _srel(job.S, np.array([c.S for c in chains]))
    print(f"{name}: factor differs from the literal restatement by {rel:.3e} (relative)")
    assert rel <= S_RTOL
    assert job.skipped == 0


@pytest.mark.parametrize("name", RC.ALL)
def test_factor_update_algebra(name):
    """after every step of the reference: S S' = S_prev (I + c z z') S_prev' (formed in NumPy), S lower triangular with a positive diagonal, the
    padded block the identity bit for bit, nothing skipped"""
    case = RC.make(name)
    job = RC.ref_job(case, nchains=1)
    assert job.set_state(case["x0"][:1]) == 0
    E, D = job.E, job.D
    for _ in range(case["nsteps"]):
        prev = job.S_padded[0]
        assert job.run(1) == 0
        z, c = job.last_draw()
        S = job.S_padded[0]
        want = prev @ (np.eye(E) + c * np.outer(z, z)) @ prev.T
        assert np.max(np.abs(S @ S.T - want)) <= S_RTOL * np.max(np.abs(want))
        assert np.array_equal(np.triu(S, 1), np.zeros((E, E))) and np.all(np.diag(S) > 0)
        assert np.array_equal(S[D:, :], np.eye(E)[D:, :]) and np.array_equal(S[:, D:], np.eye(E)[:, D:]), "padding is not the identity block"
        assert np.array_equal(z[D:], np.zeros(E - D))
        assert np.array_equal(job.S[0], S[:D, :D])
    assert job.skipped == 0


def test_update_is_skipped_where_it_cannot_be_factored():
    """R4: a non-finite c (what a non-finite z . z or ratio arithmetic would hand on), z . z = 0, or a c that makes I + c z z' indefinite: the factor
    stays as it was bit for bit and the update counts as skipped"""
    S = np.array([[0.9, 0.0, 0.0, 0.0], [0.3, 0.6, 0.0, 0.0], [-0.2, 0.25, 0.8, 0.0], [0.0, 0.0, 0.0, 1.0]])
    z = np.array([0.4, -1.3, 0.7, 0.0])
    w = S @ z
    for c, zz in ((np.nan, z @ z), (np.inf, z @ z), (-np.inf, z @ z), (0.1, 0.0), (0.1, np.nan), (-5.0, z @ z)):
        out, ok = RR.update_c(S, c, zz, w)
        assert ok == 0 and np.array_equal(out, S), (c, zz)
    out, ok = RR.update_c(S, 0.1, z @ z, w)
    assert ok == 1 and not np.array_equal(out, S)
    np.testing.assert_allclose(out @ out.T, S @ (np.eye(4) + 0.1 * np.outer(z, z)) @ S.T, rtol=1e-13, atol=1e-15)
    # ... and through the job: skipped counts it
    case = RC.make("gauss_d3")
    job = RC.ref_job(case, nchains=1)
    assert job.set_state(case["x0"][:1]) == 0
    job.desc.ram_targetrate = float("nan")                           # (not a valid descriptor: only to reach the skip)
    before = job.S.copy()
    assert job.run(1) == 0
    assert job.skipped == 1 and np.array_equal(job.S, before)


def test_proposal_outside_the_support_counts_as_acceptance_probability_zero():
    """R3: ratio = -inf gives min(1, exp(ratio)) = 0, as exp(-Inf) does in the reference; NaN too (where the reference's chol would throw)"""
    lib = O.load()
    want = lib.ko_ram_coef(2, 4, 0.7, 0.234, -1e300, 1.5)
    assert lib.ko_ram_coef(2, 4, 0.7, 0.234, -np.inf, 1.5) == want == min(1.0, 2 * 5 ** -0.7) * (0.0 - 0.234) / 1.5
    assert lib.ko_ram_coef(2, 4, 0.7, 0.234, np.nan, 1.5) == want
    assert lib.ko_ram_coef(2, 4, 0.7, 0.234, 3.0, 1.5) == lib.ko_ram_coef(2, 4, 0.7, 0.234, np.inf, 1.5) == lib.ko_ram_coef(2, 4, 0.7, 0.234, 0.0, 1.5)
    case = RC.make("halfspace_d2")
    job = RC.ref_job(case)
    assert job.set_state(case["x0"]) == 0
    assert job.run(case["nsteps"]) == 0
    assert np.all(job.X[:, 0] >= 0) and np.all(np.isfinite(job.S)) and job.skipped == 0


def _status(**over):
    X, y = cases.swiss_data()
    kw = dict(sampler=L.SAMPLER_RAM, target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=10, ram_S0=np.eye(4), ram_targetrate=0.234, ram_gamma=0.7)
    kw.update(over)
    if "target" in over and "ram_S0" not in over and kw["sampler"] == L.SAMPLER_RAM:
        kw["ram_S0"] = np.eye(kw["target"].ndims)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


def test_create_maps_and_refuses_like_the_issue_says(klib, monkeypatch):
    assert L.SAMPLER_RAM == 6
    ok = (0, L.ERR_HIP)                                               # (no GPU here: an accepted job gets as far as the device)
    assert _status() in ok
    assert _status(verbose=True, period=5) in ok
    assert _status(monitor=L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT) in ok
    assert _status(ram_S0=np.array([[1.0, 9.0, 9.0, 9.0], [0.5, 1.0, 9.0, 9.0], [0.0, 0.1, 2.0, 9.0], [0.0, 0.0, 0.3, 1.0]])) in ok     # (the lower triangle is read)
    for d, n in ((1, 50), (3, 50), (8, 200), (3, 40)):               # kinds 2 (row split) and 0
        X, y = cases.synthetic_logit(n, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) in ok
    # user-defined whole-vector closures, plain and likelihood + prior form; the autodiff marker is tolerated as for MH
    assert _status(target=SC.quad_target(0.5, np.eye(3), np.eye(3))) in ok
    assert _status(target=RC.make("likprior_d5")["target"]) in ok
    assert _status(target=K.CustomTarget(8, cases.SRC_NEGDOT)) in ok
    # RAM.jl:100-102
    bad = np.eye(4); bad[2, 2] = 0.0
    assert _status(ram_S0=bad) == L.ERR_INVALID_ARG
    bad = np.eye(4); bad[1, 1] = -1.0
    assert _status(ram_S0=bad) == L.ERR_INVALID_ARG
    assert _status(ram_S0=None) == L.ERR_INVALID_ARG
    for tr in (0.0, 1.0, -0.1, float("nan")):
        assert _status(ram_targetrate=tr) == L.ERR_INVALID_ARG
    for g in (0.5, 1.01, 0.0, float("nan")):
        assert _status(ram_gamma=g) == L.ERR_INVALID_ARG
    assert _status(ram_gamma=1.0) in ok
    # the three fields belong to RAM alone
    mh = dict(sampler=L.SAMPLER_MH, mh_sigma=np.ones(4))
    assert _status(**mh, ram_S0=None, ram_targetrate=0.0, ram_gamma=0.0) in ok
    assert _status(**mh, ram_S0=np.eye(4), ram_targetrate=0.0, ram_gamma=0.0) == L.ERR_INVALID_ARG
    assert _status(**mh, ram_S0=None, ram_targetrate=0.234, ram_gamma=0.0) == L.ERR_INVALID_ARG
    assert _status(**mh, ram_S0=None, ram_targetrate=0.0, ram_gamma=0.7) == L.ERR_INVALID_ARG
    # any tuner but VanillaMCTuner
    assert _status(tuner=L.TUNER_ACCEPT_RATE, targetrate=0.5) == L.ERR_UNSUPPORTED
    assert _status(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.6, da_nadapt=10) == L.ERR_UNSUPPORTED
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
    # 5 stays reserved
    assert _status(sampler=5, ram_S0=None, ram_targetrate=0.0, ram_gamma=0.0) == L.ERR_INVALID_ARG
    # the getter and the setter need a handle
    assert klib.klara_get_ram_factor(None, None, None) == L.ERR_INVALID_ARG and klib.klara_set_ram_factor(None, None) == L.ERR_INVALID_ARG


def test_check_custom_target_for_ram(klib):
    """klara_check_custom_target(src, KLARA_SAMPLER_RAM, D) compiles the RAM kernels of a user's target (no GPU needed)"""
    def check(src, d, sampler=L.SAMPLER_RAM):
        return klib.klara_check_custom_target(src.encode(), sampler, d)
    assert check(SC.SRC_QUAD_TENSOR, 3) == 0, klib.klara_compile_log()
    assert check(SC.SRC_QUAD_TENSOR, 8) == 0, klib.klara_compile_log()
    assert check(cases.SRC_BANANA_LT_ONLY, 2) == 0                    # no gradient closure is needed
    assert check(RC.SRC_HALFSPACE, 2) == 0, klib.klara_compile_log()
    assert check(RC.make("likprior_d5")["target"].source, 5) == 0, klib.klara_compile_log()
    assert check(SC.SRC_QUAD_TENSOR, 9) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT).source, 4) == L.ERR_UNSUPPORTED
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=5) == L.ERR_INVALID_ARG
    assert check(SC.SRC_QUAD_TENSOR, 3, sampler=7) == L.ERR_INVALID_ARG
    K.CustomTarget(3, SC.SRC_QUAD_TENSOR).check(L.SAMPLER_RAM)


def test_python_api_mirrors_the_reference_constructors():
    s = K.RAM()                                                       # RAM(S0=1., n=1)
    assert s.kind == L.SAMPLER_RAM and np.array_equal(s.S0, [[1.0]]) and s.targetrate == 0.234 and s.gamma == 0.7
    assert np.array_equal(K.RAM(0.5, 3).S0, 0.5 * np.eye(3))
    assert np.array_equal(K.RAM(np.ones(4)).S0, np.eye(4))            # RAM(S0::Vector): diagm(S0)
    M = np.array([[1.0, 7.0], [0.5, 2.0]])
    assert np.array_equal(K.RAM(M, targetrate=0.4, gamma=1.0).S0, [[1.0, 0.0], [0.5, 2.0]])      # RAM(S0::Matrix): RealLowerTriangular(S0)
    with pytest.raises(AssertionError, match="All diagonal elements of initial adaptation matrix must be positive"):
        K.RAM(np.array([1.0, 0.0]))
    with pytest.raises(AssertionError, match="Target acceptance rate should be between 0 and 1"):
        K.RAM(np.ones(2), targetrate=1.0)
    with pytest.raises(AssertionError, match="Exponent of stepsize must be greater than 0.5 and less or equal to 1"):
        K.RAM(np.ones(2), gamma=0.5)


def test_basic_mc_job_maps_ram_to_the_descriptor(monkeypatch):
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
    K.BasicMCJob(K.likelihood_model(p), K.RAM(np.ones(4), targetrate=0.3), K.BasicMCRange(nsteps=50, burnin=10), {"p": RC.SWISS_X0},
                 tuner=K.VanillaMCTuner(verbose=True))
    assert seen["sampler"] == L.SAMPLER_RAM and np.array_equal(seen["ram_S0"], np.eye(4))
    assert seen["ram_targetrate"] == 0.3 and seen["ram_gamma"] == 0.7
    assert seen["tuner"] == L.TUNER_VANILLA and seen["verbose"] and "mh_sigma" not in seen
    with pytest.raises(NotImplementedError):
        K.BasicMCJob(K.likelihood_model(p), K.RAM(np.ones(4)), K.BasicMCRange(nsteps=50, burnin=10), {"p": RC.SWISS_X0}, tuner=K.AcceptanceRateMCTuner(0.3))


def test_julia_binding_maps_ram():
    """mechanical check of julia/KlaraHIP: RAM is Klara's own (imported, not exported), mapped to SAMPLER_RAM with S0, targetrate and γ, and
    ramfactor is exported"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"const\s+SAMPLER_RAM\s*=\s*Int32\(6\)", src)
    assert re.search(r"import\s+Klara:[^\n]*\bRAM\b", src)
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    names = {t for t in re.split(r"[,\s]+", export) if t}
    assert "ramfactor" in names and "RAM" not in names
    m = re.search(r"isa\(sampler,\s*RAM\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S)
    assert m, "no RAM branch in the sampler mapping"
    body = m.group(1)
    assert "SAMPLER_RAM" in body and "sampler.S0" in body and "sampler.targetrate" in body and "sampler.γ" in body
    assert re.search(r"^function ramfactor\(job::HIPMCJob\)", src, re.M) and "klara_get_ram_factor" in src
    assert "ram_S0::Ptr{Float64}; ram_targetrate::Float64; ram_gamma::Float64" in src


@pytest.mark.parametrize("fname", ["ram_swiss", "ram_gauss_d3"])
def test_reference_reproduces_the_goldens(fname):
    """the committed vectors (tests/golden/make_golden_ram.py) still come out of the CPU reference bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_ram", ROOT / "tests" / "golden" / "make_golden_ram.py")
    mg = importlib.util.module_from_spec(spec); spec.loader.exec_module(mg)
    g = np.load(ROOT / "tests" / "golden" / f"{fname}.npz")
    out = mg.run_case(mg.GOLDEN[fname])
    for k in ("x0", "accept", "X", "LT", "S", "skipped"):
        assert np.array_equal(out[k], g[k]), f"{fname}: {k} differs from the golden"
