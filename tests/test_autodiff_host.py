"""Forward-mode autodiff of user-defined targets (KLARA_USER_AUTODIFF, klara.jl_amd/csrc/klara_autodiff.h) without a GPU: the compile check and
its refusals, the host build of the header against analytic derivatives, the header's two invariants, and the Python / Julia host mapping."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import autodiff_cases as A
import autodiff_ref as R
import cases
import klara_jl_amd as K
import oracle_ffi as O
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
EPS = A.EPS
SOURCES = A.host_sources()
IDS = [s[0] for s in SOURCES]

MEASURED, MEASURED_ORDER2 = A.MEASURED, A.MEASURED_ORDER2


def _points(d):
    return np.random.default_rng(1).standard_normal((50, d))


def _check(klib, src, sampler, d):
    return klib.klara_check_custom_target(src.encode(), sampler, d)


# ---- 1. the compile check: these fail without the feature (KLARA_ERR_COMPILE: no gradient closure)
def test_autodiff_sources_compile_without_a_gpu(klib):
    assert _check(klib, A.marked(A.AD_NEGDOT), L.SAMPLER_MALA, 3) == 0
    assert _check(klib, A.marked(A.AD_NEGDOT), L.SAMPLER_HMC, 33) == 0             # (staged: 4 lanes per chain)
    assert _check(klib, A.marked(A.AD_LOGIT, 2), L.SAMPLER_SMMALA, 4) == 0         # (the metric by nested duals)
    assert _check(klib, A.marked(A.AD_NN_LL + A.AD_NN_LP, parts=True), L.SAMPLER_MALA, 5) == 0
    assert _check(klib, A.marked(A.AD_BANANA), L.SAMPLER_MH, 2) == 0               # (MH / slice: the double instantiation only)
    assert _check(klib, A.marked(A.AD_LOGIT, 2), L.SAMPLER_MALA, 4) == 0           # (order 2 with another sampler is order 1)
    K.CustomTarget.autodiff(3, A.AD_ERF).check(L.SAMPLER_HMC)
    K.CustomTarget.autodiff(4, A.AD_LOGIT, A.swiss_block(), order=2).check(L.SAMPLER_SMMALA)


def test_autodiff_refusals(klib):
    # the marker without the generic function: KLARA_ERR_COMPILE, the log names it
    assert _check(klib, A.marked(A.AD_NO_FUNCTION), L.SAMPLER_MALA, 3) == L.ERR_COMPILE
    assert b"klara_user_logtarget_ad" in klib.klara_compile_log()
    assert _check(klib, A.marked(A.AD_NN_LL, parts=True), L.SAMPLER_MALA, 5) == L.ERR_COMPILE
    assert b"klara_user_logprior_ad" in klib.klara_compile_log()
    # pair closures are not differentiated; order 2 keeps SMMALA's limits (D <= 8, not the likelihood + prior form)
    assert _check(klib, A.marked(A.AD_PAIR), L.SAMPLER_MALA, 20) == L.ERR_UNSUPPORTED
    assert _check(klib, A.marked(A.AD_PAIR), L.SAMPLER_MALA, 6) == L.ERR_UNSUPPORTED
    assert _check(klib, A.marked(A.AD_LOGIT, 2), L.SAMPLER_SMMALA, 9) == L.ERR_UNSUPPORTED
    assert _check(klib, A.marked(A.AD_NN_LL + A.AD_NN_LP, 2, parts=True), L.SAMPLER_SMMALA, 5) == L.ERR_UNSUPPORTED
    # order 1 gives SMMALA no metric
    assert _check(klib, A.marked(A.AD_LOGIT, 1), L.SAMPLER_SMMALA, 4) == L.ERR_COMPILE
    assert b"klara_user_tensorlogtarget" in klib.klara_compile_log()
    # ... and a source without the marker still needs its gradient (tests/test_host_api.py)
    with pytest.raises(K.KlaraError) as ei:
        K.CustomTarget(2, cases.SRC_BANANA_LT_ONLY).check(L.SAMPLER_HMC)
    assert ei.value.status == L.ERR_COMPILE and "klara_user_gradlogtarget" in ei.value.log


# ---- 2. the host build against the truth
@pytest.mark.parametrize("name,text,d,data,parts,truth", SOURCES, ids=IDS)
def test_host_build_against_the_truth(name, text, d, data, parts, truth):
    """Gradient of the host build (g++ -ffp-contract=off, one direction per sweep) against the analytic gradient in numpy.longdouble at 50 standard
    normal points, as |error| / (eps * sum |terms| of the element's sum).  Measured maxima: negdot 0 (exact) at every D; banana 1.394; logit swiss
    2.313, D = 9 0.726; quartic chain D = 33 1.055, D = 100 1.058; Normal-Normal 0.850; erf 2.575; Gaussian D = 3 0.787.  The cap is 4 x those."""
    h = R.HostTarget(A.marked(text, 1, 0, parts), d, data)
    worst = 0.0
    for x in _points(d):
        gt, mag = truth(x, data)
        g = h.grad(x).astype(A.LD)
        worst = max(worst, float(np.max(np.abs(g - gt) / (EPS * mag))))
    print(f"{name}: largest error ratio {worst:.3f} (measured {MEASURED[name]})")
    assert worst <= 4.0 * MEASURED[name]


@pytest.mark.parametrize("name,text,d,data,truth", A.host_sources_order2(), ids=[s[0] for s in A.host_sources_order2()])
def test_host_build_of_the_metric_against_the_truth(name, text, d, data, truth):
    """minus the Hessian by nested duals against the analytic one; measured maxima: logit swiss 5.333, Gaussian D = 3 0 (exact)"""
    h = R.HostTarget(A.marked(text, 2), d, data)
    worst = 0.0
    for x in _points(d):
        Gt, mag = truth(x, data)
        G = h.tensor(x).astype(A.LD)
        worst = max(worst, float(np.max(np.abs(G - Gt) / (EPS * mag))))
    print(f"{name}: largest error ratio {worst:.3f} (measured {MEASURED_ORDER2[name]})")
    assert worst <= 4.0 * MEASURED_ORDER2[name]


# ---- 3. / 4. the invariants
@pytest.mark.parametrize("name,text,d,data,parts,truth", SOURCES, ids=IDS)
def test_a2_the_chunk_width_does_not_change_the_bits(name, text, d, data, parts, truth):
    src = A.marked(text, 1, 0, parts)
    hs = [R.HostTarget(src, d, data, chunk=c) for c in (1, 4, d)]
    for x in _points(d)[:10]:
        g = [h.grad(x) for h in hs]
        assert g[0].tobytes() == g[1].tobytes() == g[2].tobytes()


def test_a2_the_metric_does_not_depend_on_the_chunk_widths():
    for name, text, d, data, _ in A.host_sources_order2():
        hs = [R.HostTarget(A.marked(text, 2), d, data, chunk=c, chunk2=c2) for c, c2 in ((1, 1), (d, d), (2, 3))]
        for x in _points(d)[:10]:
            G = [h.tensor(x) for h in hs]
            assert G[0].tobytes() == G[1].tobytes() == G[2].tobytes()


@pytest.mark.parametrize("name,text,d,data,parts,truth", SOURCES, ids=IDS)
def test_a1_the_dual_carries_the_value_of_the_double_instantiation(name, text, d, data, parts, truth):
    h = R.HostTarget(A.marked(text, 1, 0, parts), d, data)
    for x in _points(d)[:20]:
        assert np.float64(h.value(x)).tobytes() == np.float64(h.dual_value(x)).tobytes()


# ---- 5. against the hand-written gradient
def test_negdot_reproduces_the_hand_written_gradient():
    for d in (3, 33):
        h = R.HostTarget(A.marked(A.AD_NEGDOT), d)
        for x in _points(d):
            assert np.array_equal(h.grad(x), -2.0 * x)
    kw = dict(sampler=L.SAMPLER_MALA, target_kind=L.TARGET_CUSTOM, nchains=37, ndims=3, nsteps=30, driftstep=0.6)
    x0 = np.random.default_rng(2).standard_normal((37, 3))
    hand = O.OracleJob(custom_src=cases.SRC_NEGDOT, **kw)
    ad = R.AdOracleJob(custom_src=A.marked(A.AD_NEGDOT), **kw)
    assert hand.set_state(x0) == 0 and ad.set_state(x0) == 0
    assert hand.run(30) == 0 and ad.run(30) == 0
    assert 0.0 < hand.accept.mean() < 1.0
    assert np.array_equal(hand.accept, ad.accept) and np.array_equal(hand.X, ad.X) and np.array_equal(hand.LT, ad.LT) and np.array_equal(hand.G, ad.G)


# ---- 6. the host API
def test_diffoptions_mirrors_the_reference():
    o = K.DiffOptions()
    assert (o.mode, o.order, o.targets, o.chunksize, o.compiled) == ("reverse", 1, [False, False, False], 0, True)
    o = K.DiffOptions(mode=":forward", order=2, chunksize=4)
    assert (o.mode, o.order, o.chunksize) == ("forward", 2, 4)
    with pytest.raises(AssertionError, match="Mode of automatic differentation must be :reverse or :forward, got sideways"):
        K.DiffOptions(mode="sideways")
    with pytest.raises(AssertionError, match="Order of differentiation must be 1 or 2, got order=3"):
        K.DiffOptions(order=3)
    with pytest.raises(AssertionError, match="Length of targets must be 3"):
        K.DiffOptions(targets=[True])
    with pytest.raises(AssertionError, match="chunksize can not be negative, got chunksize=-1"):
        K.DiffOptions(chunksize=-1)


def test_reverse_mode_is_refused_where_a_parameter_is_built():
    with pytest.raises(NotImplementedError, match="forward"):
        K.BasicContMuvParameter("p", logtarget=A.AD_NEGDOT, ndims=3, diffopts=K.DiffOptions())
    with pytest.raises(NotImplementedError, match="forward"):
        K.BasicContMuvParameter("p", loglikelihood=A.AD_NN_LL, logprior=A.AD_NN_LP, ndims=5, diffopts=K.DiffOptions(mode="reverse"))


def test_custom_target_autodiff_prepends_the_defines():
    t = K.CustomTarget.autodiff(3, A.AD_NEGDOT)
    assert t.source == "#define KLARA_USER_AUTODIFF 1\n" + A.AD_NEGDOT and t.autodiff_order == 1 and not t.has_tensor
    t = K.CustomTarget.autodiff(4, A.AD_LOGIT, A.swiss_block(), order=2, chunksize=2)
    assert t.source.startswith("#define KLARA_USER_AUTODIFF 2\n#define KLARA_USER_AUTODIFF_CHUNK 2\n") and t.autodiff_order == 2 and t.has_tensor
    assert K.CustomTarget(3, cases.SRC_NEGDOT).autodiff_order == 0
    with pytest.raises(ValueError):
        K.CustomTarget.autodiff(3, A.AD_NEGDOT, order=3)
    with pytest.raises(ValueError):
        K.CustomTarget.autodiff(3, A.AD_NEGDOT, chunksize=-2)


def test_parameter_with_diffopts_maps_to_the_autodiff_source(monkeypatch):
    """the swiss forwarddiff example: BasicContMuvParameter(:p, loglikelihood=..., logprior=..., diffopts=DiffOptions(mode=:forward))"""
    import klara_jl_amd.api as api
    seen = {}

    class FakeEngine:
        def __init__(self, **kw):
            seen.update(kw)

        def set_state(self, x):
            pass

    monkeypatch.setattr(api, "Engine", FakeEngine)
    blk = A.nn_block(5)
    p = K.BasicContMuvParameter("p", loglikelihood=A.AD_NN_LL, logprior=A.AD_NN_LP, ndims=5, data=blk, diffopts=K.DiffOptions(mode="forward"))
    assert p.target.source == A.marked(A.AD_NN_LL + "\n" + A.AD_NN_LP, parts=True) and p.target.has_parts and p.target.autodiff_order == 1
    K.BasicMCJob(K.likelihood_model(p), K.MALA(0.9), K.BasicMCRange(nsteps=20), {"p": np.zeros(5)})
    assert seen["sampler"] == L.SAMPLER_MALA and seen["target"] is p.target and np.array_equal(seen["target"].data, blk)
    p = K.BasicContMuvParameter("p", logtarget=A.AD_LOGIT, ndims=4, data=A.swiss_block(), diffopts=K.DiffOptions(mode="forward", order=2, chunksize=2))
    assert p.target.source == A.marked(A.AD_LOGIT, 2, 2) and p.target.has_tensor
    K.BasicMCJob(K.likelihood_model(p), K.SMMALA(0.02), K.BasicMCRange(nsteps=20), {"p": np.zeros(4)}, tuner=K.AcceptanceRateMCTuner(0.5))
    assert seen["sampler"] == L.SAMPLER_SMMALA and seen["target"].autodiff_order == 2
    t = K.CustomTarget.autodiff(3, A.AD_NEGDOT)
    assert K.BasicContMuvParameter("p", logtarget=t).target is t
    with pytest.raises(ValueError):
        K.BasicContMuvParameter("p", logtarget=A.AD_NEGDOT, diffopts=K.DiffOptions(mode="forward"))            # ndims
    with pytest.raises(ValueError):
        K.BasicContMuvParameter("p", loglikelihood=A.AD_NN_LL, logprior=A.AD_NN_LP, gradloglikelihood=cases.SRC_NN_GLL, gradlogprior=cases.SRC_NN_GLP,
                                ndims=5, diffopts=K.DiffOptions(mode="forward"))


def test_julia_binding_maps_diffopts():
    """mechanical check of julia/KlaraHIP: Klara's own DiffOptions is imported by name, CustomTarget and HIPParameter take diffopts=, and the source gets
    the marker with the order and the chunk size; reverse mode is refused"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"import\s+Klara:[^\n]*(\n[^\n]*){0,3}\bDiffOptions\b", src)
    m = re.search(r"function autodiff_source\(.*?\nend", src, re.S)
    assert m, "no autodiff_source"
    body = m.group(0)
    assert "diffopts.mode == :forward" in body and "mode=:forward" in body
    assert '"#define KLARA_USER_AUTODIFF "' in body and "diffopts.order" in body
    assert '"#define KLARA_USER_AUTODIFF_CHUNK "' in body and "diffopts.chunksize" in body
    assert re.search(r"CustomTarget\(ndims::Integer, src::AbstractString, data::Vector\{Float64\}=Float64\[\]; diffopts=nothing\)", src)
    assert re.search(r"HIPParameter\(key::Symbol; logtarget::HIPTarget=.*\n\s*diffopts=nothing", src)
    assert "with_diffopts(logtarget, diffopts)" in src


def test_the_header_is_embedded_for_the_run_time_compiler():
    mk = (ROOT / "klara.jl_amd" / "csrc" / "Makefile").read_text()
    assert mk.count("klara_autodiff.h") >= 3
    hdr = (ROOT / "klara.jl_amd" / "csrc" / "klara_autodiff.h").read_text()
    for banned in ("<math.h>", "std::exp", "std::log", "std::erf"):
        assert banned not in hdr, banned
