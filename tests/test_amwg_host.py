"""The AMWG sampler and the Roberts-Rosenthal tuner without a GPU: the ids and refusals of the C ABI, the run-time compilation of the AMWG kernels of a
user's closure for gfx950, the Python API's constructor forms and assertions, the tuner's schedule and hand-counted windows, the CPU reference
(tests/amwg_ref.py) against the independent NumPy restatement (tests/amwg_mirror.py), the statistical soundness of the reference, and the mechanical
checks of the Julia mapping and the header text."""
import re
from pathlib import Path

import numpy as np
import pytest

import amwg_cases as WC
import amwg_ref as WR
import cases
import klara_jl_amd as K
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent


def _status(**over):
    X, y = cases.swiss_data()
    kw = dict(target=K.LogisticTarget(X, y, 100.0), nchains=4, nsteps=20, amwg_logsigma0=np.zeros(4), **WC.amwg(period=50))
    kw.update(over)
    if "target" in over and "amwg_logsigma0" not in over and kw["sampler"] == L.SAMPLER_AMWG:
        kw["amwg_logsigma0"] = np.zeros(kw["target"].ndims)
    try:
        K.Engine(**kw).close()
    except K.KlaraError as e:
        return e.status
    return 0


NOT_AMWG = dict(amwg_logsigma0=None, tuner=L.TUNER_VANILLA, targetrate=0.0)


def test_create_maps_and_refuses_like_the_issue_says(klib, monkeypatch):
    assert L.SAMPLER_AMWG == 10 and L.TUNER_ROBERTS_ROSENTHAL == 3
    ok = (0, L.ERR_HIP)                                               # (without a GPU an accepted job gets as far as the device)
    assert _status() in ok                                            # 10 is accepted
    assert _status(verbose=True, period=5) in ok
    assert _status(monitor=L.MON_ACCEPT | L.MON_SUMMARIES | L.MON_HISTORY | L.MON_HIST_LT) in ok
    for d, n in ((1, 50), (3, 40), (8, 200), (11, 70), (16, 300)):    # kinds 2 (row split) and 0, E = 2 .. 16
        X, y = cases.synthetic_logit(n, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) in ok
    for d in (1, 5, 16, 17, 32):                                      # whole-vector closures, plain and likelihood + prior form
        assert _status(target=WC.quad_target(0.5, np.eye(d))) in ok
    assert _status(target=WC.make("likprior_d5")["target"]) in ok
    import autodiff_cases as ADC
    assert _status(target=ADC.target(ADC.AD_BANANA, 2, np.array([100.0]))) in ok      # an autodiff source: its double instantiation
    # 5, 7, 9 and 11 are refused
    for s in (5, 7, 9, 11):
        assert _status(sampler=s, **NOT_AMWG) == L.ERR_INVALID_ARG, s
    # the tuner and the sampler go together, per chain
    mh = dict(sampler=L.SAMPLER_MH, mh_sigma=np.ones(4))
    assert _status(**mh, **NOT_AMWG) in ok
    assert _status(**mh, **{**NOT_AMWG, "tuner": L.TUNER_ROBERTS_ROSENTHAL, "targetrate": 0.44}) == L.ERR_UNSUPPORTED      # tuner 3 with MH
    assert _status(tuner=L.TUNER_VANILLA) == L.ERR_UNSUPPORTED                                                            # AMWG with Vanilla
    assert _status(tuner=L.TUNER_ACCEPT_RATE) == L.ERR_UNSUPPORTED
    assert _status(tuner_mode=L.TUNE_POOLED) == L.ERR_UNSUPPORTED
    assert _status(tuner=4) == L.ERR_INVALID_ARG
    # amwg_logsigma0: required for AMWG, finite, and AMWG's alone
    assert _status(amwg_logsigma0=None) == L.ERR_INVALID_ARG
    assert _status(amwg_logsigma0=np.array([0.0, np.inf, 0.0, 0.0])) == L.ERR_INVALID_ARG
    assert _status(amwg_logsigma0=np.array([0.0, np.nan, 0.0, 0.0])) == L.ERR_INVALID_ARG
    assert _status(**mh, **{**NOT_AMWG, "amwg_logsigma0": np.zeros(4)}) == L.ERR_INVALID_ARG
    # RobertsRosenthalMCTuner.jl:89-93
    for v in (0.0, 1.0, -0.2, float("nan")):
        assert _status(targetrate=v) == L.ERR_INVALID_ARG
    assert _status(period=0) == L.ERR_INVALID_ARG
    # D = 33, and a logistic job beyond the row-split kernels
    assert _status(target=WC.quad_target(0.5, np.eye(33))) == L.ERR_UNSUPPORTED
    for d in (17, 20):
        X, y = cases.synthetic_logit(60, d)
        assert _status(target=K.LogisticTarget(X, y, 10.0)) == L.ERR_UNSUPPORTED
    # pair closures, the Gaussian and hierarchical families
    assert _status(target=K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT)) == L.ERR_UNSUPPORTED
    assert _status(target=K.CustomTarget.pairwise(20, cases.SRC_PAIR_NEGDOT)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDiagTarget.negdot(4)) == L.ERR_UNSUPPORTED
    assert _status(target=K.GaussDenseTarget(np.eye(4))) == L.ERR_UNSUPPORTED
    assert _status(target=cases.rats_target()) == L.ERR_UNSUPPORTED
    # more than one lane per chain
    monkeypatch.setenv("KLARA_CUSTOM_LANES", "4")
    assert _status(target=WC.quad_target(0.5, np.eye(3))) == L.ERR_UNSUPPORTED
    monkeypatch.delenv("KLARA_CUSTOM_LANES")
    # the getters need a handle
    assert klib.klara_get_amwg_state(None, None, None, None) == L.ERR_INVALID_ARG
    assert klib.klara_set_amwg_logsigma(None, None) == L.ERR_INVALID_ARG
    assert klib.klara_get_amwg_accept_mask(None, None, 0, None) == L.ERR_INVALID_ARG


def test_check_custom_target_compiles_the_amwg_kernels(klib):
    """klara_check_custom_target(src, KLARA_SAMPLER_AMWG, D) compiles the AMWG kernels of a user's closure for gfx950 (no GPU needed) at D = 1, 5, 16, 17, 32
    (E = 2, 8, 16, 32, 32), in the plain and the likelihood + prior form"""
    import ram_cases as RC

    def check(src, d, sampler=L.SAMPLER_AMWG):
        return klib.klara_check_custom_target(src.encode(), sampler, d)
    for d in (1, 5, 16, 17, 32):
        assert check(WC.SRC_QUAD, d) == 0, klib.klara_compile_log()
        assert check(WC.make(f"likprior_d{d}")["target"].source, d) == 0, klib.klara_compile_log()
    assert check(cases.SRC_BANANA_LT_ONLY, 2) == 0
    assert check(RC.SRC_HALFSPACE, 2) == 0, klib.klara_compile_log()
    import autodiff_cases as ADC
    assert check(ADC.target(ADC.AD_BANANA, 2, np.array([100.0])).source, 2) == 0, klib.klara_compile_log()
    assert check(WC.SRC_QUAD, 33) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(4, cases.SRC_PAIR_NEGDOT).source, 4) == L.ERR_UNSUPPORTED
    assert check(K.CustomTarget.pairwise(20, cases.SRC_PAIR_NEGDOT).source, 20) == L.ERR_UNSUPPORTED
    for s in (5, 7, 9, 11):
        assert check(WC.SRC_QUAD, 3, sampler=s) == L.ERR_INVALID_ARG
    K.CustomTarget(3, WC.SRC_QUAD).check(L.SAMPLER_AMWG)


def test_python_api_mirrors_the_reference_constructors():
    s = K.MuvAMWG(np.array([0.5, 1.0, 2.0]))                          # MuvAMWG(σ::RealVector): map(log, σ), no bounds
    assert s.kind == L.SAMPLER_AMWG and np.array_equal(s.logsigma0, np.log([0.5, 1.0, 2.0]))
    assert np.all(np.isneginf(s.lower)) and np.all(np.isposinf(s.upper))
    s = K.MuvAMWG(4)                                                  # MuvAMWG(d; lower, upper, σ = 1.)
    assert np.array_equal(s.logsigma0, np.zeros(4)) and s.lower.size == 4
    s = K.MuvAMWG(3, sigma=2.0)
    assert np.array_equal(s.logsigma0, np.full(3, np.log(2.0)))
    assert np.array_equal(K.MuvAMWG(3, **{"σ": 2.0}).logsigma0, s.logsigma0)
    assert np.array_equal(K.MuvAMWG(2, lower=[-np.inf, -np.inf], upper=[np.inf, np.inf]).logsigma0, np.zeros(2))
    assert K.AMWG is K.MuvAMWG
    # W5: a finite bound is refused, by name
    with pytest.raises(NotImplementedError, match="`lower`"):
        K.MuvAMWG(2, lower=[0.0, -np.inf])
    with pytest.raises(NotImplementedError, match="`upper`"):
        K.MuvAMWG(2, upper=[np.inf, 5.0])
    with pytest.raises(ValueError):
        K.MuvAMWG(2, lower=[-np.inf])
    with pytest.raises(TypeError):
        K.MuvAMWG(np.ones(2), sigma=2.0)
    t = K.RobertsRosenthalMCTuner()                                   # RobertsRosenthalMCTuner(; targetrate=0.44, period=50, verbose=false)
    assert t.kind == L.TUNER_ROBERTS_ROSENTHAL and (t.targetrate, t.period, t.verbose) == (0.44, 50, False)
    t = K.RobertsRosenthalMCTuner(targetrate=0.3, period=7, verbose=True)
    assert (t.targetrate, t.period, t.verbose) == (0.3, 7, True)
    for v in (0.0, 1.0, -1.0):
        with pytest.raises(AssertionError, match="Target acceptance rate should be between 0 and 1"):
            K.RobertsRosenthalMCTuner(targetrate=v)
    with pytest.raises(AssertionError, match="Tuning period should be positive"):
        K.RobertsRosenthalMCTuner(period=0)
    for name in ("MuvAMWG", "AMWG", "RobertsRosenthalMCTuner"):
        assert name in K.__all__
    klara = set((ROOT / "tests" / "golden" / "klara_exports.txt").read_text().split())
    assert {"MuvAMWG", "AMWG", "RobertsRosenthalMCTuner"} <= klara


def test_basic_mc_job_maps_amwg_to_the_descriptor(monkeypatch):
    import klara_jl_amd.api as A
    seen = {}

    class FakeEngine:
        def __init__(self, **kw):
            seen.clear(); seen.update(kw)

        def set_state(self, x):
            pass

    monkeypatch.setattr(A, "Engine", FakeEngine)
    X, y = cases.swiss_data()
    p = K.BasicContMuvParameter("p", logtarget=K.LogisticTarget(X, y, 100.0))
    rng = K.BasicMCRange(nsteps=50, burnin=10)
    K.BasicMCJob(K.likelihood_model(p), K.MuvAMWG(np.full(4, 0.5)), rng, {"p": WC.SWISS_X0}, tuner=K.RobertsRosenthalMCTuner(targetrate=0.3, period=7))
    assert seen["sampler"] == L.SAMPLER_AMWG and np.array_equal(seen["amwg_logsigma0"], np.log(np.full(4, 0.5)))
    assert seen["tuner"] == L.TUNER_ROBERTS_ROSENTHAL and (seen["targetrate"], seen["period"], seen["verbose"]) == (0.3, 7, False)
    assert "mh_sigma" not in seen and "am_C0" not in seen and "tuner_mode" not in seen
    K.BasicMCJob(K.likelihood_model(p), K.MuvAMWG(4), rng, {"p": WC.SWISS_X0})                  # no tuner given: the reference's defaults
    assert seen["tuner"] == L.TUNER_ROBERTS_ROSENTHAL and (seen["targetrate"], seen["period"]) == (0.44, 50)
    with pytest.raises(NotImplementedError):
        K.BasicMCJob(K.likelihood_model(p), K.MuvAMWG(4), rng, {"p": WC.SWISS_X0}, tuner=K.VanillaMCTuner())
    with pytest.raises(NotImplementedError):
        K.BasicMCJob(K.likelihood_model(p), K.MH(np.ones(4)), rng, {"p": WC.SWISS_X0}, tuner=K.RobertsRosenthalMCTuner())


def test_delta_schedule_and_hand_counted_windows():
    """δ = min(0.01, batch^-1/2): 0.01 up to batch 10,000, below it from 10,001 on; logσ after windows counted by hand"""
    assert WR.delta_of(1) == 0.01 and WR.delta_of(10000) == 0.01
    assert WR.delta_of(10001) < 0.01 and WR.delta_of(10001) == 1.0 / np.sqrt(10001.0)
    assert WR.delta_of(40000) == 0.005
    # period 5, target rate 0.44: 3 of 5 accepted -> 0.6 >= 0.44: up; 2 of 5 -> 0.4 < 0.44: down; 0 -> down; 5 -> up
    ls = np.array([0.0, 1.0, -2.0, 0.25]); acc = np.array([3, 2, 0, 5], np.int32)
    WR.tune(ls, acc, 5, 0.44, 0.01)
    assert np.array_equal(ls, np.array([0.0 + 0.01, 1.0 - 0.01, -2.0 - 0.01, 0.25 + 0.01])) and not acc.any()
    # a rate equal to the target moves up: the reference's test is rate < targetrate
    ls = np.array([0.0]); acc = np.array([2], np.int32)
    WR.tune(ls, acc, 5, 0.4, 0.01)
    assert ls[0] == 0.01
    # a job: the windows of the coordinate masks, counted here, give the reference's logσ — and the schedule restarts with the job
    case = WC.make("mirror_d3")
    job = WC.ref_job(case, nchains=2)
    assert job.set_state(case["x0"][:2]) == 0 and job.run(23) == 0
    for c in range(2):
        ls = np.array(case["amwg_logsigma0"], dtype=float)
        for w in range(4):                                            # four complete windows in 23 transitions; the fifth is open
            for i in range(3):
                k = int(((job.masks[5 * w:5 * w + 5, c] >> i) & 1).sum())
                ls[i] = ls[i] + (-0.01 if k / 5 < 0.44 else 0.01)
        assert np.array_equal(job.logsigma[c], ls)
        assert np.array_equal(job.accepted[c], [int(((job.masks[20:23, c] >> i) & 1).sum()) for i in range(3)])
        assert np.array_equal(job.naccept_coord[c], [int(((job.masks[:, c] >> i) & 1).sum()) for i in range(3)])
    assert job.reset() == 0
    assert np.array_equal(job.logsigma, np.broadcast_to(case["amwg_logsigma0"], (2, 3))) and not job.accepted.any() and not job.naccept_coord.any() and job.t == 0


def test_reference_matches_the_numpy_restatement():
    """D = 3 quadratic, 60 transitions, period 5 (12 tuning events): every coordinate mask equal, the states within 1e-12 (the restatement's normals come
    from libm, a few ulp from the library's), logσ equal (sums of ±0.01 in one order)"""
    case = WC.make("mirror_d3")
    job = WC.reference("mirror_d3")
    chains = WC.mirror_chains(case)
    for c in chains:
        c.run(case["nsteps"])
    masks = np.array([c.masks for c in chains], dtype=np.uint32).T
    assert np.array_equal(masks, job.masks), "coordinate masks differ between the reference and the NumPy restatement"
    dx = np.abs(job.X - np.array([c.x for c in chains])).max()
    dlt = np.abs(job.LT - np.array([c.lt for c in chains])).max()
    print(f"states differ by {dx:.3e}, log-targets by {dlt:.3e}")
    assert dx <= 1e-12 and dlt <= 1e-12
    assert np.array_equal(job.logsigma, np.array([c.logsigma for c in chains]))
    assert np.array_equal(job.accepted, np.array([c.accepted for c in chains]))
    # the masks are no constant: every coordinate is accepted somewhere and rejected somewhere, and the restatement's literal batch / δ are the schedule's
    for i in range(3):
        bit = (job.masks >> i) & 1
        assert 0 < bit.mean() < 1
    assert all(c.deltas == [0.01] * 12 for c in chains)
    assert np.array_equal(job.accept, (job.masks != 0).astype(np.uint8)) and np.array_equal(job.naccept, job.accept.sum(axis=0))


# Bounds of the soundness test, from reasoning (not from the run): the tuner moves logσ up when a window's rate is >= the target and down otherwise, so it
# settles where the two are equally likely: P(Binomial(25, p) < 0.44 * 25 = 11) = 1/2 at p* = 0.427.  logσ then wanders around its level in steps of 0.01;
# the acceptance rate of a random-walk proposal changes by about -0.2 per unit of log standard deviation near there, i.e. -0.1 per unit of logσ, and the
# wander stays well within +-0.5: |p - p*| <= 0.05, plus the binomial noise of 20,000 correlated trials (below 0.01).
RATE_LO, RATE_HI = 0.427 - 0.06, 0.427 + 0.06


def test_reference_is_statistically_sound():
    """N(0, diag(1, 100)), 4 chains started in equilibrium, equal start scales logσ0 = 3, period 25, 9,000 transitions of adaptation and 5,000 kept: the second
    coordinate's logσ ends above the first's by about log(100) = 4.6 (the variance ratio: logσ is a log-variance), the kept transitions' per-coordinate
    acceptance lies around the level the tuner settles at, and the pooled means lie within five Monte Carlo standard errors of 0.  The standard error is
    that of batch means: the kept samples of every chain in 20 batches of 250, SE = sd of the 80 batch means / sqrt(80)."""
    period, n, adapt, keep, nb = 25, 4, 9000, 5000, 20
    x0 = np.random.default_rng(2024).standard_normal((n, 2)) * np.array([1.0, 10.0])
    job = WR.AmwgRefJob(target_kind=L.TARGET_GAUSS_DIAG, nchains=n, ndims=2, nsteps=adapt + keep, burnin=adapt, amwg_logsigma0=np.full(2, 3.0),
                        targetrate=0.44, period=period, seed=77, gauss_w=np.array([0.5, 0.005]), want_hist=True)
    assert job.set_state(x0) == 0 and job.run(adapt + keep) == 0
    gap = job.logsigma[:, 1] - job.logsigma[:, 0]
    kept = job.masks[adapt:]
    rates = [float(((kept >> i) & 1).mean()) for i in range(2)]
    h = job.hist
    assert h.shape == (keep, n, 2)
    mean = h.mean(axis=(0, 1))
    bm = h.reshape(nb, keep // nb, n, 2).mean(axis=1).reshape(nb * n, 2)
    se = bm.std(axis=0, ddof=1) / np.sqrt(nb * n)
    print(f"logσ {job.logsigma.mean(axis=0)}, gap {gap}, kept acceptance {rates}, pooled means {mean}, batch-means SE {se}, variances {h.var(axis=(0, 1))}")
    assert np.all(job.logsigma[:, 1] > job.logsigma[:, 0]) and np.all(np.abs(gap - np.log(100.0)) < 1.0)
    assert all(RATE_LO <= r <= RATE_HI for r in rates), rates
    assert np.all(np.abs(mean) <= 5.0 * se), (mean, se)
    assert np.all(job.logsigma != 3.0)


def test_julia_binding_maps_amwg():
    """mechanical check of julia/KlaraHIP: MuvAMWG and RobertsRosenthalMCTuner are Klara's own (imported, not exported), mapped to SAMPLER_AMWG and
    TUNER_ROBERTS_ROSENTHAL with logσ0, the target rate and the period; amwgstate is exported — a name Klara does not export"""
    src = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    assert re.search(r"const\s+SAMPLER_AMWG\s*=\s*Int32\(10\)", src) and re.search(r"const\s+TUNER_ROBERTS_ROSENTHAL\s*=\s*Int32\(3\)", src)
    imp = re.search(r"^import Klara: ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    assert re.search(r"\bMuvAMWG\b", imp) and re.search(r"\bRobertsRosenthalMCTuner\b", imp)
    export = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", src, re.M).group(1)
    names = {t for t in re.split(r"[,\s]+", export) if t}
    assert "amwgstate" in names and "MuvAMWG" not in names and "RobertsRosenthalMCTuner" not in names
    klara = set((ROOT / "tests" / "golden" / "klara_exports.txt").read_text().split())
    assert "MuvAMWG" in klara and "RobertsRosenthalMCTuner" in klara and "amwgstate" not in klara
    m = re.search(r"isa\(sampler,\s*MuvAMWG\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S)
    assert m, "no MuvAMWG branch in the sampler mapping"
    body = m.group(1)
    for f in ("SAMPLER_AMWG", "sampler.logσ0", "sampler.lower", "sampler.upper", "amwg_logsigma0", "`lower`", "`upper`"):
        assert f in body, f
    m = re.search(r"elseif isa\(tn,\s*RobertsRosenthalMCTuner\)(.*?)(?:\n\s*elseif|\n\s*else)", src, re.S)
    assert m and "TUNER_ROBERTS_ROSENTHAL" in m.group(1) and "tn.targetrate" in m.group(1)
    assert re.search(r"^function amwgstate\(job::HIPMCJob\)", src, re.M) and "klara_get_amwg_state" in src
    # the struct, the keyword constructor and its positional call list the new field in the header's place
    jstruct = re.search(r"struct KlaraDesc\n(.*?)\nend", src, re.S).group(1)
    jnames = [n for n, _ in re.findall(r"(\w+)::([\w{}]+)", jstruct)]
    assert jnames == [n for n, _ in L.KlaraDesc._fields_]
    assert jnames[jnames.index("slice_widths") + 1] == "amwg_logsigma0"


def test_header_states_the_sampler(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    assert re.search(r"KLARA_SAMPLER_AMWG\s*=\s*10", hdr) and re.search(r"KLARA_TUNER_ROBERTS_ROSENTHAL\s*=\s*3", hdr)
    assert re.search(r"#define\s+KLARA_ABI_VERSION\s+6\b", hdr) and L.KLARA_ABI_VERSION == 6 and klib.klara_abi_version() == 6
    body = hdr[hdr.index("typedef struct klara_desc"):hdr.index("} klara_desc;")]
    cnames = [n for _, n in re.findall(r"^\s{4}((?:const\s+)?\w+\*?)\s+(\w+);", body, re.M)]
    assert cnames == [n for n, _ in L.KlaraDesc._fields_] and cnames[-1] == "stream"
    assert L.KlaraDesc.amwg_logsigma0.offset == L.KlaraDesc.slice_widths.offset + 8 and L.KlaraDesc.amwg_logsigma0.size == 8
    for fn in ("klara_get_amwg_state", "klara_set_amwg_logsigma", "klara_get_amwg_accept_mask"):
        assert fn in L.EXPORTS and hasattr(klib, fn) and re.search(rf"klara_status {fn}\(", hdr)
    for w in ("W1-W6", "ceil(D/2) + (i >> 1)", "KLARA_ERR_UNSUPPORTED"):
        assert w in hdr[hdr.index("MuvAMWG(sigma)"):hdr.index("KLARA_SAMPLER_AMWG = 10")]
    design = (ROOT / "DESIGN.md").read_text()
    for k in ("W1", "W2", "W3", "W4", "W5", "W6"):
        assert re.search(rf"\b{k}\b", design), k
    for doc in ("README.md", "INTEGRATION.md"):
        assert "AMWG" in (ROOT / doc).read_text(), doc
