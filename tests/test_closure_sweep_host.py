"""The closure sweep (tests/closure_sweep.py, tests/test_gpu_closure_sweep.py) without a GPU: the plan mirror over every staged dimension, the sweep's
dimension tables against the plan classes, every sweep job on the oracle alone (its acceptance window — where the step rule is proven before a GPU sees
it), the compile check of the new closures, and the host build of the coupled likelihood + prior closure's autodiff form.  CPU only (-m "not gpu").

Worked example of the checks biting (run on the CPU, both in this file):
  * test_tables_cover_every_class_and_fail_when_the_plan_moves changes the pad rule and an E of `plan` and sees the coverage assertions fail;
  * test_a_shifted_third_row_is_silent_on_a_separable_target reads a gradient row one element off, as an aliased `ts` row would be: the separable
    likelihood + prior pair of the named case family gives the same bits at almost every element (its rows do not depend on a neighbour), the coupled
    closure of sweep (b) moves them everywhere."""
import ctypes as C
import time

import numpy as np
import pytest

import autodiff_cases as A
import autodiff_ref as R
import cases
import closure_sweep as S
import klara_jl_amd as K
import oracle_ffi as O
from klara_jl_amd import _lib as L


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in ("KLARA_CUSTOM_LANES", "KLARA_CUSTOM_WPB"):
        monkeypatch.delenv(name, raising=False)


# ---- 1. the mirror over every staged dimension
def test_stage_bytes_and_elements_per_lane_within_their_limits():
    for rows in (2, 3):
        for d in S.DIMS:
            g, e, wpb, padded = S.plan(d, rows)
            assert S.stage_bytes(d, rows) <= S.LDS_BYTES, (rows, d, S.stage_bytes(d, rows))
            assert e <= 16 and e == 2 * ((d + 2 * g - 1) // (2 * g)) and g * e >= d and wpb in (2, 4) and g in (4, 8, 16, 32, 64), (rows, d, g, e, wpb)
            assert O.default_layout(L.TARGET_CUSTOM, d, custom_rows=rows) == (0, g, e)
            assert not (padded and rows == 2), d         # 2 dp + 2 = 0 (mod 32) needs an odd dp


def test_class_counts():
    two, three = S.classes(2), S.classes(3)
    for rows, cl in ((2, two), (3, three)):
        print(f"\nrows = {rows}: {len(cl)} plans, {len({k[:3] for k in cl})} (G, E, wpb) shapes")
        for (g, e, wpb, padded), ds in cl.items():
            print(f"  G={g:2d} E={e:2d} wpb={wpb} pad={int(padded)}: {len(ds):3d} dimensions, {ds[0]} .. {ds[-1]}")
    assert len(two) == 24 and all(not k[3] for k in two)
    assert len({k[:3] for k in three}) == 23 and len(three) == 40
    assert sorted(d for k, ds in three.items() if k[3] for d in ds)[:8] == [41, 42, 73, 74, 105, 106, 137, 138]


def _coverage(rows, jobs, plan=None):
    """None, or what is wrong with a table"""
    plan = plan or S.plan
    cl = {}
    for d in S.DIMS:
        cl.setdefault(plan(d, rows), []).append(d)
    dims = [d for d, _ in jobs]
    if len(set(dims)) != len(dims):
        return "a dimension twice"
    hit = [plan(d, rows) for d in dims]
    if set(hit) != set(cl):
        return f"plans not hit: {sorted(set(cl) - set(hit))}"
    if len(hit) != len(set(hit)):
        return "a plan hit twice"
    return None


def test_tables_cover_every_class():
    """every plan once — both pad values where a (G, E, wpb) shape has both —, no dimension twice"""
    assert _coverage(2, S.TWO_ROW_JOBS) is None, _coverage(2, S.TWO_ROW_JOBS)
    assert _coverage(3, S.THREE_ROW_JOBS) is None, _coverage(3, S.THREE_ROW_JOBS)
    assert len(S.TWO_ROW_JOBS) == 24 and len(S.THREE_ROW_JOBS) == 40
    # (b): a padded D wherever the shape has one, and then an unpadded neighbour too
    three = S.classes(3)
    hit = {S.plan(d, 3) for d, _ in S.THREE_ROW_JOBS}
    for shape in {k[:3] for k in three}:
        assert (shape + (True,) in hit) == (shape + (True,) in three)
    print()
    for rows, jobs in ((2, S.TWO_ROW_JOBS), (3, S.THREE_ROW_JOBS)):
        for d, kind in jobs:
            g, e, wpb, padded = S.plan(d, rows)
            print(f"rows={rows} (G={g}, E={e}, wpb={wpb}, pad={int(padded)}) -> D={d} {kind}, {S.nchains(d, rows)} chains")


def test_sampler_rotation():
    for rows, jobs in ((2, S.TWO_ROW_JOBS), (3, S.THREE_ROW_JOBS)):
        kinds = [k for _, k in jobs]
        assert kinds.count("mh") == 2 and kinds.count("slice") == 2
        assert set(kinds) == set(S.GRADIENT_KINDS) | {"mh", "slice"}
        for d, kind in jobs:
            g, _, wpb, _ = S.plan(d, rows)
            assert kind in S.GRADIENT_KINDS or (wpb == 4 and g < 64), (rows, d, kind)      # every wpb = 2 and every G = 64 class: a gradient sampler
        for want in (2, 4):
            assert {k for d, k in jobs if S.plan(d, rows)[2] == want} >= {"mala", "hmc", "hmc_da"}


def test_workgroup_shape_and_autodiff_tables(monkeypatch):
    assert sorted(S.plan(d, rows)[0] for rows, d, _ in S.WPB_JOBS) == [8, 16, 64]
    assert any(S.plan(d, rows)[3] for rows, d, _ in S.WPB_JOBS)
    for rows, d, _ in S.WPB_JOBS:
        shapes = []
        for wpb in ("2", "4"):
            monkeypatch.setenv("KLARA_CUSTOM_WPB", wpb)
            g, e, w, _ = S.plan(d, rows)
            assert w == int(wpb) and S.stage_bytes(d, rows) <= S.LDS_BYTES, (rows, d, wpb)       # the rows fit at both
            shapes.append((g, e))
        assert shapes[0] == shapes[1]
    monkeypatch.delenv("KLARA_CUSTOM_WPB")
    for rows, d, kind, chunk in S.AD_JOBS:
        assert S.plan(d, rows)[:3] == S.AD_EXPECTED[(rows, d)] and kind in ("mala", "hmc")
    two = [S.plan(d, 2) for rows, d, _, c in S.AD_JOBS if rows == 2 and c == 0]
    assert sorted(p[1] for p in two) == [8, 10, 12, 14, 16] and sum(p[2] == 2 for p in two) == 2 and sum(p[0] == 64 for p in two) == 1
    three = [S.plan(d, 3) for rows, d, _, _ in S.AD_JOBS if rows == 3]
    assert {p[1] for p in three} >= {6, 16} and any(p[3] for p in three)
    assert [(d, c) for rows, d, _, c in S.AD_JOBS if c] == [(45, 5)] and S.plan(45, 2)[1] == 12
    assert S.PAIR_DIMS == [17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 97, 100, 104, 127, 128, 129, 255, 256, 257, 511, 512, 513, 777, 1023, 1024]
    assert len(S.PAIR_JOBS) == 26 + 3 * 9


def test_tables_cover_every_class_and_fail_when_the_plan_moves():
    """the coverage check bites: with another pad rule, or another E at one G, the same tables no longer cover the classes"""
    def no_pad_rule(d, rows):
        g, e, wpb, _ = S.plan(d, rows)
        return g, e, wpb, False
    def other_e(d, rows):
        g, e, wpb, padded = S.plan(d, rows)
        return g, (e + 2 if (g == 16 and e == 12) else e), wpb, padded
    assert _coverage(3, S.THREE_ROW_JOBS, no_pad_rule) == "a plan hit twice"
    assert _coverage(2, S.TWO_ROW_JOBS, other_e) == "a plan hit twice"
    assert _coverage(3, S.THREE_ROW_JOBS, other_e) == "a plan hit twice"
    assert _coverage(2, S.TWO_ROW_JOBS[:-1]).startswith("plans not hit")


# ---- 2. every sweep job on the oracle alone
def _alone(case, layout, ad=False):
    t0 = time.time()
    st, rate, job = S.oracle_alone(case, layout, ad)
    print(f"{case['name']}: layout {tuple(layout)}, {case['nchains']} chains x {case['nsteps']} transitions, oracle acceptance {rate:.3f}, "
          f"{time.time() - t0:.2f} s")
    assert st == 0, (case["name"], st)            # (a slice job: never KLARA_ERR_SLICE_STUCK)
    if case["sampler"] == L.SAMPLER_SLICE:
        assert rate == 1.0
    else:
        assert 0.05 < rate < 0.95, (case["name"], rate)
    return job


@pytest.mark.parametrize("rows,d,kind", [(2, d, k) for d, k in S.TWO_ROW_JOBS] + [(3, d, k) for d, k in S.THREE_ROW_JOBS],
                         ids=[f"rows{r}-d{d}-{k}" for r, jobs in ((2, S.TWO_ROW_JOBS), (3, S.THREE_ROW_JOBS)) for d, k in jobs])
def test_staged_jobs_on_the_oracle_alone(rows, d, kind):
    case = S.staged_case(rows, d, kind)
    g, e, wpb, _ = S.plan(d, rows)
    assert case["nchains"] == wpb * (64 // g) + 64 // g + 1
    job = _alone(case, (0, g, e))
    if case.get("tuner", 0) == L.TUNER_DUAL_AVERAGING:
        assert case["da_nadapt"] == 9 < case["nsteps"]
    if rows == 3 and kind not in ("mh", "slice"):
        # ll + lp is the composed log-target (-s + -(k/2 t): the bits of the whole-vector closure's -s - (k/2) t), and gll + glp is ANOTHER rounding than the
        # whole-vector closure's gradient (site term + both coupling terms in one chain of additions): the two forms are different jobs
        lib = O.compile_user_target(case["target"].source, d)[0]
        whole = O.compile_user_target(cases.SRC_QUARTIC_CHAIN, d)[0]
        dp = C.POINTER(C.c_double)
        for f in (lib.klara_user_loglikelihood, lib.klara_user_logprior):
            f.restype, f.argtypes = C.c_double, [dp, C.c_int, dp, C.c_longlong]
        whole.klara_user_gradlogtarget.restype, whole.klara_user_gradlogtarget.argtypes = None, [dp, C.c_int, dp, C.c_longlong, dp]
        data = case["target"].data
        differs = 0
        for c in range(case["nchains"]):
            x = np.ascontiguousarray(job.X[c]); gw = np.zeros(d)
            args = (x.ctypes.data_as(dp), d, data.ctypes.data_as(dp), data.size)
            assert lib.klara_user_loglikelihood(*args) + lib.klara_user_logprior(*args) == job.LT[c]
            whole.klara_user_gradlogtarget(*args, gw.ctypes.data_as(dp))
            differs += int(np.count_nonzero(gw != job.G[c]))
        assert differs > 0


@pytest.mark.parametrize("rows,d,kind", S.WPB_JOBS, ids=[f"rows{r}-d{d}-{k}" for r, d, k in S.WPB_JOBS])
def test_workgroup_shape_jobs_on_the_oracle_alone(rows, d, kind):
    g, e, _, _ = S.plan(d, rows)
    _alone(S.staged_case(rows, d, kind, n=4 * (64 // g) + 64 // g + 1), (0, g, e))


@pytest.mark.parametrize("rows,d,kind,chunk", S.AD_JOBS, ids=[f"rows{r}-d{d}-{k}-c{c}" for r, d, k, c in S.AD_JOBS])
def test_autodiff_jobs_on_the_host_build_alone(rows, d, kind, chunk):
    g, e, _, _ = S.plan(d, rows)
    _alone(S.ad_case(rows, d, kind, chunk), (0, g, e), ad=True)


@pytest.mark.parametrize("kind", ["mala", "hmc", "mh", "slice"])
def test_pair_jobs_on_the_oracle_alone(kind):
    for d, k in S.PAIR_JOBS:
        if k == kind:
            layout = O.default_layout(L.TARGET_CUSTOM, d, pair_form=True)
            assert layout[:2] == (3, S.pair_lanes(d))
            _alone(S.pair_case(d, kind), layout)


# ---- 3. compile checks (no GPU needed)
def test_new_closures_compile(klib):
    def check(src, sampler, d):
        st = klib.klara_check_custom_target(src.encode(), sampler, d)
        assert st == 0, (st, klib.klara_compile_log())
    assert S.plan(105, 3) == (8, 14, 2, True) and S.plan(106, 3)[3] and S.plan(120, 2)[1] == 16
    check(S.coupled_target(105).source, L.SAMPLER_HMC, 105)
    check(A.marked(S.AD_QC_LL + S.AD_QC_LP, parts=True), L.SAMPLER_MALA, 106)
    check(A.marked(A.AD_QUARTIC_CHAIN), L.SAMPLER_HMC, 120)


# ---- 4. the host builds of the coupled closure agree
PARTS_D = 105


def _hand_gradient(d):
    lib = O.compile_user_target(S.coupled_target(d).source, d)[0]
    dp = C.POINTER(C.c_double)
    lib.klara_user_gradlogtarget.restype, lib.klara_user_gradlogtarget.argtypes = None, [dp, C.c_int, dp, C.c_longlong, dp]
    def grad(x):
        x = np.ascontiguousarray(x, dtype=np.float64); g = np.zeros(d)
        lib.klara_user_gradlogtarget(x.ctypes.data_as(dp), d, S.QC_DATA.ctypes.data_as(dp), 2, g.ctypes.data_as(dp))
        return g
    return grad


def test_host_builds_of_the_coupled_closure_agree():
    """Gradient of the likelihood + prior autodiff form (g++, one direction per sweep) and the hand-written gll + glp (gcc, klara_custom_compose.h's one addition
    per element) at 50 standard-normal points of D = 105, each against the analytic gradient in numpy.longdouble and against one another, as
    |difference| / (eps * sum |terms|) — tests/test_autodiff_host.py's measure.  Measured maxima: hand-written 1.102, autodiff 1.079, between the two 1.604;
    the cap on all three is 4 x the hand-written form's."""
    d = PARTS_D
    hand = _hand_gradient(d)
    ad = R.HostTarget(A.marked(S.AD_QC_LL + S.AD_QC_LP, parts=True), d, S.QC_DATA)
    worst = dict(hand=0.0, ad=0.0, between=0.0)
    for x in np.random.default_rng(1).standard_normal((50, d)):
        gt, mag = A.truth_quartic(x, S.QC_DATA)
        gh, ga = hand(x).astype(A.LD), ad.grad(x).astype(A.LD)
        worst["hand"] = max(worst["hand"], float(np.max(np.abs(gh - gt) / (A.EPS * mag))))
        worst["ad"] = max(worst["ad"], float(np.max(np.abs(ga - gt) / (A.EPS * mag))))
        worst["between"] = max(worst["between"], float(np.max(np.abs(ga - gh) / (A.EPS * mag))))
    print(f"quartic_parts_d{d}: largest error ratios {worst} (measured: hand-written {A.MEASURED['quartic_parts_hand_d105']}, autodiff {A.MEASURED['quartic_parts_d105']})")
    cap = 4.0 * A.MEASURED["quartic_parts_hand_d105"]
    assert worst["hand"] <= cap and worst["ad"] <= cap and worst["between"] <= cap, worst


# ---- 5. why the three-row sweep runs a COUPLED closure
def test_a_shifted_third_row_is_silent_on_a_separable_target():
    """A `ts` row read from one chain's row too far (a wrong stride in a pad case) hands a lane its neighbour chain's gradlogprior.  Modelled on the host: the prior
    gradient of chain c + 1 in place of chain c's, at two chains whose states agree in all but ONE element (the situation right after a launch of identical
    starts, or of any two chains that differ where the reader does not look).  With the separable pair the composed gradient moves at that one element
    only — D - 1 of D elements stay bit-identical, and a comparison of the other lanes' elements passes —; with the coupled closure of sweep (b) the
    element's two neighbours move as well, so a lane boundary between them cannot hide it, and ll + lp moves by the coupling term.  (This is the host-side
    argument; the GPU jobs themselves draw independent starts, where any aliasing moves every element of either target.)"""
    d = 106
    dp = C.POINTER(C.c_double)
    moved = {}
    for name, target in (("separable", S.separable_target(d)), ("coupled", S.coupled_target(d))):
        lib = O.compile_user_target(target.source, d)[0]
        lib.klara_user_gradlogprior.restype, lib.klara_user_gradlogprior.argtypes = None, [dp, C.c_int, dp, C.c_longlong, dp]
        x = 0.5 * np.random.default_rng(3).standard_normal(d)
        y = x.copy(); y[13] += 0.25                                         # the neighbouring chain: 13 is the last element of lane 0 at E = 14
        gx, gy = np.zeros(d), np.zeros(d)
        lib.klara_user_gradlogprior(x.ctypes.data_as(dp), d, S.QC_DATA.ctypes.data_as(dp), 2, gx.ctypes.data_as(dp))
        lib.klara_user_gradlogprior(y.ctypes.data_as(dp), d, S.QC_DATA.ctypes.data_as(dp), 2, gy.ctypes.data_as(dp))
        moved[name] = np.flatnonzero(gx != gy).tolist()
    assert moved["separable"] == [13]
    assert moved["coupled"] == [12, 13, 14]          # 14 is lane 1's first element: the shift shows on a lane that does not own the element that differs
