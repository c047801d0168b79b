"""The pooled effective sample size without a device: tests/ess_ref.py's exact rational reference, its mirror of the device's order of operations and its
derived bounds held against each other on every shape tests/test_gpu_ess.py runs; klara_jl_amd.stats.pooled_ess against exact; what the estimator is
for (chains that disagree); the m = 1 relation to the per-chain imse estimator; the refusals, the rank verdicts and the surface of the C ABI and the
bindings; the merge through torch.distributed."""
import math
import multiprocessing as mp
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest

import klara_jl_amd as K
from klara_jl_amd import _lib as L

import chain_stats_ref as R
import ess_ref as E
import rhat_ref as H

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------- the references against each other, on the GPU tests' shapes
def test_every_shape_has_an_admissible_input_and_none_is_dropped():
    cs = E.cases()
    assert len(cs) == len(set(cs)) >= 70
    seen = {"N": set(), "D": set(), "ml": set(), "kind": set(), "nr": set(), "off": set(), "split_odd": False, "split_even": False}
    for c in cs:
        N, D, ml, ncols, off, kind, nr = c
        hist, exs, _ = E.case_data(c)                                        # raises when no seed is admissible
        assert hist.shape == (ncols, N, D) and (True in exs) == (ncols >= 8)
        for ex in exs.values():
            assert E.admissible(ex, 1) and E.admissible(ex, nr)
        seen["N"].add(N); seen["D"].add(D); seen["ml"].add(ml); seen["kind"].add(kind); seen["nr"].add(nr); seen["off"].add(off)
        seen["split_odd"] |= ncols >= 8 and ncols % 2 == 1; seen["split_even"] |= ncols >= 8 and ncols % 2 == 0
    assert seen["N"] == set(E.NS) and seen["D"] == {1, 3, 4, 100, 1024} and seen["ml"] == set(E.MAXLAGS) and seen["kind"] == set(E.SPLIT_KINDS)
    assert seen["nr"] == {1, 2, 3, 4} and seen["off"] == set(E.OFFSETS) and seen["split_odd"] and seen["split_even"]
    for ml in E.MAXLAGS:                                                     # every window meets every length, the clipped ones among them
        assert {E.ncols_of(k, ml) for k in E.NCOLS_KINDS} <= {c[3] for c in cs if c[2] == ml and c[0] == 3}
    assert any(c[0] * c[1] > E.ESS_BLOCKS * E.THREADS for c in cs)           # more unit-series than stage 1 has lanes
    assert any(len(ex["cols"]) and np.any(ex["wsum"] > 0) for c in cs for ex in E.case_data(c)[1].values())


@pytest.mark.parametrize("case", E.cases(), ids=lambda c: "N%d-D%d-lag%d-n%d-off%g-%s-r%d" % c)
def test_mirror_and_stats_are_within_the_bound_of_exact(case):
    """mirror and mirror_ranks within bound() of exact with identical pairs; the streamed sums do not depend on the launches; stats.pooled_ess within the
    plain form's bound of exact"""
    N, D, ml, ncols, _, kind, nranks = case
    hist, exs, _ = E.case_data(case)
    bounds = H.rank_bounds(N)[nranks]
    for split, ex in exs.items():
        mir = E.mirror(hist, ml, split)
        E.check(mir, None, ex, 1, (case, split))
        mrk = E.mirror_ranks(bounds, hist, ml, split)
        E.check(mrk, None, ex, nranks, (case, split, "ranks"))
        assert np.array_equal(mir["pairs"], mrk["pairs"])
        if not split:
            cut = E.mirror(hist, ml, False, E.launch_splits(ncols, kind))
            for k in ("csum", "wsum", "mean", "bsum", "rho", "tau", "ess"):
                assert np.array_equal(cut[k], mir[k], equal_nan=True), (case, k)
        st = K.stats.pooled_ess(hist, ml, split)
        E.check(st, None, ex, 1, (case, split, "stats"), plain=True)
        assert np.array_equal(st["window_exhausted"], st["pairs"] == (max(ex["L"] - 1, 0) // 2 + 1))


def test_streamed_sums_are_exact_on_the_grid_and_stream_state_is_stream_f64s():
    """What bound() starts from: on the dyadic grid S, total, head and tail are exact — equal to integer arithmetic; and the state restated here gives, through
    k_acov_finalize's formulas, chain_stats_ref.stream_f64's estimators bit for bit"""
    v = R.ar1_series(90, 12, 5) + 1e6 * E.SD
    for W, splits in ((8, [90]), (40, E.launch_splits(90, "ragged")), (128, E.launch_splits(90, "32s"))):
        S, head, tail, total = E.stream_state(v, W, splits)
        zi = np.rint((v - v[0]) / E.GRID).astype(np.int64)
        for k in range(min(W, 90)):
            assert np.array_equal(S[k] / E.GRID ** 2, (zi[k:] * zi[:90 - k]).sum(axis=0).astype(np.float64))
            assert np.array_equal(tail[k] / E.GRID, zi[89 - k].astype(np.float64)) and np.array_equal(head[k], v[k])
        assert np.array_equal(total / E.GRID, zi.sum(axis=0).astype(np.float64))
        c, mu = E.unit_lagged_sums((S, head, tail, total), 90, min(W - 1, 89))
        imse, _ = R.stream_f64(v, W, splits)
        kk = (min(W - 1, 89) - 1) // 2
        for i in range(v.shape[1]):                                          # imse from c = n acv, as k_acov_finalize sums it
            a = c[:, i] / 90.0
            gs = gprev = 0.0
            for j in range(kk + 1):
                pair = 0.0 + a[2 * j]
                pair += a[2 * j + 1]
                if pair <= 0.0:
                    break
                gm = gprev if (j > 0 and pair > gprev) else pair
                gs += gm; gprev = gm
            assert (-a[0] + 2.0 * gs) / 90.0 == imse[i]


# ---------------------------------------------------------------- the reason it exists
def _iid_chains(mu_sd, seed=3):
    rng = np.random.default_rng(seed)
    m, n, D = 32, 400, 3
    mu = mu_sd * rng.standard_normal((m, D))
    return rng.standard_normal((n, m, D)) + mu[None], m, n, D


def test_chains_that_disagree_are_not_worth_m_times_n_draws():
    """m = 32 iid N(mu_j, 1) chains of n = 400, the mu_j spread 3 sd apart, maxlag = 31.  Each chain's own ESS is about n — its autocovariance is taken
    around its own mean — so their sum says 12,800 draws.  Pooled: with B = the sample variance of the mu_j (about 9) and W about 1, every
    rho[k] = 1 - (W - csum[k] / (m n)) / var+ is rho_b + (1 - rho_b) r_k with rho_b = 1 - W / var+ (about 0.9) and r_k the pooled within-chain
    autocorrelation, 0 +- 1 / sqrt(m n) = 0.009.  No pair is <= 0, the window (16 pairs) is exhausted in every dimension, and tau = -1 + 2 (1 + sum_(k=1..31)
    rho[k]) = 1 + 62 rho_b + 2 (1 - rho_b) sum r_k: the last term has sd 2 * 0.1 * sqrt(31) * 0.009 = 0.01, and the monotone clamp moves a pair by the same
    order; 0.5 is fifty of those.  tau is about 1.8 * 32 - 1, the pooled ESS below a tenth of the per-chain sum."""
    x, m, n, D = _iid_chains(3.0)
    out = K.stats.pooled_ess(x, 31)
    per_chain = np.array([[K.stats.ess(x[:, c, d], "imse", 31) for d in range(D)] for c in range(m)]).sum(axis=0)
    assert np.all(per_chain > 0.7 * m * n)
    assert np.all(out["ess"] < 0.1 * per_chain), (out["ess"], per_chain)
    assert np.all(out["window_exhausted"]) and np.all(out["pairs"] == 16)
    W = out["wsum"] / (m * (n - 1)); varp = (n - 1) / n * W + out["bsum"] / (m - 1)
    rho_b = 1.0 - W / varp
    assert np.all(np.abs(rho_b - 0.9) < 0.06)                                # B = 9 chi2_31 / 31: rho_b in 0.9 +- 3 * 0.02
    assert np.all(np.abs(out["tau"] - (1.0 + 62.0 * rho_b)) < 0.5), (out["tau"], 1.0 + 62.0 * rho_b)
    assert np.all(np.abs(out["tau"] - (1.8 * 32 - 1)) < 62 * 0.06 + 0.5)
    ex = E.exact(np.rint(x / E.GRID) * E.GRID, 31)                           # and the exact reference sees the same
    assert np.all(ex["pairs"] == 16) and np.allclose(ex["tau"], out["tau"], rtol=0.01)


def test_chains_that_agree_are_worth_the_sum_of_their_own_ess():
    """The same chains with a common mu.  Both estimates are m n / tau-hat with tau = 1: the pooled rho[k] has sd 1 / sqrt(m n) = 0.009 and tau-hat sums about
    three of them twice — a relative sd of 3 %; a chain's own tau-hat has sd 2 sqrt(3 / n) = 0.17, so the mean over 32 chains of n / tau-hat has a relative
    sd of 3 % and, 1 / tau being convex, a bias of about var(tau-hat) = 3 %.  0.25 is five standard deviations of their difference plus the bias."""
    x, m, n, D = _iid_chains(0.0)
    out = K.stats.pooled_ess(x, 31)
    per_chain = np.array([[K.stats.ess(x[:, c, d], "imse", 31) for d in range(D)] for c in range(m)]).sum(axis=0)
    assert np.all(np.abs(out["ess"] / per_chain - 1.0) < 0.25), (out["ess"], per_chain)
    assert np.all(np.abs(out["ess"] / (m * n) - 1.0) < 0.15) and not np.any(out["window_exhausted"])


def test_one_chain_reproduces_the_imse_estimator_up_to_the_n_minus_1_factors():
    """m = 1: W = c(0) / (n - 1), var+ = (n - 1) / n W = acv_0 (StatsBase's autocov at lag 0), so rho[k] = acv_k / acv_0 - 1 / (n - 1) for k >= 1 and
    rho[0] = 1 by definition: P_0 = Gamma_0 / acv_0 - 1 / (n - 1) and P_j = Gamma_j / acv_0 - 2 / (n - 1), Gamma_j the pairs of mcvar.jl:75-105.  The shifts are
    the same for all j >= 1, so the monotone clamp decides alike from the second comparison on.  Where neither estimator clamps and both stop after the same
    J >= 1 pairs,
        tau = -1 + 2 sum_(j < J) P_j = (n / (n - 1)) iact_imse - (4 J - 2) / (n - 1),        ess = n / tau
    (iact_imse = mcvar_imse / mcvar_iid = (n - 1) / n (-1 + 2 sum Gamma_j / acv_0)).  Asserted on exact rationals of both references, for the series of
    chain_stats_ref.series_a that meet the condition (decided on exact quantities; most do)."""
    V = R.series_a()
    n = V.shape[0]
    used = 0
    for i in range(V.shape[1]):
        a = R.exact(V[:, i], 31)
        b = E.exact(np.ascontiguousarray(V[:, i].reshape(n, 1, 1)), 31)
        J = int(b["pairs"][0])
        if a["m"] != J or J < 1 or a["imse"] != a["ipse"]:
            continue
        c, _, _ = R._exact_crossproducts(V[:, i], 31)
        g = [c[2 * j] + c[2 * j + 1] for j in range(J)]
        if any(g[j] > g[j - 1] for j in range(1, J)) or (J > 1 and g[1] * (n - 1) - 2 * c[0] > g[0] * (n - 1) - c[0]):
            continue                                                         # (a clamp in either sequence)
        used += 1
        want = n / (n - 1) * a["iact_imse"] - (4 * J - 2) / (n - 1)
        assert abs(b["tau"][0] - want) <= 16 * E.U * (abs(want) + 4 * J / (n - 1) + 2 * a["iact_imse"]), (i, b["tau"][0], want)
        assert abs(b["ess"][0] - n / want) <= 32 * E.U * n / want
        got = K.stats.pooled_ess(V[:, i].reshape(n, 1, 1), 31)
        assert got["nunits"] == 1 and abs(got["tau"][0] - want) < 1e-9 and got["bsum"][0] == 0.0 and np.isfinite(got["ess"][0])
    assert used >= 8, used


# ---------------------------------------------------------------- the surface
def test_header_and_binding_declare_the_new_symbols(klib):
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    for name in ("klara_gather_ess", "klara_selftest_ess", "klara_selftest_ess_ranks"):
        assert name in L.EXPORTS and hasattr(klib, name) and re.search(r"klara_status " + name + r"\(", hdr), name
    for name, val in (("KLARA_ESS_STREAMED", 0), ("KLARA_ESS_HISTORY", 1), ("KLARA_ESS_SPLIT", 2)):
        assert re.search(r"#define " + name + r"\s+" + str(val) + r"\b", hdr) and getattr(L, name[6:]) == val
    assert re.search(r"#define KLARA_ABI_VERSION\s+6\b", hdr) and klib.klara_abi_version() == 6
    assert klib.klara_gather_ess(None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == L.ERR_INVALID_ARG
    for name in ("pooled_ess", "pooled_iact", "allreduce_ess", "gather_engine_ess_klara"):
        assert callable(getattr(K, name)), name
    assert callable(K.Engine.pooled_ess) and callable(K.stats.pooled_ess) and callable(K.stats.ess_from_sums)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "klara_gather_ess" in (ROOT / doc).read_text(), doc


def test_julia_exports_pooledess_and_gather_ess_without_touching_klaras_names():
    jl = (ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl").read_text()
    exported = set(re.split(r"[,\s]+", re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jl, re.M).group(1)))
    assert {"pooledess", "gather_ess"} <= exported
    assert re.search(r"^pooledess\(job::HIPMCJob; split::Bool=false, maxlag::Integer=0\)", jl, re.M)
    assert re.search(r"^gather_ess\(job::HIPMCJob, comm::HIPComm; split::Bool=false, maxlag::Integer=0\)", jl, re.M)
    assert jl.count("(:klara_gather_ess, lib)") == 1
    klara = set((ROOT / "tests" / "golden" / "klara_exports.txt").read_text().split())
    assert {"ess", "iact", "mcvar", "mcse"} <= klara                         # Klara's own: neither redefined nor extended here
    assert not ({"pooledess", "gather_ess"} & klara) and not (exported & {"ess", "iact", "mcvar", "mcse"})
    assert not re.search(r"^(function )?(ess|iact|mcvar|mcse)\(", jl, re.M)


def test_selftest_refuses_bad_arguments_before_any_launch(klib):
    """No device here: every refusal below has to come before the first HIP call"""
    h = E.make_hist(5, 3, 12)
    ok = dict(hist=h, maxlag=7, splits=[12], bounds=[0, 5])
    bad = [dict(maxlag=0), dict(maxlag=128), dict(splits=[11]), dict(splits=[13]), dict(splits=[-1, 13]), dict(bounds=[0, 3, 3, 5]), dict(bounds=[1, 5]),
           dict(bounds=[0, 4]), dict(bounds=[0, 6])]
    for kw in bad:
        st, _ = E.selftest(klib, **{**ok, **kw})
        assert st == L.ERR_INVALID_ARG, kw
    sp = np.array([12], dtype=np.int64); bd = np.array([0, 5], dtype=np.int64)
    args = lambda N, D, ncols, hp, ml=7: (0, N, D, ncols, hp, ml, 1, sp.ctypes.data, 1, bd.ctypes.data, None, None, None, None, None)
    assert klib.klara_selftest_ess(*args(5, 3, 12, None)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(*args(0, 3, 12, h.ctypes.data)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(*args(-5, 3, 12, h.ctypes.data)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(*args(5, 0, 12, h.ctypes.data)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(*args(5, 1025, 12, h.ctypes.data)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(*args(5, 3, 1, h.ctypes.data)) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(0, 5, 3, 12, h.ctypes.data, 7, 1, None, 1, bd.ctypes.data, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess(0, 5, 3, 12, h.ctypes.data, 7, 1, sp.ctypes.data, 1, None, None, None, None, None, None) == L.ERR_INVALID_ARG


def test_rank_verdicts_for_equal_and_unequal_n_and_window(klib):
    def verdict(units, n, lags):
        u = np.asarray(units, dtype=np.int64); nn = np.asarray(n, dtype=np.int64); ll = np.asarray(lags, dtype=np.int32)
        return klib.klara_selftest_ess_ranks(len(u), u.ctypes.data, nn.ctypes.data, ll.ctypes.data)
    assert verdict([7], [100], [31]) == L.OK
    assert verdict([7, 1, 4096], [100, 100, 100], [31, 31, 31]) == L.OK
    assert verdict([7, 9], [0, 0], [0, 0]) == L.OK                           # before the first saved sample, everywhere
    assert verdict([7, 9], [100, 101], [31, 31]) == L.ERR_STATE              # the same window, different n: the counters' check
    assert verdict([7, 9, 3], [100, 100, 100], [31, 31, 15]) == L.ERR_STATE  # different windows: the (L, ~L) maximum
    assert verdict([7, 9], [20, 40], [19, 31]) == L.ERR_STATE                # both
    assert verdict([7, 9], [100, 100], [0, 127]) == L.ERR_STATE
    assert verdict([1 << 20, 1 << 20], [1 << 20, (1 << 20) + 1], [127, 127]) == L.ERR_STATE      # (no overflow in the squares)
    assert verdict([7], [100], [128]) == L.ERR_INVALID_ARG and verdict([0], [100], [3]) == L.ERR_INVALID_ARG
    assert klib.klara_selftest_ess_ranks(0, None, None, None) == L.ERR_INVALID_ARG


def test_python_surface_refuses_what_the_library_would():
    with pytest.raises(ValueError):
        K.Engine.pooled_ess(object(), mode="nope")
    with pytest.raises(ValueError):
        K.Engine.pooled_ess(object(), mode="streamed", maxlag=5)


# ---------------------------------------------------------------- the merge through torch.distributed
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_WORLD_CASE = (257, 3, 15, 60, 1e4, 2)             # N, D, maxlag, ncols, offset, seed
_WORLD_BOUNDS = [0, 100, 257]


def _local(rank, split=False):
    N, D, ml, ncols, off, seed = _WORLD_CASE
    hist = E.make_hist(N, D, ncols, off, seed)
    s = E.local_sums(np.ascontiguousarray(hist[:, _WORLD_BOUNDS[rank]:_WORLD_BOUNDS[rank + 1]]), ml, split)
    return {"mean": s["mean"], "wsum": s["wsum"], "bsum": s["bsum"], "csum": s["csum"], "nunits": s["m"], "nper": s["n"]}


def _worker(rank, world, port, q):
    import sys
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    import torch.distributed as dist
    import klara_jl_amd as K
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = K.allreduce_ess(_local(rank))
    out2 = K.allreduce_ess(_local(rank, split=True))
    refused = []
    uneven = _local(rank); uneven["nper"] += rank                            # the ranks disagree on the saved steps: every rank has to refuse
    shorter = _local(rank); shorter["csum"] = shorter["csum"][:, :16 - 3 * rank]      # ... and on the window
    for loc in (uneven, shorter):
        try:
            K.allreduce_ess(loc)
            refused.append(False)
        except ValueError:
            refused.append(True)
    q.put((rank, {k: np.asarray(v) for k, v in out.items()}, {k: np.asarray(v) for k, v in out2.items()}, refused))
    dist.destroy_process_group()


def test_allreduce_ess_world2_reproduces_mirror_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    N, D, ml, ncols, off, seed = _WORLD_CASE
    hist = E.make_hist(N, D, ncols, off, seed)
    for split, idx in ((False, 1), (True, 2)):
        want = E.mirror_ranks(_WORLD_BOUNDS, hist, ml, split)
        for r in res:
            assert r[3] == [True, True]
            for k in ("ess", "tau", "rho", "mean", "wsum", "bsum", "csum", "pairs"):
                assert np.array_equal(r[idx][k], want[k], equal_nan=True), (split, k)
            assert (int(r[idx]["nunits"]), int(r[idx]["nper"]), int(r[idx]["lags"])) == (want["nunits"], want["nper"], want["lags"])
    one = K.allreduce_ess(_local(0))                                         # no process group: this rank alone
    alone = E.mirror(np.ascontiguousarray(hist[:, :100]), ml)
    assert np.array_equal(one["ess"], alone["ess"]) and np.array_equal(one["pairs"], alone["pairs"])
    rebuilt = dict(_local(0)); rebuilt.pop("csum"); rebuilt["rho"] = alone["rho"]                # without csum: rebuilt from rho, to rounding
    assert np.allclose(K.allreduce_ess(rebuilt)["ess"], alone["ess"], rtol=1e-9)
