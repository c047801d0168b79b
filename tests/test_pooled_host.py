"""The references of the across-chain reductions (tests/pooled_ref.py) against each other, on the CPU: the NumPy restatement of the device's order of
operations against exact rational arithmetic within the derived bound, at every shape and offset tests/test_gpu_pooled.py runs on the device; its
building blocks against exact products; and klara_jl_amd.distributed's host-side versions of the same arithmetic against it bit for bit."""
import functools
import os
import socket
from fractions import Fraction

import numpy as np
import pytest

import pooled_ref as R
from klara_jl_amd import distributed as DI

CHAINS = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 3077)
DIMS = (1, 127, 128, 129, 255, 256, 257, 1024)
N_WIDE, NS_WIDE = 1025, 8          # the D cases: few saved steps keep the 1025 x 1024 inputs cheap; no kernel path depends on nsaved >= 2


def exact_cols(D):
    """at most eight columns of a wide case: the first, the last, and those around the second trip of the j += 256 loops"""
    return sorted({j for j in (0, 1, 127, 128, 255, 256, 257, D - 1) if j < D})[:8] if D > 8 else list(range(D))


@functools.lru_cache(maxsize=None)
def case(N, D, nsaved, offset):
    inp = R.make_inputs(N, D, nsaved, offset)
    return inp, R.exact(inp, exact_cols(D))


def check_margins(inp, ex):
    if inp["nsaved"] >= 2:
        margin = R.MARGIN_200 if inp["nsaved"] >= 200 else R.MARGIN
        assert ex["min_chain_m2"].min() >= 0.0 and ex["min_chain_m2_pos"].min() > margin, (ex["min_chain_m2"].min(), ex["min_chain_m2_pos"].min())


def errors(mean, m2, ex, N, ranks=1):
    """(relative M2 error, its bound, mean error, its bound) over ex's columns"""
    cols = ex["cols"]
    bm2, bmean = R.bound(N, ex, ranks)
    assert np.all(bm2 <= R.CAP), bm2.max()
    with np.errstate(all="ignore"):
        e = np.where(ex["M2"] > 0, np.abs(m2[cols] - ex["M2"]) / ex["M2"], np.abs(m2[cols]))
    return e, bm2, np.abs(mean[cols] - ex["mean"]), bmean


def test_exact_error_products_are_exact():
    """The two fma of k_moments_stage1 as the mirror writes them (Dekker products) against the correctly rounded exact value, on the tests' own sums
    (every offset) and on full-mantissa values."""
    vals = [R.clamp_inputs(64, 3, off)["sum"].ravel() for off in R.OFFSETS]
    vals += [R.chain_view(case(257, 3, 200, off)[0])[0].ravel() for off in R.OFFSETS]
    for s in vals:
        for ns in (1.0, 2.0, 7.0, 200.0):
            p = s * s
            pe = R.fma_square_error(s, p)
            qh = p / ns
            r = R.fma_remainder(qh, ns, p)
            for i in range(0, s.size, 7):
                assert pe[i] == float(Fraction(float(s[i])) * Fraction(float(s[i])) + Fraction(float(-p[i])))
                assert r[i] == float(Fraction(float(-qh[i])) * Fraction(ns) + Fraction(float(p[i])))
                assert Fraction(float(p[i])) + Fraction(float(pe[i])) == Fraction(float(s[i])) ** 2          # the square's error is exact, not just rounded


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_mirror_within_the_bound_of_exact_at_every_chain_count(offset):
    """N over every grid edge of the two stages, D = 3, 200 saved steps: |mirror - exact| inside bound(), the bound inside CAP, 1e-12 up to 242 sd (what
    the rats test asserts on the device), the sums and the accept total; every chain's exact M2 above the margin (or exactly 0: a chain that never moved).
    Prints the largest error / bound: pooled_ref.MEASURED holds these figures."""
    worst = [0.0, 0.0, 0.0]
    for N in CHAINS + (2051,):
        inp, ex = case(N, 3, 200, offset)
        check_margins(inp, ex)
        mean, m2 = R.mirror(inp)
        e, bm2, em, bmean = errors(mean, m2, ex, N)
        assert np.all(e <= bm2) and np.all(em <= bmean), (N, e.max(), bm2.max(), em.max(), bmean.max())
        if offset <= 242.0:
            assert np.all(e <= 1e-12)
        worst = [max(worst[0], (e / bm2).max()), max(worst[1], (em / bmean).max()), max(worst[2], e.max())]
        s, q, acc = R.mirror_summaries(inp)
        assert acc == ex["accept"] and (N < 5 or acc > 2 ** 32)
        assert np.all(np.abs(s - ex["S"]) <= 8 * R.merge_depth(N) * R.U * np.abs(ex["S"]) + 1e-300) and np.all(np.abs(q - ex["Q"]) <= 8 * R.merge_depth(N) * R.U * ex["Q"])
    print(f"pooled offset={offset:g} sd: M2 error / bound {worst[0]:.3g}, mean error / bound {worst[1]:.3g}, worst relative M2 error {worst[2]:.3g}")
    got = R.MEASURED[offset]
    assert all(w <= 2.0 * g for w, g in zip(worst, got)), (worst, got)          # (the docstring's figures still describe these inputs)


@pytest.mark.parametrize("D", DIMS)
def test_mirror_within_the_bound_of_exact_at_every_width(D):
    """D up to 1,024 (a second, third and fourth trip of the j += 256 loops) at 1,025 chains, offsets 0 and 1e6 sd; exact on at most eight columns."""
    for offset in (0.0, 1e6):
        inp, ex = case(N_WIDE, D, NS_WIDE, offset)
        check_margins(inp, ex)
        mean, m2 = R.mirror(inp)
        e, bm2, em, bmean = errors(mean, m2, ex, N_WIDE)
        assert np.all(e <= bm2) and np.all(em <= bmean), (D, offset, e.max(), bm2.max())
        assert np.all(np.isfinite(mean)) and np.all(m2 > 0)


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_mirror_few_saved_steps(offset):
    """nsaved = 2 (the smallest with a variance) and nsaved = 1 at the clamp, where q - s^2 is the rounding error of a square with either sign (up to
    1e4 sd)."""
    for N in (3, 1025):
        inp, ex = case(N, 3, 2, offset)
        check_margins(inp, ex)
        mean, m2 = R.mirror(inp)
        e, bm2, em, bmean = errors(mean, m2, ex, N)
        assert np.all(e <= bm2) and np.all(em <= bmean)
    if offset > 1e4:
        return          # (at 1e6 sd what the clamp removes from such sums, u (mean / sd)^2 per chain, takes the bound past CAP: not an input to use)
    inp = R.clamp_inputs(1025, 3, offset)
    ex = R.exact(inp)
    assert ex["min_chain_m2"].min() < 0.0                 # at the clamp on purpose
    mc, m2c = R.chain_moments(*R.chain_view(inp), 1.0)
    assert np.all(m2c >= 0.0) and (m2c == 0.0).any() and (m2c > 0.0).any()
    mean, m2 = R.mirror(inp)
    e, bm2, em, bmean = errors(mean, m2, ex, 1025)
    assert np.all(e <= bm2) and np.all(em <= bmean), (e.max(), bm2.max())


def test_mirror_no_saved_step_gives_zeros():
    for N in (1, 300, 1025):
        inp = R.make_inputs(N, 3, 0)
        mean, m2 = R.mirror(inp)
        assert np.all(mean == 0.0) and np.all(m2 == 0.0)
        rm, rq, cnt = R.mirror_ranks(inp, R.splits(N)["2"] if N > 1 else [0, 1])
        assert np.all(rm == 0.0) and np.all(rq == 0.0) and cnt[1] == 0 and cnt[2] == N
        assert np.all(np.array(DI._local_moments(inp["sum"], inp["sumsq"], 0)) == 0.0)


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_mirror_ranks_within_the_bound_of_exact_of_the_whole(offset):
    """2,051 chains cut into 1, 2, 3 and 5 shards as shard_chains cuts them, and unequally (1 | N - 1, N - 1 | 1, 1 | 1 | N - 2, 1025 | rest): the
    between-rank merge against exact of all the chains.  Here mean_r - mean is not zero, unlike through a one-rank communicator."""
    N = 2051
    inp, ex = case(N, 3, 200, offset)
    for name, b in R.splits(N).items():
        mean, m2, cnt = R.mirror_ranks(inp, b)
        e, bm2, em, bmean = errors(mean, m2, ex, N, ranks=len(b) - 1)
        assert np.all(e <= bm2) and np.all(em <= bmean), (name, e.max(), bm2.max())
        if offset <= 242.0:
            assert np.all(e <= 1e-12)
        assert cnt == (ex["accept"], 200 * N, N)
    assert R.shard_bounds(N, 3) == [0] + [o + c for o, c in (DI.shard_chains(N, r, 3) for r in range(3))]


def test_local_moments_is_the_mirrors_per_chain_step():
    """distributed._local_moments (the host's q - s^2 / n in double-double) bit for bit against chain_moments, the device's per-chain step."""
    for off in R.OFFSETS:
        for inp in (case(257, 3, 200, off)[0], case(1025, 3, 2, off)[0], R.clamp_inputs(300, 3, off)):
            s, q = R.chain_view(inp)
            ns = float(inp["nsaved"])
            mean, m2 = DI._local_moments(s, q, ns)
            rm, rq = R.chain_moments(s, q, ns)
            assert np.array_equal(mean, rm) and np.array_equal(m2, rq)


def _shard_moments(inp, bounds):
    out = []
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        mean, m2 = R.mirror(R.slice_inputs(inp, c0, c1))
        out.append({"mean": mean, "m2": m2, "nsamples": inp["nsaved"] * (c1 - c0), "naccept": int(inp["naccept"][c0:c1].sum() % 2 ** 52),
                    "ntransitions": 300 * (c1 - c0)})
    return out


def _ordered_allreduce(monkeypatch, locals_):
    """allreduce_moments of every rank in one process: torch.distributed's all_reduce replaced by the sum over the ranks' buffers in ascending order from
    0.0.  A rank's k-th buffer depends on the reduced buffers before it, so the ranks are run once per collective, each run replaying what is known."""
    import torch
    import torch.distributed as dist
    known = []
    state = {}

    def fake(t, op=None, group=None):
        k = state["k"]
        state["k"] += 1
        if k < len(known):
            t.copy_(known[k])
        else:
            state["rec"].setdefault(k, t.clone())
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_backend", lambda group=None: "gloo")
    monkeypatch.setattr(dist, "all_reduce", fake)
    outs = None
    for _ in range(4):
        recs, outs = [], []
        for loc in locals_:
            state.update(k=0, rec={})
            outs.append(DI.allreduce_moments(loc))
            recs.append(state["rec"])
        k = len(known)
        if k in recs[0]:
            tot = torch.zeros_like(recs[0][k])
            for r in recs:
                tot = tot + r[k]
            known.append(tot)
    assert len(known) == 3
    return outs


@pytest.mark.parametrize("offset", (0.0, 1e6))
def test_allreduce_moments_is_the_mirrors_between_rank_step_in_one_process(offset, monkeypatch):
    N = 2051
    inp, _ = case(N, 3, 200, offset)
    for name in ("2", "3", "5", "1|N-1", "1|1|N-2"):
        b = R.splits(N)[name]
        mean, m2, cnt = R.mirror_ranks(inp, b)
        for out in _ordered_allreduce(monkeypatch, _shard_moments(inp, b)):
            assert np.array_equal(out["mean"], mean) and np.array_equal(out["m2"], m2), name
            assert out["nsamples"] == cnt[1]


def _gloo_worker(rank, world, port, q):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root)); sys.path.insert(0, str(root / "tests"))
    import torch.distributed as dist
    import klara_jl_amd as K
    import pooled_ref as R2
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = []
    for off in (0.0, 1e6):
        inp = R2.make_inputs(2051, 3, 200, off)
        for b in ([0, 1026, 2051], [0, 1, 2051]):
            loc = _shard_moments(inp, b)[rank]
            out = K.allreduce_moments(loc)
            res.append((out["mean"], out["m2"], out["nsamples"]))
    q.put((rank, res))
    dist.destroy_process_group()


def test_allreduce_moments_is_the_mirrors_between_rank_step_over_gloo_world2():
    """the same over a real process group of two ranks (a two-term sum has one order)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = []
    for off in (0.0, 1e6):
        inp, _ = case(2051, 3, 200, off)
        for b in ([0, 1026, 2051], [0, 1, 2051]):
            want.append(R.mirror_ranks(inp, b))
    for rank, res in got:
        for (mean, m2, ns), (wm, wq, cnt) in zip(res, want):
            assert np.array_equal(mean, wm) and np.array_equal(m2, wq) and ns == cnt[1], rank
