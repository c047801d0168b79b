"""Multi-GPU: chains shard across ranks, no collective on the data path.

Chains are independent (`run(job::Vector) = map(run, job)`, src/jobs/jobs.jl:212), so rank r of R owns the
block [r*N/R, (r+1)*N/R) and seeds its Philox subsequences with the GLOBAL chain id: results do not depend
on R.  The only exchange is the end-of-run merge of the pooled chain summaries: every rank holds (n_r, mean_r[D], M2_r[D]) of its
chains — formed on the device without the cancellation of sumsq/n - mean^2 (klara_gather_moments, include/klara_hip.h) — and the
ranks are merged by Chan's update in three SUM all-reduces (3 counters, D weighted means, D sums of squares): ~1.6 kB at D = 100,
latency-bound over RCCL/xGMI.  Backend "nccl" (= RCCL) on GPUs, "gloo" in the CPU tests.  No rational arithmetic, no exceptions on
non-finite sums (they propagate as NaN moments on every rank alike, so no rank can leave the collectives early).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import numpy as np


def shard_chains(nchains_total: int, rank: int, world: int) -> Tuple[int, int]:
    """Block partition -> (chain_offset, nchains_local); remainders go to the low ranks."""
    base, rem = divmod(int(nchains_total), int(world))
    count = base + (1 if rank < rem else 0)
    offset = rank * base + min(rank, rem)
    return offset, count


class KlaraComm:
    """The library's own communicator (klara_comm_*: RCCL loaded by the library, include/klara_hip.h) — what a Julia binding holds as
    `HIPComm`.  `Engine.pooled_moments(comm.handle)` / `klara_gather_moments(h, comm, ...)` is then the job's one exchange."""

    def __init__(self, lib, nranks: int, rank: int, uid: bytes, device: int):
        import ctypes as C
        from . import _lib as L
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"the communicator id has {len(uid)} bytes, expected {COMM_ID_BYTES}")
        self._lib, self.handle = lib, C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        L.check(lib.klara_comm_init(C.byref(self.handle), int(nranks), int(rank), buf, int(device)), "klara_comm_init")

    @staticmethod
    def unique_id(lib) -> bytes:
        """rank 0 only: RCCL's ncclUniqueId (128 bytes) that the caller ships to the other ranks"""
        import ctypes as C
        from . import _lib as L
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        L.check(lib.klara_comm_unique_id(buf), "klara_comm_unique_id")
        return bytes(buf)

    def info(self) -> Tuple[int, int, int]:
        """(ranks, this rank, device) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)"""
        import ctypes as C
        from . import _lib as L
        n, r, d = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(self._lib.klara_comm_info(self.handle, C.byref(n), C.byref(r), C.byref(d)), "klara_comm_info")
        return n.value, r.value, d.value

    def close(self) -> None:
        if self.handle:
            self._lib.klara_comm_destroy(self.handle)
            self.handle = None


COMM_ID_BYTES = 128         # KLARA_COMM_ID_BYTES


class CommBootstrapTimeout(RuntimeError):
    """klara_comm_init did not return by the deadline; a helper thread is still inside it (the caller should leave with os._exit)"""


def bootstrap_comm(lib, rank: int, world: int, device: int, broadcast: Callable[[Optional[bytes]], bytes],
                   timeout: Optional[float] = None) -> KlaraComm:
    """One communicator over the job's ranks: rank 0 makes the id (klara_comm_unique_id), `broadcast(id on rank 0 / None elsewhere)`
    returns rank 0's bytes on every rank — the caller's transport, used for these 128 bytes and nothing else — and every rank joins
    with its own index and device (klara_comm_init is collective: it returns when all `world` ranks have called it).
    Every rank ALWAYS takes part in the broadcast, on the calling thread (a rank 0 that could not make an id broadcasts b"": all ranks
    raise together).  With `timeout`, klara_comm_init — the one call that waits for the other ranks inside RCCL — runs on a helper
    thread and CommBootstrapTimeout is raised past the deadline."""
    uid, err = None, None
    if rank == 0:
        try:
            uid = KlaraComm.unique_id(lib)
        except Exception as exc:            # the other ranks are waiting in the broadcast: tell them
            uid, err = b"", exc
    uid = broadcast(uid)
    if err is not None:
        raise err
    if uid is None or len(uid) != COMM_ID_BYTES:
        raise RuntimeError(f"rank {rank}: the broadcast did not deliver rank 0's communicator id")
    if timeout is None:
        return KlaraComm(lib, world, rank, uid, device)
    import threading
    box = {}

    def join():
        try:
            box["comm"] = KlaraComm(lib, world, rank, uid, device)
        except Exception as exc:
            box["error"] = exc
    th = threading.Thread(target=join, daemon=True)
    th.start(); th.join(timeout=timeout)
    if th.is_alive():
        raise CommBootstrapTimeout(f"rank {rank}: klara_comm_init did not return within {timeout:.0f} s (RCCL bootstrap)")
    if "error" in box:
        raise box["error"]
    return box["comm"]


def torch_broadcast_bytes(group=None) -> Callable[[Optional[bytes]], bytes]:
    """`broadcast` for bootstrap_comm over an initialised torch.distributed group (any backend; gloo in bench.py)"""
    def bc(b: Optional[bytes]) -> bytes:
        import torch.distributed as dist
        box = [b]
        dist.broadcast_object_list(box, src=0, group=group)
        return box[0]
    return bc


def gather_engine_moments_klara(engine, comm: KlaraComm) -> Dict[str, np.ndarray]:
    """The job's one exchange through the C ABI alone: klara_gather_moments(h, comm, ...) — per-chain moments pooled on the device and
    merged over the ranks by three RCCL all-reduces on the job's stream.  Same keys as gather_engine_summaries."""
    if engine.monitor & 0x4:
        mean, m2, ns, nacc, ntr, nc = engine.pooled_moments(comm.handle)
    else:                               # no running sums: the counters alone (klara_gather_summaries with NULL sums: one all-reduce)
        import ctypes as C
        from . import _lib as L
        na, nt, nsm, nch = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(engine._lib.klara_gather_summaries(engine._h, comm.handle, None, None, C.byref(na), C.byref(nt), C.byref(nsm), C.byref(nch)),
                "klara_gather_summaries")
        mean = m2 = None; ns, nacc, ntr, nc = 0, int(na.value), int(nt.value), int(nch.value)
    out = {"naccept": float(nacc), "ntransitions": float(ntr), "nsamples": float(ns), "nchains": float(nc)}
    if ns > 0:
        out.update(mean=mean, m2=m2, var=m2 / ns, sum=mean * ns, sumsq=m2 + ns * mean ** 2)
    if ntr > 0:
        out["acceptance"] = nacc / ntr
    return out


def _two_prod(a: np.ndarray, b: np.ndarray):
    """a * b = p + e exactly (Dekker / Veltkamp splitting; numpy has no fma)."""
    p = a * b
    def split(v):
        c = 134217729.0 * v                    # 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a); bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _local_moments(s: np.ndarray, q: np.ndarray, n: float):
    """(mean, M2 = sum (x - mean)^2) per dimension from raw sums with the one cancelling subtraction, q - s^2/n, carried in
    double-double: evaluated in plain doubles it loses mean^2/var digits (rats alpha_c: mean 242, sd 2.7 -> 4 digits); this way the
    only error left is the rounding already inside the raw sums themselves.  Non-finite sums give NaN / inf moments (no exception)."""
    if n <= 0:
        return np.zeros_like(s), np.zeros_like(s)
    with np.errstate(all="ignore"):
        p, pe = _two_prod(s, s)                 # s^2 = p + pe
        qh = p / n
        t, te = _two_prod(qh, np.full_like(qh, n))
        r = (p - t) - te                        # p = qh * n + r  (p - t is exact: qh * n is within an ulp of p)
        ql = (r + pe) / n
        m2 = (q - qh) - ql
        m2 = np.where(m2 < 0.0, 0.0, m2)
        return s / n, m2


def allreduce_moments(local: Dict[str, np.ndarray], group=None, device=None) -> Dict[str, np.ndarray]:
    """Chan's merge of per-rank moments: `local` holds mean[D], m2[D], nsamples, naccept, ntransitions of this rank's chains.
    Three SUM all-reduces — (nsamples, naccept, ntransitions), n_r mean_r, M2_r + n_r (mean_r - mean)^2 — every rank takes part in
    all three whatever its values are.  The arrays may have any width: with Engine.derived_moments()'s mean[K], m2[K], nsamples (and naccept =
    ntransitions = 0) this is the merge of a derived= closure's outputs.  Works without torch.distributed initialised (single process)."""
    import torch
    import torch.distributed as dist

    mean_l = np.asarray(local["mean"], dtype=np.float64).ravel(); m2_l = np.asarray(local["m2"], dtype=np.float64).ravel()
    n_l = float(local["nsamples"])
    live = dist.is_available() and dist.is_initialized()
    if live and device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"

    def reduce_sum(buf: np.ndarray) -> np.ndarray:
        if not live:
            return buf
        t = torch.from_numpy(np.ascontiguousarray(buf)).to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t.cpu().numpy()

    cnt = reduce_sum(np.array([n_l, float(local["naccept"]), float(local["ntransitions"])], dtype=np.float64))   # (exact below 2^53)
    ns, nacc, ntr = cnt
    with np.errstate(all="ignore"):
        wsum = reduce_sum(n_l * mean_l)
        mean = wsum / ns if ns > 0 else np.zeros_like(wsum)
        m2 = reduce_sum(m2_l + n_l * (mean_l - mean) ** 2)          # Chan: within-rank + between-rank sums of squares
    out = {"naccept": nacc, "ntransitions": ntr, "nsamples": ns}
    if ns > 0:
        out["mean"] = mean
        out["m2"] = m2
        out["var"] = m2 / ns
    if ntr > 0:
        out["acceptance"] = nacc / ntr
    return out


def gather_engine_covariance_klara(engine, comm: KlaraComm) -> Dict[str, np.ndarray]:
    """The pooled covariance of every rank's chains through the C ABI alone: klara_gather_covariance(h, comm, ...) — the ranks' (n, mean, M)
    merged by three RCCL all-reduces on the job's stream.  Keys: mean[D], m2[D, D], nsamples, nchains and, from two samples on, cov."""
    mean, m2, ns, nc = engine.pooled_covariance(comm.handle)
    out = {"mean": mean, "m2": m2, "nsamples": float(ns), "nchains": float(nc)}
    if ns > 1:
        out["cov"] = m2 / (ns - 1)
    return out


def allreduce_covariance(local: Dict[str, np.ndarray], group=None, device=None) -> Dict[str, np.ndarray]:
    """Chan's merge of per-rank covariance accumulators, the D x D form of allreduce_moments: `local` holds mean[D], m2[D, D], nsamples (and
    nchains) of this rank's chains (Engine.pooled_covariance without a communicator).  Three SUM all-reduces — the counters, n_r mean_r,
    M_r + n_r d d' with d = mean_r - mean — in that order on every rank.  Works without torch.distributed initialised (single process)."""
    import torch
    import torch.distributed as dist

    mean_l = np.asarray(local["mean"], dtype=np.float64).ravel()
    D = mean_l.size
    m2_l = np.asarray(local["m2"], dtype=np.float64).reshape(D, D)
    n_l = float(local["nsamples"])
    live = dist.is_available() and dist.is_initialized()
    if live and device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"

    def reduce_sum(buf: np.ndarray) -> np.ndarray:
        if not live:
            return buf
        t = torch.from_numpy(np.ascontiguousarray(buf)).to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t.cpu().numpy()

    cnt = reduce_sum(np.array([n_l, float(local.get("nchains", 0.0))], dtype=np.float64))   # (exact below 2^53)
    ns, nc = cnt
    with np.errstate(all="ignore"):
        wsum = reduce_sum(n_l * mean_l)
        mean = wsum / ns if ns > 0 else np.zeros_like(wsum)
        d = mean_l - mean
        m2 = reduce_sum(m2_l + n_l * (d[:, None] * d[None, :]))
    out = {"nsamples": ns, "nchains": nc, "mean": mean, "m2": m2}
    if ns > 1:
        out["cov"] = m2 / (ns - 1)
    return out


def allreduce_histogram(counts, group=None, device=None) -> np.ndarray:
    """The pooled marginal histogram of every rank's chains for hosts with their own transport: `counts` is this rank's (D, nbins + 2) table
    (Engine.pooled_histogram without a communicator; every rank built with the same marginals=).  One SUM all-reduce of 64-bit integers — exact in any
    order, so the result is the unsharded table; gloo works.  A table of any height: Engine.derived_histogram()'s (K, nbins + 2) counts merge the same
    way.  Works without torch.distributed initialised (single process)."""
    import torch
    import torch.distributed as dist

    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if np.any(c >> np.uint64(63)):
        raise ValueError("counts beyond 2^63 cannot travel as int64")
    if not (dist.is_available() and dist.is_initialized()):
        return c.copy()
    if device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.cpu().numpy().view(np.uint64).reshape(c.shape)


def gather_engine_rhat_klara(engine, comm: KlaraComm, split: bool = False) -> Dict[str, np.ndarray]:
    """R-hat over every rank's chains through the C ABI alone: klara_gather_rhat(h, comm, ...) — the ranks' (chains, mean of chain means, bsum) merged as
    the moments are and wsum summed, four RCCL all-reduces on the job's stream.  Keys as Engine.rhat."""
    return engine.rhat(split=split, comm=comm.handle)


def rhat_from_sums(wsum, bsum, m, n):
    """R-hat from wsum = sum of the units' M2 and bsum = sum (unit mean - mean)^2 over m units of n samples each, as klara_gather_rhat evaluates it:
    NaN for m < 2 or n < 2, plain IEEE division otherwise (wsum = 0 with bsum > 0: inf; both zero: NaN)."""
    wsum = np.asarray(wsum, dtype=np.float64); bsum = np.asarray(bsum, dtype=np.float64)
    if m < 2 or n < 2:
        return np.full(wsum.shape, np.nan)
    m, n = float(m), float(n)
    with np.errstate(all="ignore"):
        W = wsum / (m * (n - 1.0)); Bn = bsum / (m - 1.0)
        return np.sqrt((((n - 1.0) / n) * W + Bn) / W)


def allreduce_rhat(local: Dict[str, np.ndarray], group=None, device=None) -> Dict[str, np.ndarray]:
    """klara_gather_rhat's between-rank merge through torch.distributed, for a host that brings its own transport: `local` is this rank's
    Engine.rhat() (mean[D], wsum[D], bsum[D], nchains, nper).  Four SUM all-reduces in the library's order — the counters (m_r n_r, m_r n_r^2, m_r),
    m_r mean_r, bsum_r + m_r (mean_r - mean)^2, wsum_r — entered by every rank whatever its values are.  Raises ValueError, on every rank, when the
    ranks do not hold the same number of samples per chain.  The arrays may have any width: Engine.derived_rhat()'s dict merges the same way.  Works
    without torch.distributed initialised (single process)."""
    import torch
    import torch.distributed as dist

    mean_l = np.asarray(local["mean"], dtype=np.float64).ravel(); b_l = np.asarray(local["bsum"], dtype=np.float64).ravel()
    w_l = np.asarray(local["wsum"], dtype=np.float64).ravel()
    m_l, n_l = int(local["nchains"]), int(local["nper"])
    live = dist.is_available() and dist.is_initialized()
    if live and device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"

    def reduce_sum(buf: np.ndarray) -> np.ndarray:
        if not live:
            return buf
        t = torch.from_numpy(np.ascontiguousarray(buf)).to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t.cpu().numpy()

    cnt = reduce_sum(np.array([m_l * n_l, m_l * n_l * n_l, m_l], dtype=np.int64))
    sn, sn2, m = (int(v) for v in cnt)
    with np.errstate(all="ignore"):
        wmean = reduce_sum(float(m_l) * mean_l)
        mean = wmean / float(m) if m > 0 else np.zeros_like(wmean)
        d = mean_l - mean
        bsum = reduce_sum(b_l + float(m_l) * (d * d))
        wsum = reduce_sum(w_l)
    if sn * sn != m * sn2:                                   # the n_r are all equal exactly when (sum m n)^2 = sum m * sum m n^2
        raise ValueError("allreduce_rhat: the ranks hold different numbers of saved steps")
    n = sn // m if m else 0
    if n == 0:
        z = np.zeros_like(mean)
        return {"rhat": np.full(mean.shape, np.nan), "mean": z, "wsum": z.copy(), "bsum": z.copy(), "nchains": 0, "nper": 0}
    return {"rhat": rhat_from_sums(wsum, bsum, m, n), "mean": mean, "wsum": wsum, "bsum": bsum, "nchains": m, "nper": n}


def gather_engine_ess_klara(engine, comm: KlaraComm, mode: str = "streamed", maxlag=None) -> Dict[str, np.ndarray]:
    """The pooled effective sample size over every rank's chains through the C ABI alone: klara_gather_ess(h, comm, ...) — the ranks agree on the window,
    then R-hat's merge with the lagged sums summed beside wsum, on the job's stream.  Keys as Engine.pooled_ess."""
    return engine.pooled_ess(mode=mode, maxlag=maxlag, comm=comm.handle)


def allreduce_ess(local: Dict[str, np.ndarray], group=None, device=None) -> Dict[str, np.ndarray]:
    """klara_gather_ess's between-rank merge through torch.distributed, for a host that brings its own transport: `local` holds this rank's mean[D],
    wsum[D], bsum[D], nunits, nper and csum[D, L + 1] — stats.pooled_ess returns all of them; Engine.pooled_ess does not return csum, and without it
    csum is rebuilt from rho (m n (W - (1 - rho) var+), rounded).  The library's order: a MAX all-reduce of (L, -L) — the ranks must hold the same
    window —, then R-hat's four SUM all-reduces with wsum | csum in the last; every rank enters all of them.  Raises ValueError, on every rank, when
    the ranks hold different windows or different numbers of samples per unit.  Works without torch.distributed initialised (single process)."""
    import torch
    import torch.distributed as dist
    from .stats import ess_from_sums

    mean_l = np.asarray(local["mean"], dtype=np.float64).ravel(); b_l = np.asarray(local["bsum"], dtype=np.float64).ravel()
    w_l = np.asarray(local["wsum"], dtype=np.float64).ravel()
    m_l, n_l = int(local["nunits"]), int(local["nper"])
    D = mean_l.size
    if "csum" in local:
        c_l = np.asarray(local["csum"], dtype=np.float64).reshape(D, -1)
    else:
        rho = np.asarray(local["rho"], dtype=np.float64).reshape(D, -1)
        with np.errstate(all="ignore"):
            W = w_l / (float(m_l) * (n_l - 1.0)); varp = ((n_l - 1.0) / n_l) * W + (b_l / (m_l - 1.0) if m_l > 1 else 0.0)
            c_l = float(m_l) * n_l * (W[:, None] - (1.0 - rho) * varp[:, None])
        c_l[:, 0] = w_l
    lags = c_l.shape[1] - 1
    live = dist.is_available() and dist.is_initialized()
    if live and device is None:
        device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"

    def reduce(buf: np.ndarray, op) -> np.ndarray:
        if not live:
            return buf
        t = torch.from_numpy(np.ascontiguousarray(buf)).to(device)
        dist.all_reduce(t, op=op, group=group)
        return t.cpu().numpy()

    agree = reduce(np.array([lags, -lags], dtype=np.int64), dist.ReduceOp.MAX)
    if int(agree[0]) != -int(agree[1]):                      # max L = min L: before anything whose length depends on L is exchanged
        raise ValueError("allreduce_ess: the ranks hold different windows")
    cnt = reduce(np.array([m_l * n_l, m_l * n_l * n_l, m_l], dtype=np.int64), dist.ReduceOp.SUM)
    sn, sn2, m = (int(v) for v in cnt)
    with np.errstate(all="ignore"):
        wmean = reduce(float(m_l) * mean_l, dist.ReduceOp.SUM)
        mean = wmean / float(m) if m > 0 else np.zeros_like(wmean)
        d = mean_l - mean
        bsum = reduce(b_l + float(m_l) * (d * d), dist.ReduceOp.SUM)
        x = reduce(np.concatenate([w_l, c_l.ravel()]), dist.ReduceOp.SUM)
    if sn * sn != m * sn2:
        raise ValueError("allreduce_ess: the ranks hold different numbers of saved steps")
    n = sn // m if m else 0
    wsum, csum = x[:D], x[D:].reshape(D, lags + 1)
    ess, tau, rho, pairs = ess_from_sums(csum, wsum, bsum, m, n)
    return {"ess": ess, "tau": tau, "rho": rho, "mean": mean, "wsum": wsum, "bsum": bsum, "csum": csum, "pairs": pairs,
            "window_exhausted": pairs == (max(lags - 1, 0) // 2 + 1), "nunits": m, "nper": n, "lags": lags}


def allreduce_summaries(local: Dict[str, np.ndarray], group=None, device=None) -> Dict[str, np.ndarray]:
    """The same exchange for a caller that holds pooled RAW sums: `local` = sum[D], sumsq[D], naccept, ntransitions, nsamples of this
    rank's chains.  Returns the global sums plus the posterior moments (mean, var) and the acceptance rate; the variance comes from
    per-rank (n, mean, M2) (_local_moments) merged by allreduce_moments, never from sumsq/n - mean^2 of the reduced sums."""
    import torch
    import torch.distributed as dist

    s_l = np.asarray(local["sum"], dtype=np.float64).ravel(); q_l = np.asarray(local["sumsq"], dtype=np.float64).ravel()
    n_l = float(local["nsamples"])
    mean_l, m2_l = _local_moments(s_l, q_l, n_l)
    out = allreduce_moments({"mean": mean_l, "m2": m2_l, "nsamples": n_l, "naccept": local["naccept"],
                             "ntransitions": local["ntransitions"]}, group=group, device=device)
    live = dist.is_available() and dist.is_initialized()
    if live:
        if device is None:
            device = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.from_numpy(np.concatenate([s_l, q_l])).to(device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        sq = t.cpu().numpy()
    else:
        sq = np.concatenate([s_l, q_l])
    d = s_l.size
    out["sum"], out["sumsq"] = sq[:d], sq[d:]
    return out


def gather_engine_summaries(engine, group=None) -> Dict[str, np.ndarray]:
    """Pooled summaries of this rank's Engine merged over the job's ranks: the rank's moments come from the device
    (Engine.pooled_moments -> klara_gather_moments with no communicator), the merge is allreduce_moments."""
    with_sums = bool(engine.monitor & 0x4)
    if with_sums:
        mean, m2, ns, nacc, ntr, _ = engine.pooled_moments()
    else:
        _, _, nacc, ntr, _ = engine.pooled_summaries(with_sums=False)
        mean = m2 = np.zeros(engine.ndims); ns = 0
    out = allreduce_moments({"mean": mean, "m2": m2, "nsamples": ns, "naccept": nacc, "ntransitions": ntr}, group=group)
    if "mean" in out:                       # the raw sums a caller of the previous form reads, derived (the moments are the product)
        out["sum"] = out["mean"] * out["nsamples"]
        out["sumsq"] = out["m2"] + out["nsamples"] * out["mean"] ** 2
    return out
