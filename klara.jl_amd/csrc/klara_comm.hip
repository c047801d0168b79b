// klara_comm.hip — RCCL summary all-reduce behind the C ABI (librccl.so loaded lazily; see include/klara_hip.h): the gather calls of the pooled
// summaries, moments, covariance and R-hat, and the rank-local steps of their one between-rank merge (klara_merge.h)
#include <rccl/rccl.h>      // types only: librccl.so is dlopen'ed on first use (klara_comm_*)
#include <dlfcn.h>
#include <new>
#include "klara_handle.h"
#include "klara_rhat.h"
#include "klara_ess.h"
#include "klara_marg_host.h"

struct klara_comm {
    void* dl = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0, device = 0;
    double* buf = nullptr; size_t cap = 0;                      // device staging of a gather call (klara_merge.h MergeLayout)
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
};
static void* rccl_dl()
{
    static void* dl = nullptr;
    if (!dl) dl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!dl) dl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!dl) dl = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    return dl;
}
extern "C" klara_status klara_comm_unique_id(uint8_t id[KLARA_COMM_ID_BYTES])
{
    static_assert(KLARA_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id) return KLARA_ERR_INVALID_ARG;
    void* dl = rccl_dl();
    if (!dl) return KLARA_ERR_UNSUPPORTED;
    auto get = reinterpret_cast<ncclResult_t (*)(ncclUniqueId*)>(dlsym(dl, "ncclGetUniqueId"));
    ncclUniqueId u;
    if (!get || get(&u) != ncclSuccess) return KLARA_ERR_HIP;
    memcpy(id, u.internal, KLARA_COMM_ID_BYTES);
    return KLARA_OK;
}
extern "C" klara_status klara_comm_init(klara_comm** out, int32_t nranks, int32_t rank, const uint8_t id[KLARA_COMM_ID_BYTES],
                                        int32_t device)
{
    if (!out || !id || nranks <= 0 || rank < 0 || rank >= nranks) return KLARA_ERR_INVALID_ARG;
    void* dl = rccl_dl();
    if (!dl) return KLARA_ERR_UNSUPPORTED;
    HIPCHK(hipSetDevice(device));
    auto init = reinterpret_cast<ncclResult_t (*)(ncclComm_t*, int, ncclUniqueId, int)>(dlsym(dl, "ncclCommInitRank"));
    klara_comm* c = new (std::nothrow) klara_comm();
    if (!c) return KLARA_ERR_NOMEM;
    c->dl = dl; c->nranks = nranks; c->rank = rank; c->device = device;
    c->AllReduce = reinterpret_cast<decltype(c->AllReduce)>(dlsym(dl, "ncclAllReduce"));
    c->CommDestroy = reinterpret_cast<decltype(c->CommDestroy)>(dlsym(dl, "ncclCommDestroy"));
    c->CommCount = reinterpret_cast<decltype(c->CommCount)>(dlsym(dl, "ncclCommCount"));
    c->CommUserRank = reinterpret_cast<decltype(c->CommUserRank)>(dlsym(dl, "ncclCommUserRank"));
    ncclUniqueId u;
    memcpy(u.internal, id, KLARA_COMM_ID_BYTES);
    if (!init || !c->AllReduce || !c->CommDestroy || init(&c->comm, nranks, u, rank) != ncclSuccess) { delete c; return KLARA_ERR_HIP; }
    *out = c;
    return KLARA_OK;
}
// what the communicator itself says it is (ncclCommCount / ncclCommUserRank), not what the caller passed to klara_comm_init
extern "C" klara_status klara_comm_info(klara_comm* c, int32_t* nranks, int32_t* rank, int32_t* device)
{
    if (!c || !c->comm) return KLARA_ERR_INVALID_ARG;
    if (!c->CommCount || !c->CommUserRank) return KLARA_ERR_UNSUPPORTED;
    int n = 0, r = 0;
    if (c->CommCount(c->comm, &n) != ncclSuccess || c->CommUserRank(c->comm, &r) != ncclSuccess) return KLARA_ERR_HIP;
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (device) *device = c->device;
    return KLARA_OK;
}
extern "C" klara_status klara_comm_destroy(klara_comm* c)
{
    if (!c) return KLARA_ERR_INVALID_ARG;
    hipSetDevice(c->device);
    if (c->comm) c->CommDestroy(c->comm);
    if (c->buf) (void)dfree(c->buf);
    delete c;
    return KLARA_OK;
}
// grow c->buf to n doubles
static hipError_t comm_reserve(klara_comm* c, size_t n)
{
    if (c->cap >= n) return hipSuccess;
    if (c->buf) (void)dfree(c->buf);
    c->buf = nullptr; c->cap = 0;
    const hipError_t e = dalloc(&c->buf, n);
    if (e == hipSuccess) c->cap = n;
    return e;
}
// A gather call's fixed sequence of collectives on c->buf: a rank that returned at its first local failure would leave the others waiting in
// theirs.  Local errors are remembered, every collective is still entered, the status is reported after the last one (finish).
struct CommSeq {
    klara_comm* c; hipStream_t st; bool bad = false;
    void H(hipError_t e) { if (e != hipSuccess) bad = true; }
    bool reduce(size_t off, size_t n, bool is_u64, ncclRedOp_t op = ncclSum)     // in-place all-reduce of c->buf[off, off + n) on the job's stream — latency-bound
    {
        void* p = c->buf + off;
        const bool ok = c->AllReduce(p, p, n, is_u64 ? ncclUint64 : ncclDouble, op, c->comm, st) == ncclSuccess;
        if (!ok) bad = true;
        return ok;
    }
    bool finish(std::vector<double>& host)                      // the head of c->buf to the host; false: something failed on the way
    {
        H(hipMemcpyAsync(host.data(), c->buf, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        H(hipStreamSynchronize(st));
        return !bad;
    }
    bool finish(void* host, size_t bytes)                       // ... the same for a buffer of 64-bit integer words
    {
        H(hipMemcpyAsync(host, c->buf, bytes, hipMemcpyDeviceToHost, st));
        H(hipStreamSynchronize(st));
        return !bad;
    }
};
// the counters of a gather call in MergeLayout's slots (the accept total comes from the device)
static void local_counters(const klara_handle* h, long long nsaved, unsigned long long cnt[MergeLayout::NCOUNTERS])
{
    const unsigned long long N = (unsigned long long)h->d.nchains;
    cnt[MergeLayout::ACCEPTED] = 0; cnt[MergeLayout::TRANSITIONS] = (unsigned long long)h->steps_done * N;
    cnt[MergeLayout::SAMPLES] = (unsigned long long)nsaved * N; cnt[MergeLayout::CHAINS] = N;
}

extern "C" klara_status klara_gather_summaries(klara_handle* h, klara_comm* c, double* sum, double* sumsq, uint64_t* naccept,
                                               uint64_t* ntransitions, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h || !c) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    if ((sum || sumsq) && !h->sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t D = (size_t)h->d.ndims;
    const MergeLayout L{ D, D };                                // no merge here: sum | sumsq | 4 counters, the layout's head up to wsum
    HIPCHK(comm_reserve(c, L.wsum()));
    CommSeq q{ c, h->stream };
    q.H(hipMemsetAsync(c->buf, 0, L.wsum() * sizeof(double), h->stream));
    q.H(pool_summaries_async(h, h->sum != nullptr, c->buf));
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    local_counters(h, h->nsaved, cnt);
    q.H(hipMemcpyAsync(c->buf + L.counters() + 1, cnt + 1, 3 * sizeof(cnt[0]), hipMemcpyHostToDevice, h->stream));
    q.reduce(0, L.counters(), false);
    q.reduce(L.counters(), MergeLayout::NCOUNTERS, true);
    std::vector<double> host(L.wsum());
    if (!q.finish(host)) return KLARA_ERR_HIP;
    if (sum) memcpy(sum, host.data(), D * sizeof(double));
    if (sumsq) memcpy(sumsq, host.data() + D, D * sizeof(double));
    memcpy(cnt, host.data() + L.counters(), sizeof(cnt));
    if (naccept) *naccept = cnt[MergeLayout::ACCEPTED];
    if (ntransitions) *ntransitions = cnt[MergeLayout::TRANSITIONS];
    if (nsamples) *nsamples = cnt[MergeLayout::SAMPLES];
    if (nchains) *nchains = cnt[MergeLayout::CHAINS];
    return KLARA_OK;
}

// ---- the rank-local steps of the between-rank merge (klara_merge.h): n_r mean_r, to be summed over the ranks ...
__global__ void k_scale(double* __restrict__ dst, const double* __restrict__ src, double f, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[j] = f * src[j];
}
// ... and, with wsum and ntot summed: mean = wsum / ntot, M += n_r d_i d_j with d = mean_r - mean.  K = D D: every (i, j) of the matrix; K = D: its
// diagonal, d_i and d_j the same value
__global__ __launch_bounds__(256) void k_merge_between(double* __restrict__ M, const double* __restrict__ mean_r, const double* __restrict__ wsum,
                                                       const unsigned long long* __restrict__ ntot, double n_r, int D, int K, double* __restrict__ mean_out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= K) return;
    const int i = K == D ? idx : idx / D, j = K == D ? idx : idx - i * D;
    const double nt = (double)*ntot;                            // (no saved sample on any rank: zeros, as chan_merge leaves them without a communicator)
    const double mi = nt > 0.0 ? wsum[i] / nt : 0.0, mj = nt > 0.0 ? wsum[j] / nt : 0.0;
    const double di = mean_r[i] - mi, dj = mean_r[j] - mj;
    if (i == j) mean_out[i] = mi;
    M[idx] = M[idx] + n_r * (di * dj);
}
hipError_t merge_scale_async(hipStream_t st, const MergeLayout& L, double* buf, double n_r)
{
    return klara_start(k_scale, dim3((unsigned)((L.D + 255) / 256)), dim3(256), 0, st, buf + L.wsum(), buf + L.mean_r(), n_r, (int)L.D);
}
hipError_t merge_between_async(hipStream_t st, const MergeLayout& L, double* buf, double n_r)
{
    const unsigned long long* ntot = reinterpret_cast<const unsigned long long*>(buf + L.counters()) + MergeLayout::SAMPLES;
    return klara_start(k_merge_between, dim3((unsigned)((L.K + 255) / 256)), dim3(256), 0, st, buf + L.M(), buf + L.mean_r(), buf + L.wsum(), ntot, n_r,
                       (int)L.D, (int)L.K, buf + L.mean());
}
// the merge of this rank's staged mean_r | M_r | counters in c->buf with the other ranks', then the whole buffer to the host and the summed counters to cnt
static bool comm_merge(CommSeq& q, const MergeLayout& L, unsigned long long cnt[MergeLayout::NCOUNTERS], std::vector<double>& host)
{
    double* buf = q.c->buf;
    const double n_r = (double)cnt[MergeLayout::SAMPLES];
    if (!merge_ranks(q.st, L, 1, &buf, &n_r, [&](size_t off, size_t n, bool is_u64) { return q.reduce(off, n, is_u64); })) q.bad = true;
    if (q.finish(host)) memcpy(cnt, host.data() + L.counters(), MergeLayout::NCOUNTERS * sizeof(cnt[0]));
    return !q.bad;
}

klara_status gather_moments_arrays(klara_handle* h, klara_comm* c, int W, const double* sum, const double* sumsq, const double* X, const long long* held,
                                   const unsigned long long* naccept, long long nsaved, double* partial, double* out, double* mean, double* m2,
                                   uint64_t* nsamples, uint64_t* naccept_out, uint64_t* ntransitions, uint64_t* nchains)
{
    const size_t D = (size_t)W;
    const long long N = (long long)h->d.nchains;
    const MergeLayout L{ D, D };
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    local_counters(h, nsaved, cnt);
    std::vector<double> host(L.size());
    if (!c) {                                                               // this handle's chains only: mean | M2 | accept total
        HIPCHK(pool_moments_async(h->stream, sum, sumsq, X, held, naccept, N, W, nsaved, partial, out));
        HIPCHK(hipMemcpyAsync(host.data(), out, (L.counters() + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(&cnt[0], host.data() + L.counters(), sizeof(cnt[0]));
    } else {
        HIPCHK(comm_reserve(c, L.size()));
        CommSeq q{ c, h->stream };
        q.H(pool_moments_async(h->stream, sum, sumsq, X, held, naccept, N, W, nsaved, partial, c->buf));       // mean_r | M2_r | accept total = counter slot 0
        q.H(hipMemcpyAsync(c->buf + L.counters() + 1, cnt + 1, 3 * sizeof(cnt[0]), hipMemcpyHostToDevice, h->stream));
        if (!comm_merge(q, L, cnt, host)) return KLARA_ERR_HIP;
    }
    if (mean) memcpy(mean, host.data() + (c ? L.mean() : L.mean_r()), D * sizeof(double));
    if (m2) memcpy(m2, host.data() + L.M(), D * sizeof(double));
    if (naccept_out) *naccept_out = cnt[MergeLayout::ACCEPTED];
    if (ntransitions) *ntransitions = cnt[MergeLayout::TRANSITIONS];
    if (nsamples) *nsamples = cnt[MergeLayout::SAMPLES];
    if (nchains) *nchains = cnt[MergeLayout::CHAINS];
    return KLARA_OK;
}

extern "C" klara_status klara_gather_moments(klara_handle* h, klara_comm* c, double* mean, double* m2, uint64_t* nsamples,
                                             uint64_t* naccept, uint64_t* ntransitions, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    return gather_moments_arrays(h, c, h->d.ndims, h->sum, h->sumsq, h->X, h->held, h->naccept, (long long)h->nsaved, h->pool_partial, h->pooled_out, mean, m2,
                                 nsamples, naccept, ntransitions, nchains);
}

// The pooled covariance (klara_cov.h): this rank's (mean_r, M_r) from its accumulators, then — with a communicator — the D x D form of the same merge
extern "C" klara_status klara_gather_covariance(klara_handle* h, klara_comm* c, double* mean, double* m2, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->cov_S) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t D = (size_t)h->d.ndims, DD = D * D;
    const MergeLayout L{ D, DD };
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    local_counters(h, h->cov_n, cnt);
    const double n_r = (double)cnt[MergeLayout::SAMPLES];
    std::vector<double> host(L.size());
    // this rank's mean | M (before the first saved sample: zeros)
    const auto local = [&](double* out) -> hipError_t {
        if (h->cov_n == 0) return hipMemsetAsync(out, 0, (D + DD) * sizeof(double), h->stream);
        return klara_cov_launch_finalize(h->cov, h->cov_S, h->cov_T, h->cov_pivot, n_r, out, h->stream);
    };
    if (!c) {
        HIPCHK(local(h->cov_out));
        HIPCHK(hipMemcpyAsync(host.data(), h->cov_out, (D + DD) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        HIPCHK(comm_reserve(c, L.size()));
        CommSeq q{ c, h->stream };
        q.H(local(c->buf));
        q.H(hipMemcpyAsync(c->buf + L.counters(), cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream));
        if (!comm_merge(q, L, cnt, host)) return KLARA_ERR_HIP;
    }
    if (mean) memcpy(mean, host.data() + (c ? L.mean() : L.mean_r()), D * sizeof(double));
    if (m2) memcpy(m2, host.data() + L.M(), DD * sizeof(double));
    if (nsamples) *nsamples = cnt[MergeLayout::SAMPLES];
    if (nchains) *nchains = cnt[MergeLayout::CHAINS];
    return KLARA_OK;
}

// The pooled marginal histograms (klara_marg.h): the table is only read.  With a communicator the staging buffer is, in 64-bit words,
//   v [NV] | ~v [NV] | counts [D (nbins + 2)] | saved samples, chains,     NV = 2 D + 1, v = nbins and the bit patterns of lo and hi (klara_marg_host.h)
// and the call is two steps.  (1) An integer maximum all-reduce over v | ~v, read back and waited for: max(~v) = ~min(v), so the ranks' parameters are the
// same exactly when max(v) = ~max(~v) in every word (klara_marg_words_agree).  Every rank evaluates that on the same reduced values, so either all go on or
// all return KLARA_ERR_STATE here — before the sum, whose length D (nbins + 2) would differ between ranks that differ in nbins.  (2) The 64-bit integer sum
// of the counts and the two counters.  A local HIP failure before (1) is remembered and (1) is still entered; a rank that cannot read (1)'s result back
// cannot know what the others decided and returns KLARA_ERR_HIP without entering (2).  NV comes from this rank's D: ranks of different ndims are not one job.
klara_status gather_histogram_arrays(klara_handle* h, klara_comm* c, int W, const KMargGeom& geom, const unsigned long long* table, long long nsaved,
                                     const double* lohi, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains)
{
    const size_t D = (size_t)W, K = klara_marg_count_elems(geom), NV = 2 * D + 1;
    const uint64_t cnt[2] = { (uint64_t)nsaved * (uint64_t)h->d.nchains, (uint64_t)h->d.nchains };
    std::vector<uint64_t> host(K + 2);                          // counts | saved samples, chains
    if (!c) {
        HIPCHK(hipMemcpyAsync(host.data(), table, K * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(host.data() + K, cnt, sizeof(cnt));
    } else {
        HIPCHK(comm_reserve(c, 2 * NV + K + 2));
        std::vector<uint64_t> v(2 * NV);
        klara_marg_agreement_words(geom.nbins, lohi, lohi + D, (int32_t)D, v.data());
        CommSeq q{ c, h->stream };
        q.H(hipMemcpyAsync(c->buf, v.data(), v.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        q.reduce(0, 2 * NV, true, ncclMax);
        if (!q.finish(v.data(), v.size() * sizeof(uint64_t))) return KLARA_ERR_HIP;
        if (!klara_marg_words_agree(v.data(), NV)) return KLARA_ERR_STATE;      // the same verdict on every rank: none enters the sum
        q.H(hipMemcpyAsync(c->buf + 2 * NV, table, K * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
        q.H(hipMemcpyAsync(c->buf + 2 * NV + K, cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream));
        q.reduce(2 * NV, K + 2, true);
        q.H(hipMemcpyAsync(host.data(), c->buf + 2 * NV, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        q.H(hipStreamSynchronize(h->stream));
        if (q.bad) return KLARA_ERR_HIP;
    }
    if (counts) memcpy(counts, host.data(), K * sizeof(uint64_t));
    if (nsamples) *nsamples = host[K];
    if (nchains) *nchains = host[K + 1];
    return KLARA_OK;
}

extern "C" klara_status klara_gather_histogram(klara_handle* h, klara_comm* c, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->marg_counts) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    return gather_histogram_arrays(h, c, h->d.ndims, h->marg, h->marg_counts, h->marg_n, h->marg_host.data(), counts, nsamples, nchains);
}

// ---- the Gelman–Rubin diagnostic (klara_rhat.h): the same merge with units (chains, or half-chains) where the samples stand — rank r stages the mean of
// its units' means, Bsum_r and Wsum_r — and, after it, R-hat from the totals on the host
void rhat_counters(unsigned long long m, unsigned long long n, unsigned long long cnt[MergeLayout::NCOUNTERS])
{
    cnt[MergeLayout::UNIT_SAMPLES] = m * n; cnt[MergeLayout::UNIT_SAMPLES_SQ] = m * n * n; cnt[MergeLayout::UNITS] = m; cnt[MergeLayout::CHAINS] = 0;
}
klara_status rhat_finish(size_t D, const double* host, bool merged, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* units, int64_t* nper)
{
    const MergeLayout L{ D, D, D };
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    memcpy(cnt, host + L.counters(), sizeof(cnt));
    const unsigned long long m = cnt[MergeLayout::UNITS], sn = cnt[MergeLayout::UNIT_SAMPLES], sn2 = cnt[MergeLayout::UNIT_SAMPLES_SQ];
    // every rank evaluates this on the same three sums: the same status everywhere
    if ((unsigned __int128)sn * sn != (unsigned __int128)m * sn2) return KLARA_ERR_STATE;
    const unsigned long long n = m ? sn / m : 0;
    const bool none = n == 0;                                               // before the first saved sample: NaN and zeros
    const double* mu = host + (merged ? L.mean() : L.mean_r());
    for (size_t j = 0; j < D; ++j) {
        if (rhat) rhat[j] = none ? (double)NAN : rhat_value(host[L.extra() + j], host[L.M() + j], (double)m, (double)n);
        if (mean) mean[j] = none ? 0.0 : mu[j];
        if (wsum) wsum[j] = none ? 0.0 : host[L.extra() + j];
        if (bsum) bsum[j] = none ? 0.0 : host[L.M() + j];
    }
    if (units) *units = none ? 0 : m;
    if (nper) *nper = (int64_t)n;
    return KLARA_OK;
}

klara_status gather_rhat_arrays(klara_handle* h, klara_comm* c, int32_t split, int W, const double* sum, const double* sumsq, const double* X,
                                const long long* held, long long nsaved, double** ws, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* nchains,
                                int64_t* nper)
{
    const int D = W;
    const long long N = h->d.nchains;
    const MergeLayout L{ (size_t)D, (size_t)D, (size_t)D };
    if (!*ws) HIPCHK(h->mem.alloc(ws, klara_rhat_partial_elems(D) + L.size()));
    if (split && !h->rhat_half) HIPCHK(h->mem.alloc(&h->rhat_half, (size_t)4 * (size_t)N * (size_t)D));
    // units and samples per unit.  A split of 1 to 3 saved steps is refused, but only after the reductions: no rank leaves the others waiting in theirs
    const long long n = split ? nsaved / 2 : nsaved;
    const bool too_short = split && nsaved > 0 && nsaved < 4;
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    rhat_counters((unsigned long long)(split ? 2 * N : N), (unsigned long long)n, cnt);
    const auto stage = [&](double* buf) -> hipError_t {                     // zeros | this rank's mean_r, Bsum_r, Wsum_r | its counters
        hipError_t e = hipMemsetAsync(buf, 0, L.size() * sizeof(double), h->stream);
        if (e == hipSuccess && n > 0 && !too_short)
            e = split ? rhat_split_async(h->stream, h->hist, nsaved, N, D, h->rhat_half, *ws, buf + L.mean_r(), buf + L.extra())
                      : rhat_sums_async(h->stream, sum, sumsq, X, held, N, D, nsaved, *ws, buf + L.mean_r(), buf + L.extra());
        if (e == hipSuccess) e = hipMemcpyAsync(buf + L.counters(), cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream);
        return e;
    };
    std::vector<double> host(L.size());
    if (!c) {
        double* buf = *ws + klara_rhat_partial_elems(D);
        HIPCHK(stage(buf));
        HIPCHK(hipMemcpyAsync(host.data(), buf, L.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        HIPCHK(comm_reserve(c, L.size()));
        CommSeq q{ c, h->stream };
        q.H(stage(c->buf));
        if (!comm_merge(q, L, cnt, host)) return KLARA_ERR_HIP;
    }
    const klara_status st = rhat_finish((size_t)D, host.data(), c != nullptr, rhat, mean, wsum, bsum, nchains, nper);
    return st != KLARA_OK ? st : too_short ? KLARA_ERR_STATE : KLARA_OK;
}

// (the split form reads the stored history of the coordinates: W = ndims only)
extern "C" klara_status klara_gather_rhat(klara_handle* h, klara_comm* c, int32_t split, double* rhat, double* mean, double* wsum, double* bsum,
                                          uint64_t* nchains, int64_t* nper)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    if (split ? (!h->hist || h->ring || !(h->d.monitor & KLARA_MON_HISTORY)) : !h->sum) return KLARA_ERR_STATE;   // (split: needs every saved step)
    HIPCHK(hipSetDevice(h->d.device));
    return gather_rhat_arrays(h, c, split, h->d.ndims, h->sum, h->sumsq, h->X, h->held, (long long)h->nsaved, &h->rhat_ws, rhat, mean, wsum, bsum, nchains, nper);
}

// ---- the pooled effective sample size (klara_ess.h): R-hat's merge with the units' lagged sums riding in the X slot — rank r stages the mean of its units'
// means, Bsum_r and, as plain sums, Wsum_r | csum_r[D][L + 1] — and, after it, the one statement of the estimator on the host
void ess_agreement_words(int L, uint64_t v[2]) { v[0] = (uint64_t)(uint32_t)L; v[1] = ~v[0]; }
bool ess_words_agree(const uint64_t v[2]) { return v[0] == ~v[1]; }                 // max(v) = ~max(~v) = min(v): every rank holds the same L

klara_status ess_finish(size_t D, int Lg, const double* host, bool merged, double* ess, double* tau, double* rho, double* mean, double* wsum, double* bsum,
                        int32_t* pairs, uint64_t* units, int64_t* nper, double* csum)
{
    const size_t R = (size_t)Lg + 1;
    const MergeLayout L{ D, D, D + D * R };
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    memcpy(cnt, host + L.counters(), sizeof(cnt));
    const unsigned long long m = cnt[MergeLayout::UNITS], sn = cnt[MergeLayout::UNIT_SAMPLES], sn2 = cnt[MergeLayout::UNIT_SAMPLES_SQ];
    if ((unsigned __int128)sn * sn != (unsigned __int128)m * sn2) return KLARA_ERR_STATE;       // (as rhat_finish: the same verdict on every rank)
    const unsigned long long n = m ? sn / m : 0;
    const bool none = n == 0, shortn = n < 4;
    const double* mu = host + (merged ? L.mean() : L.mean_r());
    const double dm = (double)m, dn = (double)n;
    std::vector<double> r(R);
    for (size_t j = 0; j < D; ++j) {
        const double ws = host[L.extra() + j], bs = host[L.M() + j];
        const double* cs = host + L.extra() + D + j * R;
        const double Wv = ws / (dm * (dn - 1.0));
        const double varp = ((dn - 1.0) / dn) * Wv + (m > 1 ? bs / (dm - 1.0) : 0.0);
        r[0] = 1.0;
        for (size_t k = 1; k < R; ++k) r[k] = shortn ? (double)NAN : 1.0 - (Wv - cs[k] / (dm * dn)) / varp;
        double sum = 0.0, prev = 0.0, t = (double)NAN;
        int np = 0;
        if (!shortn && Lg >= 1) {
            const int kk = (Lg - 1) / 2;
            for (int p = 0; p <= kk; ++p) {
                const double P = r[2 * p] + r[2 * p + 1];
                if (p >= 1 && P <= 0.0) break;                                      // Geyer's stop, from the second pair on
                const double Pm = (p >= 1 && P > prev) ? prev : P;                  // the monotone sequence
                sum = sum + Pm; prev = Pm; ++np;
            }
            t = -1.0 + 2.0 * sum;
        }
        if (ess) ess[j] = (dm * dn) / t;
        if (tau) tau[j] = t;
        if (rho) memcpy(rho + j * R, r.data(), R * sizeof(double));
        if (csum) memcpy(csum + j * R, cs, R * sizeof(double));
        if (pairs) pairs[j] = np;
        if (mean) mean[j] = none ? 0.0 : mu[j];
        if (wsum) wsum[j] = none ? 0.0 : ws;
        if (bsum) bsum[j] = none ? 0.0 : bs;
    }
    if (units) *units = none ? 0 : m;
    if (nper) *nper = (int64_t)n;
    return KLARA_OK;
}

// the verdict of a klara_gather_ess call over simulated ranks holding (units[r], n[r], L[r]): the maximum all-reduce of the agreement words and the sum of
// the counters replaced by host loops, then the very checks of the job path
extern "C" klara_status klara_selftest_ess_ranks(int32_t nranks, const int64_t* units, const int64_t* n, const int32_t* lags)
{
    if (!units || !n || !lags || nranks < 1) return KLARA_ERR_INVALID_ARG;
    for (int32_t r = 0; r < nranks; ++r)
        if (units[r] < 1 || n[r] < 0 || lags[r] < 0 || lags[r] > KLARA_ESS_MAXLAG) return KLARA_ERR_INVALID_ARG;
    uint64_t red[2] = { 0, 0 }, mine[2];
    unsigned long long sum[MergeLayout::NCOUNTERS] = { 0, 0, 0, 0 }, cnt[MergeLayout::NCOUNTERS];
    for (int32_t r = 0; r < nranks; ++r) {
        ess_agreement_words(lags[r], mine);
        for (int i = 0; i < 2; ++i) if (mine[i] > red[i]) red[i] = mine[i];
        rhat_counters((unsigned long long)units[r], (unsigned long long)n[r], cnt);
        for (int i = 0; i < MergeLayout::NCOUNTERS; ++i) sum[i] += cnt[i];
    }
    if (!ess_words_agree(red)) return KLARA_ERR_STATE;
    const MergeLayout L{ 1, 1, 1 + ((size_t)lags[0] + 1) };
    std::vector<double> host(L.size(), 0.0);
    memcpy(host.data() + L.counters(), sum, sizeof(sum));
    return ess_finish(1, lags[0], host.data(), true, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" klara_status klara_gather_ess(klara_handle* h, klara_comm* c, int32_t mode, int32_t maxlag, double* ess, double* tau, double* rho, double* mean,
                                         double* wsum, double* bsum, int32_t* pairs, uint64_t* nunits, int64_t* nper, int32_t* lags_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (mode != KLARA_ESS_STREAMED && mode != KLARA_ESS_HISTORY && mode != KLARA_ESS_SPLIT) return KLARA_ERR_INVALID_ARG;
    if (mode == KLARA_ESS_STREAMED ? maxlag != 0 : maxlag > KLARA_ESS_MAXLAG) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    const bool streamed = mode == KLARA_ESS_STREAMED, split = mode == KLARA_ESS_SPLIT;
    if (streamed ? !h->acov_S : (!h->hist || h->ring || !(h->d.monitor & KLARA_MON_HISTORY))) return KLARA_ERR_STATE;   // (history: needs every saved step)
    HIPCHK(hipSetDevice(h->d.device));
    const int D = h->d.ndims, per = split ? 2 : 1;
    const long long N = h->d.nchains, nd = N * D, E = per * nd;
    // units and samples per unit.  A split of 1 to 7 saved steps is refused, but only after the reductions: no rank leaves the others waiting in theirs
    const long long nsaved = streamed ? h->acov_n : h->nsaved, n = split ? nsaved / 2 : nsaved;
    const bool too_short = split && nsaved > 0 && nsaved < 8, run = n >= 1 && !too_short;
    const long long autolag = n - 1 < 0 ? 0 : n - 1 < KLARA_ESS_MAXLAG ? n - 1 : KLARA_ESS_MAXLAG;
    const int W = streamed ? h->acov_W : (int)(maxlag > 0 ? maxlag : autolag) + 1;
    const int Lg = n >= 1 ? (int)((long long)(W - 1) < n - 1 ? (long long)(W - 1) : n - 1) : 0;
    const MergeLayout L{ (size_t)D, (size_t)D, (size_t)D + (size_t)D * ((size_t)Lg + 1) };
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    rhat_counters((unsigned long long)(per * N), (unsigned long long)n, cnt);
    if (c) HIPCHK(comm_reserve(c, L.size()));
    // the streamed state: the job's own, or a temporary one fed from the stored history (3 W N D doubles, twice that for the split form; freed below)
    DeviceArrays tmp;
    EssState st[2] = { { h->acov_S, h->acov_head, h->acov_tail, h->acov_total, nullptr }, { nullptr, nullptr, nullptr, nullptr, nullptr } };
    double* ws = nullptr;
    hipError_t le = hipSuccess;                                             // local failures: remembered, every reduction is still entered
    const size_t wse = klara_ess_ws_elems(E, D, W);
    if (run && streamed) {
        if (!h->ess_ws) le = h->mem.alloc(&h->ess_ws, wse + L.extra() + (size_t)D + (size_t)D * (size_t)W);
        ws = h->ess_ws;
    } else if (run) {
        le = ess_alloc_states(tmp, per, W, nd, st);
        if (le == hipSuccess) le = tmp.alloc(&ws, wse + L.size());
        if (le == hipSuccess) le = ess_feed_history_async(h->stream, h->hist, nsaved, nd, W, per, st);
    }
    const auto stage = [&](double* buf) -> hipError_t {                     // zeros | this rank's mean_r, Bsum_r, Wsum_r | csum_r | its counters
        hipError_t e = hipMemsetAsync(buf, 0, L.size() * sizeof(double), h->stream);
        if (e == hipSuccess && run && le == hipSuccess) e = ess_reduce_async(h->stream, st, per, n, W, nd, D, ws, buf + L.mean_r(), buf + L.extra());
        if (e == hipSuccess) e = hipMemcpyAsync(buf + L.counters(), cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream);
        return e;
    };
    const auto leave = [&](klara_status s) { (void)hipStreamSynchronize(h->stream); (void)tmp.release(); return s; };
    std::vector<double> host(L.size(), 0.0);
    if (!c) {
        if (!run) memcpy(host.data() + L.counters(), cnt, sizeof(cnt));
        else {
            hipError_t e = le;
            if (e == hipSuccess) e = stage(ws + wse);
            if (e == hipSuccess) e = hipMemcpyAsync(host.data(), ws + wse, L.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) return leave(KLARA_ERR_HIP);
        }
    } else {
        // (1) the ranks' L, by an integer maximum over (L, ~L) as klara_gather_histogram's parameters: either all go on or all return KLARA_ERR_STATE
        // here, before the merge whose X slot has a length that depends on L
        uint64_t v[2];
        ess_agreement_words(Lg, v);
        CommSeq q1{ c, h->stream };
        q1.H(hipMemcpyAsync(c->buf, v, sizeof(v), hipMemcpyHostToDevice, h->stream));
        q1.reduce(0, 2, true, ncclMax);
        if (!q1.finish(v, sizeof(v))) return leave(KLARA_ERR_HIP);
        if (!ess_words_agree(v)) return leave(KLARA_ERR_STATE);
        // (2) R-hat's merge; the equal-n check is ess_finish's, on the summed counters
        CommSeq q{ c, h->stream };
        q.H(le);
        q.H(stage(c->buf));
        if (!comm_merge(q, L, cnt, host)) return leave(KLARA_ERR_HIP);
    }
    const bool synced = hipStreamSynchronize(h->stream) == hipSuccess, clean = tmp.release();
    if (!synced || !clean) return KLARA_ERR_HIP;
    const klara_status s = ess_finish((size_t)D, Lg, host.data(), c != nullptr, ess, tau, rho, mean, wsum, bsum, pairs, nunits, nper, nullptr);
    if (lags_out) *lags_out = Lg;
    return s != KLARA_OK ? s : too_short ? KLARA_ERR_STATE : KLARA_OK;
}
