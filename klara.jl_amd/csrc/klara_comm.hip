// klara_comm.hip — RCCL summary all-reduce behind the C ABI (librccl.so loaded lazily; see include/klara_hip.h)
#include <rccl/rccl.h>      // types only: librccl.so is dlopen'ed on first use (klara_comm_*)
#include <dlfcn.h>
#include <new>
#include "klara_handle.h"

struct klara_comm {
    void* dl = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0, device = 0;
    double* buf = nullptr; size_t cap = 0;                      // device staging: 2D doubles + 4 u64
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
extern "C" klara_status klara_gather_summaries(klara_handle* h, klara_comm* c, double* sum, double* sumsq, uint64_t* naccept,
                                               uint64_t* ntransitions, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h || !c) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    if ((sum || sumsq) && !h->sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t D = (size_t)h->d.ndims;
    if (c->cap < 2 * D + 4) {
        if (c->buf) (void)dfree(c->buf);
        c->buf = nullptr; c->cap = 0;
        HIPCHK(dalloc(&c->buf, 2 * D + 4));
        c->cap = 2 * D + 4;
    }
    // From here on every rank is inside a fixed sequence of collectives: a rank that returned at its first local failure would leave the others
    // waiting in theirs.  Local errors are remembered, every collective is still entered, the status is reported after the last one.
    bool bad = false;
    const auto H = [&](hipError_t e) { if (e != hipSuccess) bad = true; };
    H(hipMemsetAsync(c->buf, 0, (2 * D + 4) * sizeof(double), h->stream));
    H(pool_summaries_async(h, h->sum != nullptr, c->buf));
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(c->buf + 2 * D);
    const unsigned long long local[3] = { (unsigned long long)h->steps_done * (unsigned long long)h->d.nchains,
                                          (unsigned long long)h->nsaved * (unsigned long long)h->d.nchains,
                                          (unsigned long long)h->d.nchains };
    H(hipMemcpyAsync(cnt + 1, local, sizeof(local), hipMemcpyHostToDevice, h->stream));
    // two in-place all-reduces on the job's stream: 2D doubles, 4 counters — (2D + 4) x 8 B per rank, latency-bound
    if (c->AllReduce(c->buf, c->buf, 2 * D, ncclDouble, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
    if (c->AllReduce(cnt, cnt, 4, ncclUint64, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
    std::vector<double> host(2 * D + 4);
    H(hipMemcpyAsync(host.data(), c->buf, (2 * D + 4) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    H(hipStreamSynchronize(h->stream));
    if (bad) return KLARA_ERR_HIP;
    if (sum) memcpy(sum, host.data(), D * sizeof(double));
    if (sumsq) memcpy(sumsq, host.data() + D, D * sizeof(double));
    unsigned long long out[4];
    memcpy(out, host.data() + 2 * D, sizeof(out));
    if (naccept) *naccept = out[0];
    if (ntransitions) *ntransitions = out[1];
    if (nsamples) *nsamples = out[2];
    if (nchains) *nchains = out[3];
    return KLARA_OK;
}

// the between-rank merge of the pooled moments (klara_monitors.hip pool_moments_async has each rank's): n_r mean_r, to be summed over the ranks ...
__global__ void k_scale(double* __restrict__ dst, const double* __restrict__ src, double f, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[j] = f * src[j];
}
// rank-local part of the between-rank merge: buf[j] = mean_r -> M2_r + n_r (mean_r - mean)^2 with mean = wsum[j] / ntot
__global__ void k_moments_between(double* __restrict__ m2, const double* mean_r, const double* __restrict__ wsum,
                                  const unsigned long long* __restrict__ ntot, double n_r, int D, double* mean_out)   // (mean_out may be mean_r)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D) return;
    const double nt = (double)*ntot;
    const double mean = nt > 0.0 ? wsum[j] / nt : 0.0, d = mean_r[j] - mean;       // (no saved sample on any rank: zeros, as chan_merge leaves them without a communicator)
    mean_out[j] = mean;
    m2[j] = m2[j] + n_r * (d * d);
}
hipError_t moments_scale_async(hipStream_t stream, double* wsum, const double* mean_r, double n_r, int D)
{
    hipLaunchKernelGGL(k_scale, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, stream, wsum, mean_r, n_r, D);
    return hipGetLastError();
}
hipError_t moments_between_async(hipStream_t stream, double* m2, const double* mean_r, const double* wsum, const unsigned long long* ntot, double n_r,
                                 int D, double* mean_out)
{
    hipLaunchKernelGGL(k_moments_between, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, stream, m2, mean_r, wsum, ntot, n_r, D, mean_out);
    return hipGetLastError();
}

extern "C" klara_status klara_gather_moments(klara_handle* h, klara_comm* c, double* mean, double* m2, uint64_t* nsamples,
                                             uint64_t* naccept, uint64_t* ntransitions, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t D = (size_t)h->d.ndims;
    unsigned long long cnt[4] = { 0, (unsigned long long)h->steps_done * (unsigned long long)h->d.nchains,
                                  (unsigned long long)h->nsaved * (unsigned long long)h->d.nchains, (unsigned long long)h->d.nchains };
    std::vector<double> host(2 * D + 1);
    if (!c) {                                                               // this handle's chains only
        HIPCHK(pool_moments_async(h, h->pooled_out));
        HIPCHK(hipMemcpyAsync(host.data(), h->pooled_out, (2 * D + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(&cnt[0], host.data() + 2 * D, sizeof(cnt[0]));
    } else {
        // device staging: [0, D) mean_r -> mean, [D, 2D) M2_r -> M2, [2D] accept total, then [2D+1, 2D+4) counters, [2D+4, 3D+4) n_r mean_r
        if (c->cap < 3 * D + 4) {
            if (c->buf) (void)dfree(c->buf);
            c->buf = nullptr; c->cap = 0;
            HIPCHK(dalloc(&c->buf, 3 * D + 4));
            c->cap = 3 * D + 4;
        }
        // (as in klara_gather_summaries: once the sequence of collectives starts, every rank goes through all of it; errors are reported after the last)
        bool bad = false;
        const auto H = [&](hipError_t e) { if (e != hipSuccess) bad = true; };
        H(pool_moments_async(h, c->buf));
        unsigned long long* dcnt = reinterpret_cast<unsigned long long*>(c->buf + 2 * D);
        H(hipMemcpyAsync(dcnt + 1, cnt + 1, 3 * sizeof(cnt[0]), hipMemcpyHostToDevice, h->stream));
        double* wsum = c->buf + 2 * D + 4;
        const double n_r = (double)cnt[2];
        H(moments_scale_async(h->stream, wsum, c->buf, n_r, (int)D));
        // three in-place all-reduces on the job's stream: 4 counters, D weighted means, D sums of squares — latency-bound
        if (c->AllReduce(dcnt, dcnt, 4, ncclUint64, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        if (c->AllReduce(wsum, wsum, D, ncclDouble, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        H(moments_between_async(h->stream, c->buf + D, c->buf, wsum, dcnt + 2, n_r, (int)D, c->buf));
        if (c->AllReduce(c->buf + D, c->buf + D, D, ncclDouble, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        std::vector<double> hostc(2 * D + 4);
        H(hipMemcpyAsync(hostc.data(), c->buf, (2 * D + 4) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        H(hipStreamSynchronize(h->stream));
        if (bad) return KLARA_ERR_HIP;
        memcpy(host.data(), hostc.data(), 2 * D * sizeof(double));
        memcpy(cnt, hostc.data() + 2 * D, sizeof(cnt));
    }
    if (mean) memcpy(mean, host.data(), D * sizeof(double));
    if (m2) memcpy(m2, host.data() + D, D * sizeof(double));
    if (naccept) *naccept = cnt[0];
    if (ntransitions) *ntransitions = cnt[1];
    if (nsamples) *nsamples = cnt[2];
    if (nchains) *nchains = cnt[3];
    return KLARA_OK;
}

// The pooled covariance (klara_cov.h): this rank's (mean_r, M_r) from its accumulators, then — with a communicator — the D x D form of the merge above
extern "C" klara_status klara_gather_covariance(klara_handle* h, klara_comm* c, double* mean, double* m2, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->cov_S) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t D = (size_t)h->d.ndims, DD = D * D;
    unsigned long long cnt[4] = { 0, (unsigned long long)h->steps_done * (unsigned long long)h->d.nchains,
                                  (unsigned long long)h->cov_n * (unsigned long long)h->d.nchains, (unsigned long long)h->d.nchains };
    const double n_r = (double)cnt[2];
    std::vector<double> host(D + DD);
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
        // device staging: [0, D) mean_r, [D, D + DD) M_r -> M, 4 counters, [.. + D) n_r mean_r, [.. + D) mean
        const size_t need = 3 * D + DD + 4;
        if (c->cap < need) {
            if (c->buf) (void)dfree(c->buf);
            c->buf = nullptr; c->cap = 0;
            HIPCHK(dalloc(&c->buf, need));
            c->cap = need;
        }
        // (as in klara_gather_summaries: once the sequence of collectives starts, every rank goes through all of it; errors are reported after the last)
        bool bad = false;
        const auto H = [&](hipError_t e) { if (e != hipSuccess) bad = true; };
        H(local(c->buf));
        unsigned long long* dcnt = reinterpret_cast<unsigned long long*>(c->buf + D + DD);
        H(hipMemcpyAsync(dcnt, cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream));
        double* wsum = c->buf + D + DD + 4;
        double* mean_out = wsum + D;
        H(moments_scale_async(h->stream, wsum, c->buf, n_r, (int)D));
        if (c->AllReduce(dcnt, dcnt, 4, ncclUint64, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        if (c->AllReduce(wsum, wsum, D, ncclDouble, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        H(klara_cov_launch_between(h->stream, c->buf + D, c->buf, wsum, dcnt + 2, n_r, (int)D, mean_out));
        if (c->AllReduce(c->buf + D, c->buf + D, DD, ncclDouble, ncclSum, c->comm, h->stream) != ncclSuccess) bad = true;
        std::vector<double> hostc(need);
        H(hipMemcpyAsync(hostc.data(), c->buf, need * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        H(hipStreamSynchronize(h->stream));
        if (bad) return KLARA_ERR_HIP;
        memcpy(host.data(), hostc.data() + 2 * D + DD + 4, D * sizeof(double));
        memcpy(host.data() + D, hostc.data() + D, DD * sizeof(double));
        memcpy(cnt, hostc.data() + D + DD, sizeof(cnt));
    }
    if (mean) memcpy(mean, host.data(), D * sizeof(double));
    if (m2) memcpy(m2, host.data() + D, DD * sizeof(double));
    if (nsamples) *nsamples = cnt[2];
    if (nchains) *nchains = cnt[3];
    return KLARA_OK;
}
