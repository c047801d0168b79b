// klara_derived.hip — derived quantities (klara_desc.derived_nout > 0; klara_derived.h): the host launcher of the run-time compiled kernel, the calls that read
// the chains' sums and hand them to the coordinate reductions (klara_comm.hip), the compile check and the self tests.
#include "klara_handle.h"

// ------------------------------------------------------------------------------------------------------------------- update
hipError_t klara_derived_launch_update(KlaraJit* jit, const KDerivedGeom& g, const double* hist, long long col0, long long m, const double* data, long long ndata,
                                       double* dsum, double* dsumsq, double* stage, const KMargGeom* marg, const double* par, unsigned long long* counts,
                                       double* values_out, hipStream_t st)
{
    hipError_t e = hipSuccess;
    const size_t NK = (size_t)g.N * (size_t)g.K;
    for (long long done = 0; done < m && e == hipSuccess; done += KLARA_DERIVED_MAX_COLS) {
        const int mm = (int)(m - done < KLARA_DERIVED_MAX_COLS ? m - done : KLARA_DERIVED_MAX_COLS);
        e = klara_jit_launch_derived(jit, g, hist, col0 + done, mm, data, ndata, dsum, dsumsq, stage, st);
        if (e == hipSuccess && stage && counts) e = klara_marg_launch_update(*marg, stage, 0, mm, par, counts, st);      // the piece's outputs: a history of K dimensions
        if (e == hipSuccess && stage && values_out)
            e = hipMemcpyAsync(values_out + (size_t)done * NK, stage, (size_t)mm * NK * sizeof(double), hipMemcpyDeviceToDevice, st);
    }
    return e;
}

// ------------------------------------------------------------------------------------------------------------------- reading
extern "C" klara_status klara_get_derived_sums(klara_handle* h, double* sum, double* sumsq, int64_t* nsaved_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->der_sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t bytes = (size_t)h->d.nchains * (size_t)h->der.K * sizeof(double);
    if (sum) HIPCHK(hipMemcpyAsync(sum, h->der_sum, bytes, hipMemcpyDeviceToHost, h->stream));
    if (sumsq) HIPCHK(hipMemcpyAsync(sumsq, h->der_sumsq, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nsaved_out) *nsaved_out = h->der_n;
    return KLARA_OK;
}

// The reductions read X and held unconditionally (a sojourn not yet folded into the coordinate sums): the derived sums hold every saved step already, so held
// is N zeros and X any valid N x K array — dsum itself.  The accept total the moments' kernels also form is of N zeros and is not reported.
extern "C" klara_status klara_gather_derived_moments(klara_handle* h, klara_comm* c, double* mean, double* m2, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->der_sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    return gather_moments_arrays(h, c, h->der.K, h->der_sum, h->der_sumsq, h->der_sum, h->der_zero, reinterpret_cast<const unsigned long long*>(h->der_zero),
                                 h->der_n, h->der_partial, h->der_out, mean, m2, nsamples, nullptr, nullptr, nchains);
}

extern "C" klara_status klara_gather_derived_rhat(klara_handle* h, klara_comm* c, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* nchains,
                                                  int64_t* nper)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->der_sum) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    return gather_rhat_arrays(h, c, 0, h->der.K, h->der_sum, h->der_sumsq, h->der_sum, h->der_zero, h->der_n, &h->der_rhat_ws, rhat, mean, wsum, bsum, nchains, nper);
}

extern "C" klara_status klara_gather_derived_histogram(klara_handle* h, klara_comm* c, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->der_counts) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    return gather_histogram_arrays(h, c, h->der.K, h->der_marg, h->der_counts, h->der_n, h->der_marg_host.data(), counts, nsamples, nchains);
}

// ------------------------------------------------------------------------------------------------------------------- no device needed
extern "C" klara_status klara_check_derived(const char* src, int32_t ndims, int32_t nout)
{
    if (!src || ndims < 1 || ndims > 1024 || nout < 1 || nout > KLARA_DERIVED_MAX_OUT) return KLARA_ERR_INVALID_ARG;
    return klara_jit_create_derived(src, ndims, nout, false, false, nullptr);
}

extern "C" klara_status klara_selftest_derived_plan(int64_t nchains, int32_t ndims, int32_t nout, int32_t* chains_per_wg, int32_t* stride, int32_t* threads,
                                                    int64_t* workgroups, int64_t* lds_bytes)
{
    KDerivedGeom g;
    if (nout > KLARA_DERIVED_MAX_OUT || !klara_derived_plan(nchains, ndims, nout, &g)) return KLARA_ERR_INVALID_ARG;
    if (chains_per_wg) *chains_per_wg = g.CH;
    if (stride) *stride = g.stride;
    if (threads) *threads = g.threads;
    if (workgroups) *workgroups = g.nwg;
    if (lds_bytes) *lds_bytes = (int64_t)g.lds_bytes;
    return KLARA_OK;
}

// ------------------------------------------------------------------------------------------------------------------- self test
// The kernel on a caller's value history: klara_derived_launch_update launch by launch with col0 running through the history, as klara_run issues them (an
// empty launch skipped), from the zeroed accumulators klara_set_state leaves; then the sums as klara_get_derived_sums reads them.  Every argument check
// comes before any HIP call and before the compilation.
extern "C" klara_status klara_selftest_derived(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                               const int64_t* splits, const char* src, int32_t nout, const double* data, int64_t ndata, double* sum,
                                               double* sumsq, double* values)
{
    if (!hist || !splits || !src || !sum || !sumsq || nchains <= 0 || ndims < 1 || ndims > 1024 || ncols < 1 || nsplits <= 0 || nout < 1 ||
        nout > KLARA_DERIVED_MAX_OUT || ndata < 0 || (ndata > 0) != (data != nullptr))
        return KLARA_ERR_INVALID_ARG;
    long long total = 0;
    for (int j = 0; j < nsplits; ++j) {
        if (splits[j] < 0 || splits[j] > ncols) return KLARA_ERR_INVALID_ARG;
        total += splits[j];
    }
    if (total != ncols) return KLARA_ERR_INVALID_ARG;
    KDerivedGeom g;
    if (!klara_derived_plan(nchains, ndims, nout, &g)) return KLARA_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return KLARA_ERR_HIP;
    HIPCHK(hipSetDevice(device));
    const bool staged = values != nullptr;
    KlaraJit* jit = nullptr;
    KCHK(klara_jit_create_derived(src, ndims, nout, staged, true, &jit));
    const size_t nd = (size_t)nchains * (size_t)ndims, NK = (size_t)nchains * (size_t)nout;
    const hipStream_t st = 0;
    DeviceArrays mem;
    double *dh = nullptr, *dd = nullptr, *ds = nullptr, *dq = nullptr, *dstage = nullptr, *dval = nullptr;
    hipError_t e = mem.alloc(&dh, (size_t)ncols * nd);
    if (e == hipSuccess && ndata > 0) e = mem.alloc(&dd, (size_t)ndata);
    if (e == hipSuccess) e = mem.alloc(&ds, NK);
    if (e == hipSuccess) e = mem.alloc(&dq, NK);
    if (e == hipSuccess && staged) e = mem.alloc(&dstage, (size_t)KLARA_DERIVED_MAX_COLS * NK);
    if (e == hipSuccess && staged) e = mem.alloc(&dval, (size_t)ncols * NK);
    if (e == hipSuccess) e = hipMemcpy(dh, hist, (size_t)ncols * nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && ndata > 0) e = hipMemcpy(dd, data, (size_t)ndata * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(ds, 0, NK * sizeof(double));
    if (e == hipSuccess) e = hipMemset(dq, 0, NK * sizeof(double));
    long long col0 = 0;
    for (int j = 0; j < nsplits && e == hipSuccess; ++j) {
        if (splits[j] > 0)
            e = klara_derived_launch_update(jit, g, dh, col0, (long long)splits[j], dd, ndata, ds, dq, dstage, nullptr, nullptr, nullptr,
                                            staged ? dval + (size_t)col0 * NK : nullptr, st);
        col0 += splits[j];
    }
    std::vector<double> hs(NK), hq(NK);
    if (e == hipSuccess) e = hipMemcpyAsync(hs.data(), ds, NK * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hq.data(), dq, NK * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && staged) e = hipMemcpyAsync(values, dval, (size_t)ncols * NK * sizeof(double), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);               // (also after a failure: nothing of this call is in flight when its arrays go)
    if (e == hipSuccess) e = es;
    const bool clean = mem.release();
    klara_jit_destroy(jit);
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    memcpy(sum, hs.data(), NK * sizeof(double));
    memcpy(sumsq, hq.data(), NK * sizeof(double));
    return KLARA_OK;
}
