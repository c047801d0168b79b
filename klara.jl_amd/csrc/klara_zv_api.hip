// klara_zv_api.hip — zero-variance control variates (zv.jl) over the stored value and gradient histories: the entry points; kernels and launchers in klara_zv.hip
#include "klara_handle.h"
#include "klara_zv.h"

// the temporary device memory of one call is a DeviceArrays `ws` (klara_handle.h): released on every way out
#define ZVCHK(expr)                                                                                              \
    do {                                                                                                         \
        hipError_t e__ = (expr);                                                                                 \
        if (e__ != hipSuccess) { (void)hipStreamSynchronize(h->stream); (void)ws.release(); return e__ == hipErrorOutOfMemory ? KLARA_ERR_NOMEM : KLARA_ERR_HIP; } \
    } while (0)

static klara_status zv_ready(const klara_handle* h, int32_t order, KZvGeom* g)
{
    if (!h || (order != KLARA_ZV_LINEAR && order != KLARA_ZV_QUADRATIC)) return KLARA_ERR_INVALID_ARG;
    if (!h->hist || !h->hist_g || h->ring || !(h->d.monitor & KLARA_MON_HISTORY) || !(h->d.monitor & KLARA_MON_HIST_GRAD) || !h->have_state ||
        h->nsaved < 2)
        return KLARA_ERR_STATE;                                                     // (needs every saved step of both histories)
    if (!klara_zv_plan(order, h->d.ndims, g)) return KLARA_ERR_UNSUPPORTED;         // more than KLARA_ZV_MAX_TERMS control variates
    return KLARA_OK;
}

extern "C" klara_status klara_get_chain_zv(klara_handle* h, int32_t order, int32_t pooled, double* coef, double* zv_mean, double* zv_var,
                                           int32_t* info, int64_t* nsamples_out)
{
    KZvGeom g;
    const klara_status rs = zv_ready(h, order, &g);
    if (rs != KLARA_OK) return rs;
    HIPCHK(hipSetDevice(h->d.device));
    const long long N = h->d.nchains, D = h->d.ndims, n = h->nsaved, K = g.K;
    if (nsamples_out) *nsamples_out = n;
    if ((pooled ? N * n : n) < K + 2) {                                             // too few samples for K coefficients and a variance
        const size_t ncoef = (size_t)(pooled ? 1 : N) * K * D;
        if (coef) for (size_t i = 0; i < ncoef; ++i) coef[i] = NAN;
        for (size_t i = 0; i < (size_t)(N * D); ++i) { if (zv_mean) zv_mean[i] = NAN; if (zv_var) zv_var[i] = NAN; }
        if (info) for (long long c = 0; c < N; ++c) info[c] = 2;
        return KLARA_OK;
    }
    const long long chunk = klara_zv_chunk(g, N);
    const bool want_apply = zv_mean || zv_var;
    DeviceArrays ws;
    double *S = nullptr, *meanbuf = nullptr, *dcoef = nullptr, *zmean = nullptr, *zvar = nullptr, *pS = nullptr, *pmean = nullptr;
    int* dinfo = nullptr;
    ZVCHK(ws.alloc(&S, (size_t)chunk * g.s_elems));
    ZVCHK(ws.alloc(&meanbuf, (size_t)chunk * g.LDW));
    ZVCHK(ws.alloc(&dcoef, (size_t)(pooled ? 1 : chunk) * K * D));
    ZVCHK(ws.alloc(&dinfo, (size_t)(pooled ? 1 : chunk)));
    if (want_apply) { ZVCHK(ws.alloc(&zmean, (size_t)chunk * D)); ZVCHK(ws.alloc(&zvar, (size_t)chunk * D)); }
    if (pooled) {
        ZVCHK(ws.alloc(&pS, g.s_elems));
        ZVCHK(ws.alloc(&pmean, (size_t)2 * g.LDW));
        ZVCHK(hipMemsetAsync(pmean, 0, (size_t)2 * g.LDW * sizeof(double), h->stream));
        int flip = 0;
        for (long long c0 = 0; c0 < N; c0 += chunk) {                               // chains merged in ascending order, chunk after chunk
            const long long nc = N - c0 < chunk ? N - c0 : chunk;
            ZVCHK(klara_zv_launch_gram(g, h->hist, h->hist_g, N, n, c0, nc, S, meanbuf, 0, h->stream));
            ZVCHK(klara_zv_launch_merge(g, S, meanbuf, nc, (double)n, (double)c0 * (double)n, pmean + (size_t)flip * g.LDW,
                                        pmean + (size_t)(1 - flip) * g.LDW, pS, h->stream));
            flip = 1 - flip;
        }
        ZVCHK(klara_zv_launch_solve(g, pS, 1, dcoef, dinfo, h->stream));
        ZVCHK(hipStreamSynchronize(h->stream));
        int pinfo = 0;
        ZVCHK(hipMemcpy(&pinfo, dinfo, sizeof(int), hipMemcpyDeviceToHost));
        if (coef) ZVCHK(hipMemcpy(coef, dcoef, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost));
        if (info) for (long long c = 0; c < N; ++c) info[c] = pinfo;
        if (want_apply)
            for (long long c0 = 0; c0 < N; c0 += chunk) {
                const long long nc = N - c0 < chunk ? N - c0 : chunk;
                ZVCHK(klara_zv_launch_gram(g, h->hist, h->hist_g, N, n, c0, nc, S, meanbuf, 1, h->stream));      // the chains' own means again
                ZVCHK(klara_zv_launch_apply(g, h->hist, h->hist_g, N, n, c0, nc, meanbuf, dcoef, 0, zmean, zvar, nullptr, h->stream));
                ZVCHK(hipStreamSynchronize(h->stream));
                if (zv_mean) ZVCHK(hipMemcpy(zv_mean + (size_t)c0 * D, zmean, (size_t)nc * D * sizeof(double), hipMemcpyDeviceToHost));
                if (zv_var) ZVCHK(hipMemcpy(zv_var + (size_t)c0 * D, zvar, (size_t)nc * D * sizeof(double), hipMemcpyDeviceToHost));
            }
    } else {
        for (long long c0 = 0; c0 < N; c0 += chunk) {
            const long long nc = N - c0 < chunk ? N - c0 : chunk;
            ZVCHK(klara_zv_launch_gram(g, h->hist, h->hist_g, N, n, c0, nc, S, meanbuf, 0, h->stream));
            ZVCHK(klara_zv_launch_solve(g, S, nc, dcoef, dinfo, h->stream));
            if (want_apply)
                ZVCHK(klara_zv_launch_apply(g, h->hist, h->hist_g, N, n, c0, nc, meanbuf, dcoef, (size_t)K * D, zmean, zvar, nullptr, h->stream));
            ZVCHK(hipStreamSynchronize(h->stream));
            if (coef) ZVCHK(hipMemcpy(coef + (size_t)c0 * K * D, dcoef, (size_t)nc * K * D * sizeof(double), hipMemcpyDeviceToHost));
            if (info) ZVCHK(hipMemcpy(info + c0, dinfo, (size_t)nc * sizeof(int), hipMemcpyDeviceToHost));
            if (zv_mean) ZVCHK(hipMemcpy(zv_mean + (size_t)c0 * D, zmean, (size_t)nc * D * sizeof(double), hipMemcpyDeviceToHost));
            if (zv_var) ZVCHK(hipMemcpy(zv_var + (size_t)c0 * D, zvar, (size_t)nc * D * sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    return ws.release() ? KLARA_OK : KLARA_ERR_STATE;        // (KLARA_DEBUG_CANARY=1: a kernel wrote outside the workspace)
}

// one chain: its own coefficients (coef_in NULL; returned through coef_out / info_out when asked for) or given ones, and the corrected series when `value` is given
static klara_status zv_one_chain(klara_handle* h, int64_t local_chain, int32_t order, const double* coef_in, double* coef_out, int32_t* info_out,
                                 double* value, int64_t capacity_cols, int64_t* ncols_out)
{
    KZvGeom g;
    if (!h || local_chain < 0 || local_chain >= h->d.nchains || capacity_cols < 0) return KLARA_ERR_INVALID_ARG;
    const klara_status rs = zv_ready(h, order, &g);
    if (rs != KLARA_OK) return rs;
    HIPCHK(hipSetDevice(h->d.device));
    const long long N = h->d.nchains, D = h->d.ndims, n = h->nsaved, K = g.K;
    if (ncols_out) *ncols_out = n;
    const long long ncopy = value ? (n < capacity_cols ? n : capacity_cols) : 0;
    if (ncopy == 0 && !coef_out && !info_out) return KLARA_OK;
    if (!coef_in && n < K + 2) {                                                    // info = 2: no coefficients of its own
        for (size_t i = 0; i < (size_t)(ncopy * D); ++i) value[i] = NAN;
        if (coef_out) for (size_t i = 0; i < (size_t)(K * D); ++i) coef_out[i] = NAN;
        if (info_out) *info_out = 2;
        return KLARA_OK;
    }
    DeviceArrays ws;
    double *S = nullptr, *meanbuf = nullptr, *dcoef = nullptr, *series = nullptr;
    int* dinfo = nullptr;
    ZVCHK(ws.alloc(&S, g.s_elems));
    ZVCHK(ws.alloc(&meanbuf, (size_t)g.LDW));
    ZVCHK(ws.alloc(&dcoef, (size_t)K * D));
    ZVCHK(ws.alloc(&dinfo, (size_t)1));
    ZVCHK(klara_zv_launch_gram(g, h->hist, h->hist_g, N, n, local_chain, 1, S, meanbuf, coef_in ? 1 : 0, h->stream));
    if (coef_in) ZVCHK(hipMemcpyAsync(dcoef, coef_in, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else ZVCHK(klara_zv_launch_solve(g, S, 1, dcoef, dinfo, h->stream));
    if (ncopy > 0) {
        ZVCHK(ws.alloc(&series, (size_t)n * D));
        ZVCHK(klara_zv_launch_apply(g, h->hist, h->hist_g, N, n, local_chain, 1, meanbuf, dcoef, (size_t)K * D, nullptr, nullptr, series, h->stream));
    }
    ZVCHK(hipStreamSynchronize(h->stream));
    if (ncopy > 0) ZVCHK(hipMemcpy(value, series, (size_t)ncopy * D * sizeof(double), hipMemcpyDeviceToHost));   // [step][D] = NState layout (D x n, column-major)
    if (coef_out) ZVCHK(hipMemcpy(coef_out, dcoef, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost));
    if (info_out) { int v = 0; if (!coef_in) ZVCHK(hipMemcpy(&v, dinfo, sizeof(int), hipMemcpyDeviceToHost)); *info_out = v; }
    return ws.release() ? KLARA_OK : KLARA_ERR_STATE;
}

extern "C" klara_status klara_get_chain_zv_series(klara_handle* h, int64_t local_chain, int32_t order, const double* coef, double* value,
                                                  int64_t capacity_cols, int64_t* ncols_out)
{
    return zv_one_chain(h, local_chain, order, coef, nullptr, nullptr, value, capacity_cols, ncols_out);
}

extern "C" klara_status klara_get_chain_zv_one(klara_handle* h, int64_t local_chain, int32_t order, double* coef, int32_t* info, double* value,
                                               int64_t capacity_cols, int64_t* ncols_out)
{
    return zv_one_chain(h, local_chain, order, nullptr, coef, info, value, capacity_cols, ncols_out);
}
