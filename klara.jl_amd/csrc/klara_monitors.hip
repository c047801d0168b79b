// klara_monitors.hip — what a job accumulates and how it is read back: batch means, streaming autocovariances, pooled summaries and moments,
// histories, tuner state, layout and kernel queries.
#include "klara_handle.h"
#include "klara_rhat.h"

// Closes one batch of every (chain, dimension) series in [i0, i1): batch mean from the running sums at the two batch
// boundaries, then Welford's update of the mean and the sum of squared deviations of the batch means (count = batches closed
// before this one).  mcvar.jl:35-41 takes var(batch means); the history-free form never revisits a sample.
__global__ __launch_bounds__(256) void k_bm_close(const double* __restrict__ sum, const double* __restrict__ X, const long long* __restrict__ held,
                                                  int D, double* __restrict__ prev, double* __restrict__ mean,
                                                  double* __restrict__ m2, long long i0, long long i1, long long count, double batchlen)
{
    const long long i = i0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= i1) return;
    const long long hd = held[i / D];
    const double s = hd > 0 ? sum[i] + (double)hd * X[i] : sum[i];       // the running sum over the saved steps (sojourn form)
    const double b = (s - prev[i]) / batchlen;
    prev[i] = s;
    const double delta = b - mean[i];
    const double mn = mean[i] + delta / (double)(count + 1);
    mean[i] = mn;
    m2[i] = m2[i] + delta * (b - mn);
}

// every partition closes its own chains on its own stream (layout kind 3 runs chain partitions on internal streams)
hipError_t launch_bm_close(klara_handle* h, int nparts)
{
    const long long N = h->d.nchains, D = h->d.ndims;
    const int np = h->plan.kind == 3 ? nparts : 1;
    for (int j = 0; j < np; ++j) {
        long long c0 = 0, c1 = N;
        if (np > 1) part_range(h, np, j, &c0, &c1);          // (the chains the partition's transition kernels cover)
        if (c0 >= c1) break;
        const long long n = (c1 - c0) * D;
        hipLaunchKernelGGL(k_bm_close, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, j == 0 ? h->stream : h->side[j - 1], h->sum, h->X, h->held, (int)D,
                           h->bm_prev, h->bm_mean, h->bm_m2, c0 * D, c1 * D, h->bm_count, (double)h->d.bm_batchlen);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- streaming autocovariances (klara_desc.acov_maxlag): after every launch the samples it saved — columns [col0, col0 + m) of
// the value ring — update, for every (chain, dimension) series, the lagged cross-products S_k = sum_t z_t z_(t-k), k < W, the total of z
// and the last W values of z (most recent first), where z_t = x_t - pivot and the pivot is the series' first saved sample; the first W
// samples are kept as they are (head[0] is the pivot).  The autocovariance does not depend on a shift, and sums of z lose
// ((pivot - mean) / sd)^2 digits where sums of x lose (mean / sd)^2: a chain at 1e6 +- 1 keeps its ESS.  One thread per series, S and
// the window in registers.
__device__ inline double acov_pivot(const double* __restrict__ hist, long long col0, long long n_before, long long nd,
                                    const double* __restrict__ head, long long i)
{
    return n_before == 0 ? hist[col0 * nd + i] : head[i];
}
template <int WMAX>
__global__ __launch_bounds__(256) void k_acov_update(const double* __restrict__ hist, long long col0, int m, long long n_before, int W,
                                                     long long nd, double* __restrict__ S, double* __restrict__ head,
                                                     double* __restrict__ tail, double* __restrict__ total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nd) return;
    const double pivot = acov_pivot(hist, col0, n_before, nd, head, i);
    double s[WMAX], win[WMAX];
#pragma unroll
    for (int k = 0; k < WMAX; ++k) { s[k] = k < W ? S[(long long)k * nd + i] : 0.0; win[k] = k < W ? tail[(long long)k * nd + i] : 0.0; }
    double tot = total[i];
    for (int j = 0; j < m; ++j) {
        const double raw = hist[(col0 + j) * nd + i], x = raw - pivot;
        s[0] = s[0] + x * x;
#pragma unroll
        for (int k = 1; k < WMAX; ++k) s[k] = s[k] + x * win[k - 1];        // (win holds zeros where no sample exists yet)
        if (n_before + j < W) head[(n_before + j) * nd + i] = raw;
#pragma unroll
        for (int k = WMAX - 1; k > 0; --k) win[k] = win[k - 1];
        win[0] = x;
        tot = tot + x;
    }
#pragma unroll
    for (int k = 0; k < WMAX; ++k) if (k < W) { S[(long long)k * nd + i] = s[k]; tail[(long long)k * nd + i] = win[k]; }
    total[i] = tot;
}

// Lags 32 b .. 32 b + 31 (b >= 1; windows beyond 32 lags, klara_desc.acov_maxlag up to 127): the cross-products of z with its own history delayed by
// 32 b samples, y_j = z_(j - 32 b) — the same 32-lag update on the pair (z, y): S_(32b + r) += z_j y_(j - r).  y comes from the launch's own
// columns where j >= 32 b and from the tail kept by the earlier launches (tail[k] = the (k + 1)-th most recent z before this launch)
// otherwise; the passes of the higher blocks run BEFORE the lag-0 pass rewrites the tail (and, in a job's first launch, before it writes head[0]).
__global__ __launch_bounds__(256) void k_acov_update_block(const double* __restrict__ hist, long long col0, int m, long long n_before, int b, int W,
                                                           long long nd, double* __restrict__ S, const double* __restrict__ head,
                                                           const double* __restrict__ tail)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nd) return;
    const double pivot = acov_pivot(hist, col0, n_before, nd, head, i);
    const int k0 = 32 * b;
    double s[32], win[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        s[r] = k0 + r < W ? S[(long long)(k0 + r) * nd + i] : 0.0;
        win[r] = k0 + r < W ? tail[(long long)(k0 + r) * nd + i] : 0.0;            // y_(-1-r) = z_(-1-r-k0)   (zeros where no sample exists yet)
    }
    for (int j = 0; j < m; ++j) {
        const double x = hist[(col0 + j) * nd + i] - pivot;
        const double y = j >= k0 ? hist[(col0 + j - k0) * nd + i] - pivot : tail[(long long)(k0 - j - 1) * nd + i];
        s[0] = s[0] + x * y;
#pragma unroll
        for (int r = 1; r < 32; ++r) s[r] = s[r] + x * win[r - 1];
#pragma unroll
        for (int r = 31; r > 0; --r) win[r] = win[r - 1];
        win[0] = y;
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) if (k0 + r < W) S[(long long)(k0 + r) * nd + i] = s[r];
}
// ... and the tail of a window beyond 32 lags, after the lag-0 pass (which has moved entries 0..31 and written head[0]): entries 32 .. W-1 take the
// values of z that are now 33 .. W back — from this launch's columns or from the old tail, moved from the far end so that nothing is overwritten before it is read
__global__ __launch_bounds__(256) void k_acov_tail_far(const double* __restrict__ hist, long long col0, int m, int W, long long nd,
                                                       const double* __restrict__ head, double* __restrict__ tail, const double* __restrict__ old_near)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nd) return;
    const double pivot = head[i];
    for (int k = W - 1; k >= 32; --k) {                     // new tail[k] = z_(m-1-k): a column of this launch, or the old tail[k - m]
        double v;
        if (k < m) v = hist[(col0 + m - 1 - k) * nd + i] - pivot;
        else if (k - m >= 32) v = tail[(long long)(k - m) * nd + i];            // (an entry further down: not yet overwritten — k descends)
        else v = old_near[(long long)(k - m) * nd + i];                          // (one of the first 32 entries as they were BEFORE the lag-0 pass)
        tail[(long long)k * nd + i] = v;
    }
}

// (the buffers, not the handle: klara_run and klara_selftest_chain_stats launch the same kernels through this one function)
hipError_t launch_acov_update(hipStream_t stream, const double* hist, double* S, double* head, double* tail, double* near, double* total,
                              long long n_before, int W, long long nd, long long col0, long long m)
{
    const dim3 grid((unsigned)((nd + 255) / 256)), blk(256);
    if (W > 32) {       // windows beyond 32 lags: the higher lag blocks first (they read the tail as the earlier launches left it)
        for (int b = (W - 1) / 32; b >= 1; --b)
            hipLaunchKernelGGL(k_acov_update_block, grid, blk, 0, stream, hist, col0, (int)m, n_before, b, W, nd, S, head, tail);
        // (the lag-0 pass below rewrites tail[0..31]; the far tail needs their old values when fewer than 32 samples arrive: keep a copy)
        hipError_t e = hipMemcpyAsync(near, tail, (size_t)32 * nd * sizeof(double), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    if (W <= 8) hipLaunchKernelGGL((k_acov_update<8>), grid, blk, 0, stream, hist, col0, (int)m, n_before, W, nd, S, head, tail, total);
    else if (W <= 16) hipLaunchKernelGGL((k_acov_update<16>), grid, blk, 0, stream, hist, col0, (int)m, n_before, W, nd, S, head, tail, total);
    else hipLaunchKernelGGL((k_acov_update<32>), grid, blk, 0, stream, hist, col0, (int)m, n_before, W, nd, S, head, tail, total);
    if (W > 32) hipLaunchKernelGGL(k_acov_tail_far, grid, blk, 0, stream, hist, col0, (int)m, W, nd, head, tail, near);
    return hipGetLastError();
}

// autocov(v, 0:maxlag) of StatsBase (demean = true) from the streamed sums of z = x - pivot (pivot = head[0]): with m = total / n,
//   n acv_k = sum_(t>k) (z_t - m)(z_(t-k) - m) = S_k - m [(total - first k) + (total - last k)] + (n - k) m^2,
// then Geyer's truncation (mcvar.jl:75-105 imse, :137-158 ipse).
__global__ __launch_bounds__(256) void k_acov_finalize(const double* __restrict__ S, const double* __restrict__ head, const double* __restrict__ tail,
                                                       const double* __restrict__ total, long long n, int W, long long nd,
                                                       double* __restrict__ imse, double* __restrict__ ipse)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nd) return;
    const double tot = total[i], mean = tot / (double)n, pivot = head[i];
    const long long maxlag = (W - 1) < (n - 1) ? (W - 1) : (n - 1);
    const long long kk = (maxlag - 1) / 2;                       // floor((maxlag-1)/2), mcvar.jl:76
    double hs = 0.0, ts = 0.0, acv0 = 0.0, gsum_m = 0.0, gsum_p = 0.0, gprev = 0.0;
    bool stop = false;
    for (long long j = 0; j <= kk && !stop; ++j) {
        double pair = 0.0;
        for (int h2 = 0; h2 < 2; ++h2) {
            const long long k = 2 * j + h2;
            // hs / ts = sum of the first / last k values of z
            const double a = (S[k * nd + i] - mean * ((tot - ts) + (tot - hs)) + (double)(n - k) * mean * mean) / (double)n;
            if (k == 0) acv0 = a;
            pair += a;
            hs += head[k * nd + i] - pivot; ts += tail[k * nd + i];
        }
        if (pair <= 0.0) { stop = true; break; }                 // m = j (mcvar.jl:87-90)
        gsum_p += pair;
        double gm = pair;
        if (j > 0 && gm > gprev) gm = gprev;                     // monotone sequence (mcvar.jl:94-100)
        gsum_m += gm; gprev = gm;
    }
    if (imse) imse[i] = (-acv0 + 2.0 * gsum_m) / (double)n;
    if (ipse) ipse[i] = (-acv0 + 2.0 * gsum_p) / (double)n;
}

// Geyer's estimators from the streamed sums of n samples into imse / ipse (device, nd each; either may be null), on `stream`
hipError_t launch_acov_finalize(hipStream_t stream, const double* S, const double* head, const double* tail, const double* total,
                                long long n, int W, long long nd, double* imse, double* ipse)
{
    hipLaunchKernelGGL(k_acov_finalize, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, stream, S, head, tail, total, n, W, nd, imse, ipse);
    return hipGetLastError();
}

extern "C" klara_status klara_get_chain_acov_mcvar(klara_handle* h, double* mcvar_imse, double* mcvar_ipse, int64_t* nsamples_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->acov_S || !h->have_state || h->acov_n < 2) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const long long nd = (long long)h->d.nchains * h->d.ndims;
    double* buf = nullptr;
    HIPCHK(dalloc(&buf, (size_t)2 * nd));
    hipError_t e = launch_acov_finalize(h->stream, h->acov_S, h->acov_head, h->acov_tail, h->acov_total, h->acov_n, h->acov_W, nd,
                                        mcvar_imse ? buf : nullptr, mcvar_ipse ? buf + nd : nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && mcvar_imse) e = hipMemcpy(mcvar_imse, buf, nd * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mcvar_ipse) e = hipMemcpy(mcvar_ipse, buf + nd, nd * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(buf);
    if (nsamples_out) *nsamples_out = h->acov_n;
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

extern "C" klara_status klara_saved_steps(klara_handle* h, int64_t* nsaved_out)
{
    if (!h || !nsaved_out) return KLARA_ERR_INVALID_ARG;
    *nsaved_out = h->nsaved;
    return KLARA_OK;
}

extern "C" klara_status klara_get_state(klara_handle* h, double* x, double* logtarget, double* gradlogtarget)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (x) HIPCHK(hipMemcpy(x, h->X, N * D * sizeof(double), hipMemcpyDeviceToHost));
    if (logtarget) HIPCHK(hipMemcpy(logtarget, h->LT, N * sizeof(double), hipMemcpyDeviceToHost));
    if (gradlogtarget) HIPCHK(hipMemcpy(gradlogtarget, h->GR, N * D * sizeof(double), hipMemcpyDeviceToHost));
    return KLARA_OK;
}

extern "C" klara_status klara_get_accept_mask(klara_handle* h, uint8_t* mask, int64_t capacity_steps,
                                              int64_t* nsteps_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->accept) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long n = h->steps_done < capacity_steps ? h->steps_done : capacity_steps;
    if (mask && n > 0) HIPCHK(hipMemcpy(mask, h->accept, (size_t)n * (size_t)h->d.nchains, hipMemcpyDeviceToHost));
    if (nsteps_out) *nsteps_out = h->steps_done;
    return KLARA_OK;
}

extern "C" klara_status klara_get_accept_rows(klara_handle* h, int64_t first_step, int64_t nsteps, uint8_t* mask)
{
    if (!h || first_step < 0 || nsteps < 0 || (nsteps > 0 && !mask)) return KLARA_ERR_INVALID_ARG;
    if (!h->accept || !h->have_state) return KLARA_ERR_STATE;
    if (first_step + nsteps > h->steps_done) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nsteps > 0)
        HIPCHK(hipMemcpy(mask, h->accept + (size_t)first_step * (size_t)h->d.nchains, (size_t)nsteps * (size_t)h->d.nchains, hipMemcpyDeviceToHost));
    return KLARA_OK;
}

extern "C" klara_status klara_get_accept_counts(klara_handle* h, uint64_t* naccept, uint64_t* nsteps_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (naccept) HIPCHK(hipMemcpy(naccept, h->naccept, (size_t)h->d.nchains * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (nsteps_out) *nsteps_out = (uint64_t)h->steps_done;
    return KLARA_OK;
}

// sums over the saved steps from their sojourn form: out = part + held * x  (sq: x -> x * x); one product, one sum
__global__ __launch_bounds__(256) void k_sum_view(const double* __restrict__ part, const double* __restrict__ X, const long long* __restrict__ held,
                                                  long long n, int D, int sq, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long hd = held[i / D];
    const double x = X[i], v = sq ? x * x : x;
    out[i] = hd > 0 ? part[i] + (double)hd * v : part[i];
}

extern "C" klara_status klara_get_chain_sums(klara_handle* h, double* sum, double* sumsq, int64_t* nsaved_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->sum || !h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t n = (size_t)h->d.nchains * (size_t)h->d.ndims;
    if (sum || sumsq) {
        double* view = nullptr;
        HIPCHK(dalloc(&view, n));
        hipError_t e = hipSuccess;
        for (int sq = 0; sq < 2 && e == hipSuccess; ++sq) {
            double* dst = sq ? sumsq : sum;
            if (!dst) continue;
            hipLaunchKernelGGL(k_sum_view, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, sq ? h->sumsq : h->sum, h->X, h->held,
                               (long long)n, h->d.ndims, sq, view);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(dst, view, n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        (void)dfree(view);
        if (e != hipSuccess) return KLARA_ERR_HIP;
    } else {
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (nsaved_out) *nsaved_out = h->nsaved;
    return KLARA_OK;
}

// Pooled (over chains) per-dimension sums and the accepted-transition total, two stages of fixed shape => deterministic for a
// given chain count: block b of KLARA_POOL_BLOCKS adds the chains c = b, b + NB, ... column by column (a chain's D values are
// contiguous: coalesced) into partial[b][0..2D) and their accept counters into partial_acc[b]; one small block then adds the
// partials in ascending b.  (100 blocks striding over 105 MB took 167 us at 65,536 x 100; this takes ~25.)
#define KLARA_POOL_BLOCKS 1024
__global__ __launch_bounds__(256) void k_pool_stage1(const double* __restrict__ sum, const double* __restrict__ sumsq,
                                                     const double* __restrict__ X, const long long* __restrict__ held,
                                                     const unsigned long long* __restrict__ nacc, long long N, int D, int nb,
                                                     double* __restrict__ partial, unsigned long long* __restrict__ partial_acc)
{
    const int b = blockIdx.x;
    if (sum != nullptr) {
        for (int j = threadIdx.x; j < 2 * D; j += 256) {
            const bool sq = j >= D;
            const double* src = sq ? sumsq + (j - D) : sum + j;
            const double* xs = X + (sq ? j - D : j);
            double a = 0.0;
            for (long long c = b; c < N; c += nb) {                         // (a chain's sum over its saved steps: part + held * x)
                const long long hd = held[c];
                const double x = xs[c * D], v = sq ? x * x : x;
                a += hd > 0 ? src[c * D] + (double)hd * v : src[c * D];
            }
            partial[(long long)b * 2 * D + j] = a;
        }
    }
    __shared__ unsigned long long s[256];
    unsigned long long a = 0;
    for (long long c = (long long)b + (long long)threadIdx.x * nb; c < N; c += 256ll * nb) a += nacc[c];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) { if ((int)threadIdx.x < m) s[threadIdx.x] += s[threadIdx.x + m]; __syncthreads(); }
    if (threadIdx.x == 0) partial_acc[b] = s[0];
}
__global__ __launch_bounds__(256) void k_pool_stage2(const double* __restrict__ partial, const unsigned long long* __restrict__ partial_acc,
                                                     int D, int nb, bool with_sums, double* __restrict__ out)
{
    // block j < 2 D: column j of the partials; block 2 D: the accept counters.  Thread t adds the partials b = t, t + 256, ...
    // (ascending), then a fixed-shape tree over the 256 threads.
    __shared__ double sd[256];
    __shared__ unsigned long long su[256];
    const int j = blockIdx.x, t = threadIdx.x;
    if (j < 2 * D) {
        if (!with_sums) return;
        double a = 0.0;
        for (int b = t; b < nb; b += 256) a += partial[(long long)b * 2 * D + j];
        sd[t] = a;
        __syncthreads();
        for (int m = 128; m > 0; m >>= 1) { if (t < m) sd[t] += sd[t + m]; __syncthreads(); }
        if (t == 0) out[j] = sd[0];
    } else {
        unsigned long long a = 0;
        for (int b = t; b < nb; b += 256) a += partial_acc[b];
        su[t] = a;
        __syncthreads();
        for (int m = 128; m > 0; m >>= 1) { if (t < m) su[t] += su[t + m]; __syncthreads(); }
        if (t == 0) *reinterpret_cast<unsigned long long*>(out + 2 * D) = su[0];
    }
}
// out: 2 D doubles (sum, sumsq; untouched when sum is null) followed by the u64 accept total.  partial: KLARA_POOL_BLOCKS x (2 D doubles + 1 u64).
// (the buffers, not the handle: the job path and klara_selftest_pooled launch the same kernels through this one function)
hipError_t pool_summaries_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held,
                                const unsigned long long* naccept, long long N, int D, double* partial, double* out)
{
    const int nb = (int)(N < KLARA_POOL_BLOCKS ? N : KLARA_POOL_BLOCKS);
    unsigned long long* partial_acc = reinterpret_cast<unsigned long long*>(partial + (size_t)KLARA_POOL_BLOCKS * 2 * D);
    hipLaunchKernelGGL(k_pool_stage1, dim3(nb), dim3(256), 0, stream, sum, sumsq, X, held, naccept, N, D, nb, partial, partial_acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pool_stage2, dim3(2 * D + 1), dim3(256), 0, stream, partial, partial_acc, D, nb, sum != nullptr, out);
    return hipGetLastError();
}
hipError_t pool_summaries_async(klara_handle* h, bool with_sums, double* out)
{
    return pool_summaries_async(h->stream, with_sums ? h->sum : nullptr, h->sumsq, h->X, h->held, h->naccept, (long long)h->d.nchains, h->d.ndims,
                                h->pool_partial, out);
}

extern "C" klara_status klara_get_pooled_summaries(klara_handle* h, double* sum, double* sumsq,
                                                   uint64_t* naccept, uint64_t* ntransitions,
                                                   int64_t* nsaved_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const int D = h->d.ndims;
    if ((sum || sumsq) && !h->sum) return KLARA_ERR_STATE;
    HIPCHK(pool_summaries_async(h, sum || sumsq, h->pooled_out));
    std::vector<double> host(2 * (size_t)D + 1);
    HIPCHK(hipMemcpyAsync(host.data(), h->pooled_out, (2 * (size_t)D + 1) * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // one copy
    HIPCHK(hipStreamSynchronize(h->stream));
    if (sum) memcpy(sum, host.data(), D * sizeof(double));
    if (sumsq) memcpy(sumsq, host.data() + D, D * sizeof(double));
    if (naccept) memcpy(naccept, host.data() + 2 * D, sizeof(uint64_t));
    if (ntransitions) *ntransitions = (uint64_t)h->steps_done * (uint64_t)h->d.nchains;
    if (nsaved_out) *nsaved_out = h->nsaved;
    return KLARA_OK;
}

// ---- pooled moments without cancellation (the consumer is mean(chain) / var over every chain,
// src/stats/mean.jl:7-11).  sumsq/n - mean^2 from pooled raw sums loses mean^2/var digits (rats alpha_c: mean 242, sd 2.7 -> 4
// digits).  Here every chain's raw sums become (n_c, mean_c, M2_c) with the one cancelling subtraction, q - s^2/n, carried in
// double-double (s^2 = p + pe exactly by fma, the quotient's remainder by fma), and chains, blocks and ranks are merged by
// Chan's update — sums of non-negative terms only.  Fixed shapes => deterministic for a given chain count.
// (chan_merge and the per-chain (mean, M2) live in klara_rhat.h: the R-hat reduction forms and merges them with the same code)
__global__ __launch_bounds__(256) void k_moments_stage1(const double* __restrict__ sum, const double* __restrict__ sumsq,
                                                        const double* __restrict__ X, const long long* __restrict__ held,
                                                        long long N, int D, int nb, double nsaved, double* __restrict__ partial)
{
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < D; j += 256) {
        double n = 0.0, mean = 0.0, m2 = 0.0;
        for (long long c = b; c < N; c += nb) {                             // (a chain's sums over its saved steps: part + held * x)
            double mc, m2c;
            chain_moments(sum, sumsq, X, held, c, D, j, nsaved, mc, m2c);
            chan_merge(n, mean, m2, nsaved, mc, m2c);
        }
        partial[(long long)b * 2 * D + j] = mean;
        partial[(long long)b * 2 * D + D + j] = m2;
    }
}
// block j: dimension j.  Thread t merges the blocks' partials b = t, t + 256, ... (ascending), then a fixed tree over the threads.
// out[j] = mean, out[D + j] = M2 over the handle's chains; the count is nsaved * N.
__global__ __launch_bounds__(256) void k_moments_stage2(const double* __restrict__ partial, long long N, int D, int nb, double nsaved,
                                                        double* __restrict__ out)
{
    __shared__ double sn[256], sm[256], sq[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int b = t; b < nb; b += 256) {
        const long long chains = (N - b + nb - 1) / nb;                     // chains c = b, b + nb, ... < N
        chan_merge(n, mean, m2, nsaved * (double)chains, partial[(long long)b * 2 * D + j], partial[(long long)b * 2 * D + D + j]);
    }
    sn[t] = n; sm[t] = mean; sq[t] = m2;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (t < m) chan_merge(sn[t], sm[t], sq[t], sn[t + m], sm[t + m], sq[t + m]);
        __syncthreads();
    }
    if (t == 0) { out[j] = sm[0]; out[D + j] = sq[0]; }
}
// out: mean[D], M2[D], then the u64 accept total; partial as for pool_summaries_async
hipError_t pool_moments_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held,
                              const unsigned long long* naccept, long long N, int D, long long nsaved, double* partial, double* out)
{
    const int nb = (int)(N < KLARA_POOL_BLOCKS ? N : KLARA_POOL_BLOCKS);
    hipError_t e = pool_summaries_async(stream, nullptr, sumsq, X, held, naccept, N, D, partial, out);   // the accept total -> out[2 D]
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_moments_stage1, dim3(nb), dim3(256), 0, stream, sum, sumsq, X, held, N, D, nb, (double)nsaved, partial);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_moments_stage2, dim3(D), dim3(256), 0, stream, partial, N, D, nb, (double)nsaved, out);
    return hipGetLastError();
}
hipError_t pool_moments_async(klara_handle* h, double* out)
{
    return pool_moments_async(h->stream, h->sum, h->sumsq, h->X, h->held, h->naccept, (long long)h->d.nchains, h->d.ndims, (long long)h->nsaved,
                              h->pool_partial, out);
}

// Columns [first, first + count) of the saved steps from a history buffer whose column c lives at slot c % hist_cols (ring) or c:
// `width` bytes per column copied to consecutive rows of dst, `stride` bytes between the buffer's columns.
static hipError_t copy_saved_columns(const klara_handle* h, void* dst, const char* src, size_t width, size_t stride, long long first, long long count)
{
    long long done = 0;
    while (done < count) {
        const long long slot = h->ring ? (first + done) % h->hist_cols : first + done;
        long long run = count - done;
        if (h->ring && slot + run > h->hist_cols) run = h->hist_cols - slot;
        const hipError_t e = hipMemcpy2D((char*)dst + (size_t)done * width, width, src + (size_t)slot * stride, stride, width, (size_t)run, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        done += run;
    }
    return hipSuccess;
}
// the saved steps a history read returns: all of them, or the last hist_cols of a ring
static void saved_window(const klara_handle* h, long long capacity, long long* first, long long* count)
{
    const long long avail = h->ring && h->nsaved > h->hist_cols ? h->hist_cols : h->nsaved;
    *count = avail < capacity ? avail : capacity;
    *first = h->nsaved - avail;
}

extern "C" klara_status klara_get_chain(klara_handle* h, int64_t local_chain, double* value,
                                        int64_t capacity_cols, int64_t* ncols_out)
{
    if (!h || local_chain < 0 || local_chain >= h->d.nchains) return KLARA_ERR_INVALID_ARG;
    if (!h->hist || !(h->d.monitor & KLARA_MON_HISTORY)) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    long long first, n;
    saved_window(h, capacity_cols, &first, &n);
    // device layout [col][chain][D] -> Klara NState.value (D x n) column-major = n contiguous D-vectors
    if (value && n > 0)
        HIPCHK(copy_saved_columns(h, value, (const char*)(h->hist + (size_t)local_chain * D), D * sizeof(double), N * D * sizeof(double), first, n));
    if (ncols_out) { long long f2, all; saved_window(h, 0x7fffffffffffffffll, &f2, &all); *ncols_out = all; }
    return KLARA_OK;
}

extern "C" klara_status klara_get_chain_fields(klara_handle* h, int64_t local_chain, double* logtarget,
                                               double* gradlogtarget, int64_t capacity_cols, int64_t* ncols_out)
{
    if (!h || local_chain < 0 || local_chain >= h->d.nchains) return KLARA_ERR_INVALID_ARG;
    if ((logtarget && !h->hist_lt) || (gradlogtarget && !h->hist_g) || (!h->hist_lt && !h->hist_g)) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    long long first, n;
    saved_window(h, capacity_cols, &first, &n);
    if (logtarget && n > 0)
        HIPCHK(copy_saved_columns(h, logtarget, (const char*)(h->hist_lt + (size_t)local_chain), sizeof(double), N * sizeof(double), first, n));
    if (gradlogtarget && n > 0)
        HIPCHK(copy_saved_columns(h, gradlogtarget, (const char*)(h->hist_g + (size_t)local_chain * D), D * sizeof(double), N * D * sizeof(double), first, n));
    if (ncols_out) { long long f2, all; saved_window(h, 0x7fffffffffffffffll, &f2, &all); *ncols_out = all; }
    return KLARA_OK;
}

extern "C" klara_status klara_get_chain_likelihood_prior(klara_handle* h, int64_t local_chain, double* loglikelihood, double* logprior,
                                                         int64_t capacity_cols, int64_t* ncols_out)
{
    if (!h || local_chain < 0 || local_chain >= h->d.nchains) return KLARA_ERR_INVALID_ARG;
    if (!h->hist_ll) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains;
    long long first, n;
    saved_window(h, capacity_cols, &first, &n);
    if (loglikelihood && n > 0)
        HIPCHK(copy_saved_columns(h, loglikelihood, (const char*)(h->hist_ll + (size_t)local_chain), sizeof(double), N * sizeof(double), first, n));
    if (logprior && n > 0)
        HIPCHK(copy_saved_columns(h, logprior, (const char*)(h->hist_lp + (size_t)local_chain), sizeof(double), N * sizeof(double), first, n));
    if (ncols_out) { long long f2, all; saved_window(h, 0x7fffffffffffffffll, &f2, &all); *ncols_out = all; }
    return KLARA_OK;
}

// Post-hoc Monte Carlo variance estimators of src/stats/variance/mcvar.jl over the stored history, one thread per
// (chain, dimension) series; consecutive threads read consecutive dimensions of one chain (coalesced).
//   iid  : var(v)/n                                   (mcvar.jl:5)
//   bm   : batchlen * var(batch means) / nbsamples    (mcvar.jl:35-41, Flegal & Jones)
//   imse : Geyer's initial monotone sequence estimator on the empirical autocovariance (mcvar.jl:75-105);
//          autocov(v, k) = sum_t (v_t - m)(v_{t+k} - m) / n  (StatsBase, demean = true), evaluated lag pair by lag
//          pair until the first non-positive pair sum, so the cost is O(n * stopping lag) instead of O(n^2).
__global__ __launch_bounds__(256) void k_chain_stats(const double* __restrict__ hist, long long ncols, long long N, int D,
                                                     long long batchlen, long long maxlag, double* iid, double* bm,
                                                     double* imse, double* ipse)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const double* v = hist + i;                 // v[t * stride]
    const long long stride = N * D, n = ncols;
    // Deviations as (v_t - v_0) - mean(v - v_0): the first difference is exact or nearly so, and the mean of the differences carries an error of
    // n u |v - v_0| where the mean of v carries n u |v| — which, at a mean of 1e6 sd, already costs 1e-9 of imse (profiles/chain_stats_accuracy.txt).
    // A series that never moves has every deviation exactly 0 (0 / 0 = NaN for its ESS, as in the reference's arithmetic, not a ratio of noise).
    const double v0 = v[0];
    double m = 0.0;
    for (long long t = 0; t < n; ++t) m += v[t * stride] - v0;
    m /= (double)n;
    double acv0 = 0.0;
    for (long long t = 0; t < n; ++t) { const double z = (v[t * stride] - v0) - m; acv0 += z * z; }
    if (iid) iid[i] = (n > 1) ? acv0 / (double)(n - 1) / (double)n : NAN;
    if (bm) {
        const long long nb = batchlen > 0 ? n / batchlen : 0;
        if (nb > 1) {
            double sb = 0.0, sb2 = 0.0;                       // two-pass over the batch means (of v - v_0: the variance does not depend on a shift)
            for (long long b = 0; b < nb; ++b) {
                double a = 0.0;
                for (long long t = 0; t < batchlen; ++t) a += v[(b * batchlen + t) * stride] - v0;
                sb += a / (double)batchlen;
            }
            const double mb = sb / (double)nb;
            for (long long b = 0; b < nb; ++b) {
                double a = 0.0;
                for (long long t = 0; t < batchlen; ++t) a += v[(b * batchlen + t) * stride] - v0;
                const double dm = a / (double)batchlen - mb;
                sb2 += dm * dm;
            }
            bm[i] = (double)batchlen * (sb2 / (double)(nb - 1)) / (double)(nb * batchlen);
        } else bm[i] = NAN;                                   // "Choose batch size such that the number of batches is > 1"
    }
    if (imse || ipse) {
        const long long ml = maxlag < n - 1 ? maxlag : n - 1;
        const long long k = (ml - 1) / 2;                     // floor((maxlag-1)/2), mcvar.jl:76
        double gsum = 0.0, gprev = 0.0, gsum_p = 0.0;
        for (long long j = 0; j <= k; ++j) {
            double a0 = 0.0, a1 = 0.0;
            const long long l0 = 2 * j, l1 = 2 * j + 1;
            if (j == 0) a0 = acv0;
            else for (long long t = 0; t + l0 < n; ++t) a0 += ((v[t * stride] - v0) - m) * ((v[(t + l0) * stride] - v0) - m);
            for (long long t = 0; t + l1 < n; ++t) a1 += ((v[t * stride] - v0) - m) * ((v[(t + l1) * stride] - v0) - m);
            double gj = (a0 + a1) / (double)n;
            if (gj <= 0.0) break;                             // m = j (mcvar.jl:87-90)
            gsum_p += gj;                                     // initial positive sequence (mcvar.jl:137-158): no monotone step
            if (j > 0 && gj > gprev) gj = gprev;              // monotone sequence (mcvar.jl:94-100)
            gsum += gj; gprev = gj;
        }
        if (imse) imse[i] = (-acv0 / (double)n + 2.0 * gsum) / (double)n;
        if (ipse) ipse[i] = (-acv0 / (double)n + 2.0 * gsum_p) / (double)n;
    }
}

hipError_t launch_chain_stats(hipStream_t stream, const double* hist, long long ncols, long long N, int D, long long batchlen, long long maxlag,
                              double* iid, double* bm, double* imse, double* ipse)
{
    hipLaunchKernelGGL(k_chain_stats, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, stream, hist, ncols, N, D, batchlen, maxlag, iid, bm, imse, ipse);
    return hipGetLastError();
}

extern "C" klara_status klara_get_chain_mcvar(klara_handle* h, int64_t batchlen, int64_t maxlag, double* mcvar_iid,
                                              double* mcvar_bm, double* mcvar_imse)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->hist || h->ring || !(h->d.monitor & KLARA_MON_HISTORY) || !h->have_state || h->nsaved < 2) return KLARA_ERR_STATE;   // (needs every saved step)
    HIPCHK(hipSetDevice(h->d.device));
    const long long N = h->d.nchains, D = h->d.ndims, total = N * D;
    double* buf = nullptr;
    HIPCHK(dalloc(&buf, (size_t)3 * total));
    hipError_t e = launch_chain_stats(h->stream, h->hist, (long long)h->nsaved, N, (int)D, (long long)batchlen, (long long)(maxlag > 0 ? maxlag : h->nsaved - 1),
                                      mcvar_iid ? buf : nullptr, mcvar_bm ? buf + total : nullptr, mcvar_imse ? buf + 2 * total : nullptr, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && mcvar_iid) e = hipMemcpy(mcvar_iid, buf, total * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mcvar_bm) e = hipMemcpy(mcvar_bm, buf + total, total * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mcvar_imse) e = hipMemcpy(mcvar_imse, buf + 2 * total, total * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(buf);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

extern "C" klara_status klara_get_chain_mcvar_ipse(klara_handle* h, int64_t maxlag, double* mcvar_ipse)
{
    if (!h || !mcvar_ipse) return KLARA_ERR_INVALID_ARG;
    if (!h->hist || h->ring || !(h->d.monitor & KLARA_MON_HISTORY) || !h->have_state || h->nsaved < 2) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const long long N = h->d.nchains, D = h->d.ndims, total = N * D;
    double* buf = nullptr;
    HIPCHK(dalloc(&buf, (size_t)total));
    hipError_t e = launch_chain_stats(h->stream, h->hist, (long long)h->nsaved, N, (int)D, 0ll, (long long)(maxlag > 0 ? maxlag : h->nsaved - 1),
                                      nullptr, nullptr, nullptr, buf);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(mcvar_ipse, buf, total * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(buf);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

extern "C" klara_status klara_get_chain_bm(klara_handle* h, double* mcvar_bm, int64_t* nbatches_out)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->bm_prev || !h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->d.nchains * (size_t)h->d.ndims;
    const long long nb = h->bm_count;
    if (mcvar_bm) {
        HIPCHK(hipMemcpy(mcvar_bm, h->bm_m2, n * sizeof(double), hipMemcpyDeviceToHost));
        // batchlen * var(batch means) / (nbatches * batchlen)  (mcvar.jl:39-41), var = M2 / (nbatches - 1)
        for (size_t i = 0; i < n; ++i)
            mcvar_bm[i] = nb > 1 ? (double)h->d.bm_batchlen * (mcvar_bm[i] / (double)(nb - 1)) / (double)(nb * h->d.bm_batchlen) : (double)NAN;
    }
    if (nbatches_out) *nbatches_out = nb;
    return KLARA_OK;
}

extern "C" klara_status klara_get_tune(klara_handle* h, double* step, int64_t* accepted, int64_t* proposed,
                                       int64_t* totproposed)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains;
    if (h->d.tuner_mode == KLARA_TUNE_POOLED) {
        double s; long long a, pr, t;
        HIPCHK(hipMemcpy(&s, h->tune_step, sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&a, h->tune_acc, sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&pr, h->tune_prop, sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&t, h->tune_tot, sizeof(long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; ++i) {
            if (step) step[i] = s;
            if (accepted) accepted[i] = a;
            if (proposed) proposed[i] = pr;
            if (totproposed) totproposed[i] = t;
        }
        return KLARA_OK;
    }
    if (step) HIPCHK(hipMemcpy(step, h->tune_step, N * sizeof(double), hipMemcpyDeviceToHost));
    if (accepted) HIPCHK(hipMemcpy(accepted, h->tune_acc, N * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (proposed) HIPCHK(hipMemcpy(proposed, h->tune_prop, N * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (totproposed) HIPCHK(hipMemcpy(totproposed, h->tune_tot, N * sizeof(int64_t), hipMemcpyDeviceToHost));
    return KLARA_OK;
}

extern "C" klara_status klara_get_dual_averaging(klara_handle* h, double* epsbar, double* hbar)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state || !h->da_epsbar) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains;
    if (epsbar) HIPCHK(hipMemcpy(epsbar, h->da_epsbar, N * sizeof(double), hipMemcpyDeviceToHost));
    if (hbar) HIPCHK(hipMemcpy(hbar, h->da_hbar, N * sizeof(double), hipMemcpyDeviceToHost));
    return KLARA_OK;
}

// The samplers' per-chain adaptive arrays are planes — plane k holds entry k of every chain, N values — and the API's arrays are chain-major rows of `row`
// entries.  read_planes gathers out[c * row + i] = plane map(i) of chain c (map(i) < 0: zero), write_planes scatters the entries with map(i) >= 0 back.
template <class T, class Map>
static klara_status read_planes(const T* dev, size_t nplanes, size_t N, size_t row, Map map, T* out)
{
    std::vector<T> planes(nplanes * N);
    HIPCHK(hipMemcpy(planes.data(), dev, planes.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < N; ++c)
        for (size_t i = 0; i < row; ++i) { const long long k = map(i); out[c * row + i] = k < 0 ? T(0) : planes[(size_t)k * N + c]; }
    return KLARA_OK;
}
template <class T, class Map>
static klara_status write_planes(T* dev, size_t nplanes, size_t N, size_t row, Map map, const T* in)
{
    std::vector<T> planes(nplanes * N);
    for (size_t c = 0; c < N; ++c)
        for (size_t i = 0; i < row; ++i) { const long long k = map(i); if (k >= 0) planes[(size_t)k * N + c] = in[c * row + i]; }
    HIPCHK(hipMemcpy(dev, planes.data(), planes.size() * sizeof(T), hipMemcpyHostToDevice));
    return KLARA_OK;
}
static long long plane_lower(size_t D, size_t ij) { const int i = (int)(ij / D), j = (int)(ij % D); return j <= i ? (long long)ktri(j, i, (int)D) : -1ll; }   // entry (i, j) of a row-major D x D lower triangle
static const auto plane_same = [](size_t i) { return (long long)i; };                      // a vector per chain: entry i is plane i
static klara_status read_counter(const unsigned long long* dev, int64_t* out)
{
    unsigned long long k = 0;
    HIPCHK(hipMemcpy(&k, dev, sizeof(k), hipMemcpyDeviceToHost));
    *out = (int64_t)k;
    return KLARA_OK;
}

extern "C" klara_status klara_get_ram_factor(klara_handle* h, double* S, int64_t* skipped)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_RAM) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    if (S) KCHK(read_planes(h->ram_S, D * (D + 1) / 2, N, D * D, [D](size_t ij) { return plane_lower(D, ij); }, S));
    if (skipped) KCHK(read_counter(h->ram_skipped, skipped));
    return KLARA_OK;
}

extern "C" klara_status klara_set_ram_factor(klara_handle* h, const double* S)
{
    if (!h || !S || h->d.sampler != KLARA_SAMPLER_RAM) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    for (size_t c = 0; c < N; ++c)
        for (size_t i = 0; i < D; ++i)
            if (!(S[(c * D + i) * D + i] > 0.0) || !std::isfinite(S[(c * D + i) * D + i])) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return write_planes(h->ram_S, D * (D + 1) / 2, N, D * D, [D](size_t ij) { return plane_lower(D, ij); }, S);
}

extern "C" klara_status klara_get_am_state(klara_handle* h, double* Cout, double* lastmean, double* secondlastmean, int64_t* fallbacks)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_AM) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    const auto symmetric = [D](size_t ij) { const int i = (int)(ij / D), j = (int)(ij % D); return (long long)ktri(i < j ? i : j, i < j ? j : i, (int)D); };
    if (Cout) KCHK(read_planes(h->am_C, D * (D + 1) / 2, N, D * D, symmetric, Cout));
    if (lastmean) KCHK(read_planes(h->am_mean, D, N, D, plane_same, lastmean));
    if (secondlastmean) KCHK(read_planes(h->am_mean + D * N, D, N, D, plane_same, secondlastmean));
    if (fallbacks) KCHK(read_counter(h->am_fallbacks, fallbacks));
    return KLARA_OK;
}

extern "C" klara_status klara_get_amwg_state(klara_handle* h, double* logsigma, int32_t* accepted, uint64_t* naccept_coord)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_AMWG) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    if (logsigma) KCHK(read_planes(h->amwg_logsig, D, N, D, plane_same, logsigma));
    if (accepted) KCHK(read_planes((const int32_t*)h->amwg_acc, D, N, D, plane_same, accepted));
    if (naccept_coord) {                                         // the closed windows' counts + the open window's
        std::vector<int32_t> open(N * D);
        KCHK(read_planes((const uint64_t*)h->amwg_nacc, D, N, D, plane_same, naccept_coord));
        KCHK(read_planes((const int32_t*)h->amwg_acc, D, N, D, plane_same, open.data()));
        for (size_t k = 0; k < N * D; ++k) naccept_coord[k] += (uint64_t)open[k];
    }
    return KLARA_OK;
}

extern "C" klara_status klara_set_amwg_logsigma(klara_handle* h, const double* logsigma)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_AMWG || !logsigma) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    const size_t N = (size_t)h->d.nchains, D = (size_t)h->d.ndims;
    for (size_t k = 0; k < N * D; ++k) if (!std::isfinite(logsigma[k])) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    return write_planes(h->amwg_logsig, D, N, D, plane_same, logsigma);
}

extern "C" klara_status klara_get_amwg_accept_mask(klara_handle* h, uint32_t* mask, int64_t capacity_steps, int64_t* nsteps_out)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_AMWG || capacity_steps < 0) return KLARA_ERR_INVALID_ARG;
    if (!h->amwg_mask) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const long long n = h->steps_done < capacity_steps ? h->steps_done : capacity_steps;
    if (mask && n > 0) HIPCHK(hipMemcpy(mask, h->amwg_mask, (size_t)n * (size_t)h->d.nchains * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (nsteps_out) *nsteps_out = h->steps_done;
    return KLARA_OK;
}

// MH(Σ): the job's factor — one triangle for all chains, so no planes: the packed rows as KParams::mh_factor holds them
extern "C" klara_status klara_get_mh_factor(klara_handle* h, double* Lout)
{
    if (!h || h->d.sampler != KLARA_SAMPLER_MH_COV) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!Lout) return KLARA_OK;
    std::vector<double> tri(KLARA_MHCOV_TRI);
    HIPCHK(hipMemcpy(tri.data(), h->mh_factor, tri.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t D = (size_t)h->d.ndims;
    for (size_t i = 0; i < D; ++i)
        for (size_t k = 0; k < D; ++k) Lout[i * D + k] = k <= i ? tri[i * (i + 1) / 2 + k] : 0.0;
    return KLARA_OK;
}

extern "C" klara_status klara_set_mh_factor(klara_handle* h, const double* Lin)
{
    if (!h || !Lin || h->d.sampler != KLARA_SAMPLER_MH_COV) return KLARA_ERR_INVALID_ARG;
    std::vector<double> tri;
    if (!pack_mh_factor(Lin, h->d.ndims, tri)) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));                     // (the transitions queued so far read the factor they were queued with)
    HIPCHK(hipMemcpy(h->mh_factor, tri.data(), tri.size() * sizeof(double), hipMemcpyHostToDevice));
    return KLARA_OK;
}

extern "C" klara_status klara_device_ptrs(klara_handle* h, void** x, void** logtarget, void** gradlogtarget)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (x) *x = h->X;
    if (logtarget) *logtarget = h->LT;
    if (gradlogtarget) *gradlogtarget = h->GR;
    return KLARA_OK;
}

extern "C" klara_status klara_get_layout(klara_handle* h, int32_t* kind, int32_t* lanes_per_chain,
                                         int32_t* elems_per_lane)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (kind) *kind = h->plan.kind;
    if (lanes_per_chain) *lanes_per_chain = h->plan.kind == 2 ? h->plan.RS : h->plan.G;
    if (elems_per_lane) *elems_per_lane = h->plan.E;
    return KLARA_OK;
}

extern "C" klara_status klara_get_kernel_attributes(klara_handle* h, int32_t which, int32_t nsteps, int32_t* vgprs, int32_t* scratch_bytes,
                                                    int32_t* static_lds_bytes)
{
    if (!h || nsteps < 1 || which < 0 || which > 1) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    hipFuncAttributes a;
    memset(&a, 0, sizeof(a));
    KLaunch kl;
    kl.group0 = 0; kl.group_end = 0x7fffffffffffffffll; kl.t0 = 0; kl.nsteps = nsteps; kl.save_phase0 = 0; kl.save_col0 = 0;
    h->query_lanes = which == 1 ? 8 : 4;
    klara_attr_query = &a;
    const hipError_t e = launch_steps(h, kl, 1);
    klara_attr_query = nullptr;
    HIPCHK(e);
    if (vgprs) *vgprs = a.numRegs;
    if (scratch_bytes) *scratch_bytes = (int32_t)a.localSizeBytes;
    if (static_lds_bytes) *static_lds_bytes = (int32_t)a.sharedSizeBytes;
    return KLARA_OK;
}

extern "C" klara_status klara_get_shader_clock(klara_handle* h, double* mhz)
{
    if (!h || !mhz) return KLARA_ERR_INVALID_ARG;
    *mhz = 0.0;
    if (!h->clock_probe) return KLARA_OK;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int j = 0; j < 3; ++j) if (h->side[j]) HIPCHK(hipStreamSynchronize(h->side[j]));
    unsigned long long v[4] = { 0, 0, 0, 0 };
    HIPCHK(hipMemcpy(v, h->clock_probe, sizeof(v), hipMemcpyDeviceToHost));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->d.device) != hipSuccess || khz <= 0) { (void)hipGetLastError(); khz = 100000; }
    if (v[1] > v[3] && v[0] > v[2]) *mhz = (double)(v[0] - v[2]) / (double)(v[1] - v[3]) * (double)khz * 1e-3;
    return KLARA_OK;
}

extern "C" klara_status klara_get_launch_modes(klara_handle* h, int64_t counts[3], int32_t last_mode[4], int64_t last_accepted[4])
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (counts) for (int i = 0; i < 3; ++i) counts[i] = h->n_launch_mode[i];
    for (int j = 0; j < 4; ++j) {
        const bool have = h->auto_mirror != nullptr;
        if (last_mode) last_mode[j] = have ? __atomic_load_n(h->auto_mirror + 4 * j, __ATOMIC_ACQUIRE) : -1;
        if (last_accepted) last_accepted[j] = have ? __atomic_load_n(h->auto_mirror + 4 * j + 1, __ATOMIC_RELAXED) : -1;
    }
    return KLARA_OK;
}
