// klara_selftest.hip — self tests: the device's random blocks, math, normals and matrix-core probes as the kernels see them; the chain statistics kernels on a
// caller's series; the across-chain reductions and the R-hat kernels on a caller's chain sums and histories; compile checks of user targets.
#include <rocrand/rocrand_kernel.h>
#include "klara_handle.h"
#include "klara_rhat.h"
#include "klara_ess.h"

__global__ void k_rocrand_blocks(unsigned long long seed, unsigned long long subseq,
                                 unsigned long long first_block, int nblocks, unsigned int* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, subseq, 4ull * (first_block + (unsigned long long)i), &st);
    const uint4 r = rocrand4(&st);
    out[4 * i + 0] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
}

extern "C" klara_status klara_selftest_rocrand_blocks(int32_t device, uint64_t seed, uint64_t subsequence,
                                                      uint64_t first_block, int32_t nblocks, uint32_t* out)
{
    if (!out || nblocks <= 0) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    unsigned int* d = nullptr;
    HIPCHK(dalloc(&d, (size_t)4 * nblocks));
    hipError_t e = klara_start(k_rocrand_blocks, dim3((nblocks + 63) / 64), dim3(64), 0, (hipStream_t)0, (unsigned long long)seed,
                               (unsigned long long)subsequence, (unsigned long long)first_block, (int)nblocks, d);
    if (e == hipSuccess) e = hipMemcpy(out, d, sizeof(uint32_t) * 4 * (size_t)nblocks, hipMemcpyDeviceToHost);
    (void)dfree(d);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

__global__ void k_math(int op, long long n, const double* in, const double* in2, double* out)
{
    kd_tables_to_lds();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    switch (op) {
    case 0: out[i] = kd_log(in[i]); break;
    case 1: out[i] = kd_exp(in[i]); break;
    case 2: kd_sincos2pi(in[i], &s, &c); out[i] = s; break;
    case 3: kd_sincos2pi(in[i], &s, &c); out[i] = c; break;
    case 4: out[i] = __builtin_sqrt(in[i]); break;
    case 6: out[i] = kd_erf(in[i]); break;
    case 7: out[i] = kd_log_u01(in[i]); break;
    case 8: out[i] = kd_sqrt_radicand(in[i]); break;
    case 9: out[i] = kd_exp_neg(in[i]); break;
    case 10: kd_softplus_logistic(in[i], &s, &c); out[i] = s; break;
    case 11: kd_softplus_logistic(in[i], &s, &c); out[i] = c; break;
    case 12: out[i] = kd_log12(in[i]); break;
    // the 20-bit angle of kd_normal_pair_w at index k = in[i] (0 <= k < 2^20), arithmetic form: sin, cos  (ops 13 / 14 are its table form, k_math_sctab)
    case 15: kd_sincos2pi_bits(kd_angle_bits20((uint32_t)in[i] << 12), &s, &c); out[i] = s; break;
    case 16: kd_sincos2pi_bits(kd_angle_bits20((uint32_t)in[i] << 12), &s, &c); out[i] = c; break;
    default: out[i] = in[i] / in2[i]; break;
    }
}

// ops 13 / 14: sin / cos of the same angle through the remainder table (kd_sincos2pi_tab20), which every workgroup fills first — as the transition
// kernels that take the table do (klara_diagt.h SCTAB)
__global__ __launch_bounds__(256) void k_math_sctab(int op, long long n, const double* in, double* out)
{
    kd_sincos_rem_to_lds();
    kd_tables_to_lds();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s, c;
    kd_sincos2pi_tab20((uint32_t)in[i] << 12, &s, &c);
    out[i] = op == 13 ? s : c;
}

extern "C" klara_status klara_selftest_math(int32_t device, int32_t op, int64_t n, const double* in,
                                            const double* in2, double* out)
{
    if (!in || !out || n <= 0) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    double *di = nullptr, *di2 = nullptr, *dout = nullptr;
    hipError_t e = dalloc(&di, (size_t)n);
    if (e == hipSuccess) e = dalloc(&di2, (size_t)n);
    if (e == hipSuccess) e = dalloc(&dout, (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(di, in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(di2, in2 ? in2 : in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (op == 13 || op == 14) {
            // (4,096 results per workgroup: the fill is a quarter of a workgroup's work, not all of it)
            e = klara_start(k_math_sctab, dim3((unsigned)((n + 255) / 256)), dim3(256), (size_t)KD_SCREM_BYTES, (hipStream_t)0, op, (long long)n, di, dout);
        } else {
            e = klara_start(k_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)0, op, (long long)n, di, di2, dout);
        }
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
    (void)dfree(di); (void)dfree(di2); (void)dfree(dout);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

// |z| exceedance counts and raw power sums of the proposal normals, drawn exactly as the transition kernels draw them
// (kd_normal_pair_w on both halves of kd_stream_block(seed, chain, transition, slot 0)); one thread per chain, one atomic per thread
// and threshold.  counts[k] = #{|z| > thr[k]} over 4 * nchains * ntransitions normals.
__global__ __launch_bounds__(256) void k_normal_tail(unsigned long long seed, unsigned long long first_chain, long long nchains,
                                                     long long ntransitions, int nthr, const double* __restrict__ thr,
                                                     unsigned long long* __restrict__ counts, double* __restrict__ moments)
{
    kd_tables_to_lds();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = i < nchains;
    unsigned long long c[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    double s1 = 0.0, s2 = 0.0, s4 = 0.0, mx = 0.0;
    for (long long t = 0; t < ntransitions; ++t) {
        const kd_u32x4 b = kd_stream_block(seed, first_chain + (unsigned long long)(ok ? i : 0), (unsigned long long)t, 0u);
        for (int h = 0; h < 2; ++h) {                           // the block's two pairs: pair indices 0 and 8 of a transition
            double z0, z1, u1, lg;
            kd_normal_pair_w(h ? b.z : b.x, h ? b.w : b.y, &z0, &z1, &u1, &lg);
            if (!ok) continue;
            const double a0 = z0 < 0.0 ? -z0 : z0, a1 = z1 < 0.0 ? -z1 : z1;
            for (int k = 0; k < 8; ++k) if (k < nthr) c[k] += (a0 > thr[k] ? 1ull : 0ull) + (a1 > thr[k] ? 1ull : 0ull);
            s1 += z0 + z1; s2 += z0 * z0 + z1 * z1; s4 += (z0 * z0) * (z0 * z0) + (z1 * z1) * (z1 * z1);
            mx = a0 > mx ? a0 : mx; mx = a1 > mx ? a1 : mx;
        }
    }
    for (int k = 0; k < 8; ++k) if (k < nthr && c[k] != 0) atomicAdd(&counts[k], c[k]);
    if (ok) {
        atomicAdd(&moments[0], s1); atomicAdd(&moments[1], s2); atomicAdd(&moments[2], s4);
        atomicMax((unsigned long long*)&moments[3], (unsigned long long)__double_as_longlong(mx));   // (non-negative doubles order like integers)
    }
}

extern "C" klara_status klara_selftest_normal_tail(int32_t device, uint64_t seed, uint64_t first_chain, int64_t nchains,
                                                   int64_t ntransitions, int32_t nthr, const double* thr, uint64_t* counts,
                                                   double* moments)
{
    if (!thr || !counts || nthr <= 0 || nthr > 8 || nchains <= 0 || ntransitions <= 0) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    double* dthr = nullptr; unsigned long long* dc = nullptr; double* dm = nullptr;
    hipError_t e = dalloc(&dthr, 8);
    if (e == hipSuccess) e = dalloc(&dc, 8);
    if (e == hipSuccess) e = dalloc(&dm, 4);
    if (e == hipSuccess) e = hipMemcpy(dthr, thr, sizeof(double) * (size_t)nthr, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dc, 0, 8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(dm, 0, 4 * sizeof(double));
    if (e == hipSuccess) e = klara_start(k_normal_tail, dim3((unsigned)((nchains + 255) / 256)), dim3(256), 0, (hipStream_t)0, (unsigned long long)seed,
                                         (unsigned long long)first_chain, (long long)nchains, (long long)ntransitions, (int)nthr, dthr, dc, dm);
    if (e == hipSuccess) e = hipMemcpy(counts, dc, sizeof(uint64_t) * (size_t)nthr, hipMemcpyDeviceToHost);
    if (e == hipSuccess && moments) e = hipMemcpy(moments, dm, 4 * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(dthr); (void)dfree(dc); (void)dfree(dm);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

extern "C" klara_status klara_selftest_mfma_f64(int32_t device, const double* A, const double* B,
                                                const double* C, double* D)
{
    if (!A || !B || !C || !D) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    double* buf = nullptr;
    HIPCHK(dalloc(&buf, 64 + 64 + 256 + 256));
    hipError_t e = hipMemcpy(buf, A, 64 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 64, B, 64 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 128, C, 256 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = klara_launch_mfma_probe(buf, buf + 64, buf + 128, buf + 384, 0);
    if (e == hipSuccess) e = hipMemcpy(D, buf + 384, 256 * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(buf);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

extern "C" klara_status klara_selftest_mfma_f64_4x4x4(int32_t device, const double* A, const double* B,
                                                      const double* C, double* D)
{
    if (!A || !B || !C || !D) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    double* buf = nullptr;
    HIPCHK(dalloc(&buf, 256));
    hipError_t e = hipMemcpy(buf, A, 64 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 64, B, 64 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + 128, C, 64 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = klara_launch_mfma4_probe(buf, buf + 64, buf + 128, buf + 192, 0);
    if (e == hipSuccess) e = hipMemcpy(D, buf + 192, 64 * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(buf);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

// The chain statistics kernels on a caller's series: k_chain_stats over the uploaded history, then the streaming autocovariances launch by launch
// (launch_acov_update with col0 running through the history, as klara_run issues them; an empty launch is skipped there too) and their finalize step.
extern "C" klara_status klara_selftest_chain_stats(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t maxlag,
                                                   int64_t batchlen, int32_t nsplits, const int64_t* splits, double* iid, double* bm, double* imse,
                                                   double* ipse, double* stream_imse, double* stream_ipse)
{
    if (!hist || !splits || nchains <= 0 || ndims <= 0 || ncols < 2 || maxlag < 1 || maxlag > 127 || nsplits <= 0 || batchlen < 0) return KLARA_ERR_INVALID_ARG;
    long long sum = 0;
    for (int j = 0; j < nsplits; ++j) {
        if (splits[j] < 0 || splits[j] > 0x7fffffffll) return KLARA_ERR_INVALID_ARG;
        sum += splits[j];
    }
    if (sum != ncols) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const long long nd = (long long)nchains * ndims;
    const int W = maxlag + 1;
    const size_t ws = (size_t)W * nd;
    double *dh = nullptr, *S = nullptr, *head = nullptr, *tail = nullptr, *near = nullptr, *total = nullptr, *out = nullptr;
    hipError_t e = dalloc(&dh, (size_t)ncols * nd);
    if (e == hipSuccess) e = dalloc(&S, ws);
    if (e == hipSuccess) e = dalloc(&head, ws);
    if (e == hipSuccess) e = dalloc(&tail, ws);
    if (e == hipSuccess && W > 32) e = dalloc(&near, (size_t)32 * nd);
    if (e == hipSuccess) e = dalloc(&total, (size_t)nd);
    if (e == hipSuccess) e = dalloc(&out, (size_t)6 * nd);
    if (e == hipSuccess) e = hipMemcpy(dh, hist, (size_t)ncols * nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(S, 0, ws * sizeof(double));           // (what klara_set_state / klara_reset leave)
    if (e == hipSuccess) e = hipMemset(head, 0, ws * sizeof(double));
    if (e == hipSuccess) e = hipMemset(tail, 0, ws * sizeof(double));
    if (e == hipSuccess) e = hipMemset(total, 0, (size_t)nd * sizeof(double));
    const hipStream_t st = 0;
    if (e == hipSuccess) e = launch_chain_stats(st, dh, (long long)ncols, (long long)nchains, (int)ndims, (long long)batchlen, (long long)maxlag,
                                                out, out + nd, out + 2 * nd, out + 3 * nd);
    long long col0 = 0;
    for (int j = 0; j < nsplits && e == hipSuccess; ++j) {
        if (splits[j] > 0) e = launch_acov_update(st, dh, S, head, tail, near, total, col0, W, nd, col0, (long long)splits[j]);
        col0 += splits[j];
    }
    if (e == hipSuccess) e = launch_acov_finalize(st, S, head, tail, total, (long long)ncols, W, nd, out + 4 * nd, out + 5 * nd);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    double* dst[6] = { iid, bm, imse, ipse, stream_imse, stream_ipse };
    for (int k = 0; k < 6 && e == hipSuccess; ++k)
        if (dst[k]) e = hipMemcpy(dst[k], out + (size_t)k * nd, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost);
    (void)dfree(dh); (void)dfree(S); (void)dfree(head); (void)dfree(tail); if (near) (void)dfree(near); (void)dfree(total); (void)dfree(out);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

// The simulated ranks of the self tests below: one MergeLayout staging buffer per rank, all in one device array, merged by merge_ranks (klara_merge.h)
// — the very sequence klara_gather_moments / klara_gather_covariance / klara_gather_rhat run — with every all-reduce replaced by a host sum of the ranks' slices in
// ascending order of the ranks, starting from 0.0 / 0, written back to every rank.
struct SimRanks {
    MergeLayout L; hipStream_t st;
    std::vector<double*> buf; std::vector<double> n_r;
    hipError_t alloc(DeviceArrays& mem, int nranks)
    {
        double* rb = nullptr;
        const hipError_t e = mem.alloc(&rb, (size_t)nranks * L.size());
        for (int r = 0; r < nranks && e == hipSuccess; ++r) buf.push_back(rb + (size_t)r * L.size());
        n_r.assign((size_t)nranks, 0.0);
        return e;
    }
    // rank r's counters (has_accepted: slot 0 is on the device already, behind pool_moments_async's mean_r | M2_r)
    hipError_t set_counters(int r, unsigned long long nsamples, unsigned long long nchains, bool has_accepted)
    {
        const unsigned long long cnt[MergeLayout::NCOUNTERS] = { 0, 0, nsamples, nchains };
        const int first = has_accepted ? 1 : 0;
        n_r[r] = (double)nsamples;
        return hipMemcpy(buf[r] + L.counters() + first, cnt + first, (MergeLayout::NCOUNTERS - first) * sizeof(cnt[0]), hipMemcpyHostToDevice);
    }
    // rank r's counters of the R-hat form: m units of n samples each
    hipError_t set_rhat_counters(int r, unsigned long long m, unsigned long long n)
    {
        unsigned long long cnt[MergeLayout::NCOUNTERS];
        rhat_counters(m, n, cnt);
        n_r[r] = (double)m;
        return hipMemcpy(buf[r] + L.counters(), cnt, sizeof(cnt), hipMemcpyHostToDevice);
    }
    template <class T>
    bool host_sum(size_t off, size_t n)
    {
        std::vector<T> part(n), total(n, T(0));
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        for (double* b : buf) {
            if (hipMemcpy(part.data(), b + off, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return false;
            for (size_t j = 0; j < n; ++j) total[j] = total[j] + part[j];
        }
        for (double* b : buf)
            if (hipMemcpy(b + off, total.data(), n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return false;
        return true;
    }
    bool reduce(size_t off, size_t n, bool is_u64) { return is_u64 ? host_sum<unsigned long long>(off, n) : host_sum<double>(off, n); }
    // the merge; then rank 0's buffer — M, the counters and the mean are the same on every rank — to the host
    hipError_t merge(std::vector<double>& host)
    {
        if (!merge_ranks(st, L, (int)buf.size(), buf.data(), n_r.data(), [&](size_t off, size_t n, bool is_u64) { return reduce(off, n, is_u64); }))
            return hipErrorUnknown;
        host.resize(L.size());
        const hipError_t e = hipStreamSynchronize(st);
        return e != hipSuccess ? e : hipMemcpy(host.data(), buf[0], L.size() * sizeof(double), hipMemcpyDeviceToHost);
    }
};

// The across-chain reductions on a caller's per-chain sums, through the launch functions of the job path: (a) pool_summaries_async and pool_moments_async
// over all the chains; (b) the chains cut into nranks shards, pool_moments_async on every shard's slice staged as klara_gather_moments stages it, and
// that call's between-rank merge over the simulated ranks (SimRanks).
extern "C" klara_status klara_selftest_pooled(int32_t device, int64_t nchains, int32_t ndims, int64_t nsaved, const double* sum, const double* sumsq,
                                              const double* X, const int64_t* held, const uint64_t* naccept, int32_t nranks, const int64_t* bounds,
                                              int32_t with_sums, double* pooled_sum, double* pooled_sumsq, uint64_t* accept_total, double* mean, double* m2,
                                              double* ranks_mean, double* ranks_m2, uint64_t* ranks_counters)
{
    if (!sum || !sumsq || !X || !held || !naccept || !bounds || nchains <= 0 || ndims < 1 || ndims > 1024 || nsaved < 0 || nranks < 1) return KLARA_ERR_INVALID_ARG;
    if (bounds[0] != 0 || bounds[nranks] != nchains) return KLARA_ERR_INVALID_ARG;
    for (int r = 0; r < nranks; ++r) if (bounds[r + 1] <= bounds[r]) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const size_t D = (size_t)ndims, nd = (size_t)nchains * D;
    const long long N = nchains;
    const hipStream_t st = 0;
    DeviceArrays mem;
    SimRanks sim{ MergeLayout{ D, D }, st };
    double *dsum = nullptr, *dsumsq = nullptr, *dX = nullptr, *partial = nullptr, *out = nullptr;
    long long* dheld = nullptr; unsigned long long* dacc = nullptr;
    hipError_t e = mem.alloc(&dsum, nd);
    if (e == hipSuccess) e = mem.alloc(&dsumsq, nd);
    if (e == hipSuccess) e = mem.alloc(&dX, nd);
    if (e == hipSuccess) e = mem.alloc(&dheld, (size_t)N);
    if (e == hipSuccess) e = mem.alloc(&dacc, (size_t)N);
    if (e == hipSuccess) e = mem.alloc(&partial, (size_t)1024 * (2 * D + 1));            // (as klara_create sizes pool_partial)
    if (e == hipSuccess) e = mem.alloc(&out, 2 * (2 * D + 1));
    if (e == hipSuccess) e = sim.alloc(mem, nranks);
    if (e == hipSuccess) e = hipMemcpy(dsum, sum, nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dsumsq, sumsq, nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dX, X, nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dheld, held, (size_t)N * sizeof(long long), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dacc, naccept, (size_t)N * sizeof(unsigned long long), hipMemcpyHostToDevice);
    // the sum slots start as the caller's pooled_sum / pooled_sumsq (zeros without them): with_sums = 0 has to hand them back as they were
    if (e == hipSuccess) e = hipMemset(out, 0, 2 * (2 * D + 1) * sizeof(double));
    if (e == hipSuccess && pooled_sum) e = hipMemcpy(out, pooled_sum, D * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && pooled_sumsq) e = hipMemcpy(out + D, pooled_sumsq, D * sizeof(double), hipMemcpyHostToDevice);
    double* outm = out + 2 * D + 1;
    // (a)
    if (e == hipSuccess) e = pool_summaries_async(st, with_sums ? dsum : nullptr, dsumsq, dX, dheld, dacc, N, ndims, partial, out);
    if (e == hipSuccess) e = pool_moments_async(st, dsum, dsumsq, dX, dheld, dacc, N, ndims, (long long)nsaved, partial, outm);
    // (b) every rank's mean_r | M2_r | accept total (counter slot 0) and its other counters, then the merge
    for (int r = 0; r < nranks && e == hipSuccess; ++r) {
        const long long c0 = bounds[r], Nr = bounds[r + 1] - bounds[r];
        e = pool_moments_async(st, dsum + c0 * D, dsumsq + c0 * D, dX + c0 * D, dheld + c0, dacc + c0, Nr, ndims, (long long)nsaved, partial, sim.buf[r]);
        if (e == hipSuccess) e = sim.set_counters(r, (unsigned long long)nsaved * (unsigned long long)Nr, (unsigned long long)Nr, true);
    }
    std::vector<double> hout(2 * (2 * D + 1)), hr;
    if (e == hipSuccess) e = sim.merge(hr);
    if (e == hipSuccess) e = hipMemcpy(hout.data(), out, hout.size() * sizeof(double), hipMemcpyDeviceToHost);
    const bool clean = mem.release();
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    if (pooled_sum) memcpy(pooled_sum, hout.data(), D * sizeof(double));
    if (pooled_sumsq) memcpy(pooled_sumsq, hout.data() + D, D * sizeof(double));
    if (accept_total) memcpy(accept_total, hout.data() + 2 * D, sizeof(uint64_t));
    if (mean) memcpy(mean, hout.data() + 2 * D + 1, D * sizeof(double));
    if (m2) memcpy(m2, hout.data() + 3 * D + 1, D * sizeof(double));
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    memcpy(cnt, hr.data() + sim.L.counters(), sizeof(cnt));
    if (ranks_mean) memcpy(ranks_mean, hr.data() + sim.L.mean(), D * sizeof(double));
    if (ranks_m2) memcpy(ranks_m2, hr.data() + sim.L.M(), D * sizeof(double));
    if (ranks_counters) { ranks_counters[0] = cnt[MergeLayout::ACCEPTED]; ranks_counters[1] = cnt[MergeLayout::SAMPLES]; ranks_counters[2] = cnt[MergeLayout::CHAINS]; }
    return KLARA_OK;
}

extern "C" klara_status klara_check_custom_target(const char* src, int32_t sampler, int32_t ndims)
{
    if (!src || !sampler_valid(sampler) || ndims <= 0) return KLARA_ERR_INVALID_ARG;
    // the plain fused instantiation of the layout klara_create plans for a job of this target (one chain; zeros: VanillaMCTuner per chain, no monitor)
    klara_desc d;
    memset(&d, 0, sizeof(d));
    d.sampler = sampler; d.target = KLARA_TARGET_CUSTOM; d.ndims = ndims; d.nchains = 1; d.custom_src = src;
    KlaraPlan plan;
    const klara_status st = klara_plan_job(d, klara_read_overrides(), &plan);
    if (st != KLARA_OK) return st;
    const int modes[1] = { 0 };
    if (plan.jit_pair) return klara_jit_create_pair(src, sampler, ndims, plan.E / 2, plan.G, false, false, false, modes, 1, false, nullptr);
    const std::string whole = plan.rewrite == KLARA_REWRITE_PAIR_AS_WHOLE ? pair_as_whole_source(src) : std::string(src);
    return klara_jit_create(whole.c_str(), sampler, ndims, plan.E, plan.G, modes, 1, false, nullptr);
}

// ... and the SMMALA kernels with the softabs transform of the metric (klara_desc.smmala_softabs > 0): the variant klara_create compiles for such a job
extern "C" klara_status klara_check_custom_target_softabs(const char* src, int32_t ndims)
{
    if (!src || ndims <= 0) return KLARA_ERR_INVALID_ARG;
    klara_desc d;
    memset(&d, 0, sizeof(d));
    d.sampler = KLARA_SAMPLER_SMMALA; d.target = KLARA_TARGET_CUSTOM; d.ndims = ndims; d.nchains = 1; d.custom_src = src; d.smmala_softabs = 1.0;
    KlaraPlan plan;
    const klara_status st = klara_plan_job(d, klara_read_overrides(), &plan);
    if (st != KLARA_OK) return st;
    const int modes[1] = { 0 };
    return klara_jit_create(src, KLARA_SAMPLER_SMMALA, ndims, plan.E, plan.G, modes, 1, false, nullptr, true);
}

extern "C" const char* klara_compile_log(void) { return klara_jit_log(); }

// The pooled covariance kernels on a caller's value history: klara_cov_launch_update launch by launch with col0 running through the history, as klara_run
// issues them (the pivot copied before the first, an empty launch skipped), then klara_cov_launch_finalize; (b) the same on every shard's own history and
// klara_gather_covariance's between-rank merge over the simulated ranks (SimRanks).
static hipError_t selftest_cov_one(DeviceArrays& mem, const double* hist, long long N, long long c0, long long Nr, int D, long long ncols, int nsplits,
                                   const int64_t* splits, double* out, hipStream_t st)
{
    KCovGeom g;
    if (!klara_cov_plan(Nr, D, &g)) return hipErrorInvalidValue;
    const size_t nd = (size_t)Nr * D;
    double *dh = nullptr, *S = nullptr, *T = nullptr, *pivot = nullptr;
    hipError_t e = mem.alloc(&dh, (size_t)ncols * nd);
    if (e == hipSuccess) e = mem.alloc(&S, klara_cov_S_elems(g));
    if (e == hipSuccess) e = mem.alloc(&T, klara_cov_T_elems(g));
    if (e == hipSuccess) e = mem.alloc(&pivot, (size_t)D);
    // the shard's chains as a history of their own: column t at dh + t Nr D
    if (e == hipSuccess) e = hipMemcpy2D(dh, nd * sizeof(double), hist + (size_t)c0 * D, (size_t)N * D * sizeof(double), nd * sizeof(double), (size_t)ncols,
                                         hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(S, 0, klara_cov_S_elems(g) * sizeof(double));     // (what klara_set_state / klara_reset leave)
    if (e == hipSuccess) e = hipMemset(T, 0, klara_cov_T_elems(g) * sizeof(double));
    long long col0 = 0;
    for (int j = 0; j < nsplits && e == hipSuccess; ++j) {
        if (splits[j] > 0) {
            if (col0 == 0) e = hipMemcpyAsync(pivot, dh, (size_t)D * sizeof(double), hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = klara_cov_launch_update(g, dh, col0, (long long)splits[j], pivot, S, T, st);
        }
        col0 += splits[j];
    }
    if (e == hipSuccess) e = klara_cov_launch_finalize(g, S, T, pivot, (double)((unsigned long long)ncols * (unsigned long long)Nr), out, st);
    return e;
}

extern "C" klara_status klara_selftest_covariance(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                                  const int64_t* splits, int32_t nranks, const int64_t* bounds, double* mean, double* m2, double* ranks_mean,
                                                  double* ranks_m2, uint64_t* ranks_counters)
{
    if (!hist || !splits || !bounds || nchains <= 0 || ndims < 1 || ndims > KLARA_COV_MAX_DIMS || ncols < 1 || nsplits <= 0 || nranks < 1) return KLARA_ERR_INVALID_ARG;
    long long sum = 0;
    for (int j = 0; j < nsplits; ++j) {
        if (splits[j] < 0 || splits[j] > KLARA_COV_MAX_COLS) return KLARA_ERR_INVALID_ARG;
        sum += splits[j];
    }
    if (sum != ncols) return KLARA_ERR_INVALID_ARG;
    if (bounds[0] != 0 || bounds[nranks] != nchains) return KLARA_ERR_INVALID_ARG;
    for (int r = 0; r < nranks; ++r) if (bounds[r + 1] <= bounds[r]) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const size_t D = (size_t)ndims, DD = D * D;
    const hipStream_t st = 0;
    DeviceArrays mem;
    SimRanks sim{ MergeLayout{ D, DD }, st };
    double* out = nullptr;
    hipError_t e = mem.alloc(&out, D + DD);
    if (e == hipSuccess) e = sim.alloc(mem, nranks);
    // (a)
    if (e == hipSuccess) e = selftest_cov_one(mem, hist, nchains, 0, nchains, ndims, ncols, nsplits, splits, out, st);
    // (b) every rank's mean_r | M_r and its counters, then the merge
    for (int r = 0; r < nranks && e == hipSuccess; ++r) {
        const long long Nr = bounds[r + 1] - bounds[r];
        e = selftest_cov_one(mem, hist, nchains, bounds[r], Nr, ndims, ncols, nsplits, splits, sim.buf[r], st);
        if (e == hipSuccess) e = sim.set_counters(r, (unsigned long long)ncols * (unsigned long long)Nr, (unsigned long long)Nr, false);
    }
    std::vector<double> hout(D + DD), hr;
    if (e == hipSuccess) e = sim.merge(hr);
    if (e == hipSuccess) e = hipMemcpy(hout.data(), out, hout.size() * sizeof(double), hipMemcpyDeviceToHost);
    const bool clean = mem.release();
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    if (mean) memcpy(mean, hout.data(), D * sizeof(double));
    if (m2) memcpy(m2, hout.data() + D, DD * sizeof(double));
    unsigned long long cnt[MergeLayout::NCOUNTERS];
    memcpy(cnt, hr.data() + sim.L.counters(), sizeof(cnt));
    if (ranks_mean) memcpy(ranks_mean, hr.data() + sim.L.mean(), D * sizeof(double));
    if (ranks_m2) memcpy(ranks_m2, hr.data() + sim.L.M(), DD * sizeof(double));
    if (ranks_counters) { ranks_counters[0] = cnt[MergeLayout::SAMPLES]; ranks_counters[1] = cnt[MergeLayout::CHAINS]; }
    return KLARA_OK;
}

// The marginal histogram kernel (klara_marg.h) on a caller's value history: klara_marg_launch_update launch by launch with col0 running through the history,
// as klara_run issues them (an empty launch skipped), then the table as klara_gather_histogram reads it.  Every argument check comes before any HIP call.
extern "C" klara_status klara_selftest_marginals(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t nsplits,
                                                 const int64_t* splits, int64_t nbins, const double* lo, const double* hi, uint64_t* counts)
{
    if (!hist || !splits || !lo || !hi || !counts || nchains <= 0 || ndims < 1 || ndims > 1024 || ncols < 1 || nsplits <= 0 || nbins < 1 ||
        nbins > KLARA_MARG_MAX_BINS)
        return KLARA_ERR_INVALID_ARG;
    long long sum = 0;
    for (int j = 0; j < nsplits; ++j) {
        if (splits[j] < 0 || splits[j] > KLARA_MARG_MAX_COLS) return KLARA_ERR_INVALID_ARG;
        sum += splits[j];
    }
    if (sum != ncols) return KLARA_ERR_INVALID_ARG;
    for (int i = 0; i < ndims; ++i) if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || !(lo[i] < hi[i])) return KLARA_ERR_INVALID_ARG;
    KMargGeom g;
    if (!klara_marg_plan(nchains, ndims, nbins, &g)) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const size_t D = (size_t)ndims, nd = (size_t)nchains * D, K = klara_marg_count_elems(g);
    const hipStream_t st = 0;
    std::vector<double> par(lo, lo + D);
    par.insert(par.end(), hi, hi + D);
    for (size_t i = 0; i < D; ++i) par.push_back(klara_marg_inv_w(nbins, lo[i], hi[i]));
    DeviceArrays mem;
    double *dh = nullptr, *dpar = nullptr; unsigned long long* dc = nullptr;
    hipError_t e = mem.alloc(&dh, (size_t)ncols * nd);
    if (e == hipSuccess) e = mem.alloc(&dpar, par.size());
    if (e == hipSuccess) e = mem.alloc(&dc, K);
    if (e == hipSuccess) e = hipMemcpy(dh, hist, (size_t)ncols * nd * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dpar, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dc, 0, K * sizeof(unsigned long long));       // (what klara_set_state / klara_reset leave)
    long long col0 = 0;
    for (int j = 0; j < nsplits && e == hipSuccess; ++j) {
        if (splits[j] > 0) e = klara_marg_launch_update(g, dh, col0, (long long)splits[j], dpar, dc, st);
        col0 += splits[j];
    }
    std::vector<uint64_t> hc(K);
    if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), dc, K * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    const bool clean = mem.release();
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    memcpy(counts, hc.data(), K * sizeof(uint64_t));
    return KLARA_OK;
}

// The R-hat kernels (klara_rhat.h) on a caller's per-chain sums (unsplit) and / or a caller's value history (split), through the launch functions of the job
// path: the chains [c0, c0 + Nr) staged into buf as klara_gather_rhat stages them (zeros | mean_r, Bsum_r, Wsum_r | the counters are the caller's)
static hipError_t selftest_rhat_one(DeviceArrays& mem, const MergeLayout& L, bool split, const double* dsum, const double* dsumsq, const double* dX,
                                    const long long* dheld, long long nsaved, const double* hist, long long ncols, long long N, long long c0, long long Nr,
                                    int D, double* partial, double* buf, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(buf, 0, L.size() * sizeof(double), st);
    if (e != hipSuccess) return e;
    if (!split) return rhat_sums_async(st, dsum + c0 * D, dsumsq + c0 * D, dX + c0 * D, dheld + c0, Nr, D, nsaved, partial, buf + L.mean_r(), buf + L.extra());
    // the shard's chains as a history of their own: column t at dh + t Nr D
    const size_t nd = (size_t)Nr * D;
    double *dh = nullptr, *half = nullptr;
    e = mem.alloc(&dh, (size_t)ncols * nd);
    if (e == hipSuccess) e = mem.alloc(&half, 4 * nd);
    if (e == hipSuccess) e = hipMemcpy2D(dh, nd * sizeof(double), hist + (size_t)c0 * D, (size_t)N * D * sizeof(double), nd * sizeof(double), (size_t)ncols,
                                         hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rhat_split_async(st, dh, ncols, Nr, D, half, partial, buf + L.mean_r(), buf + L.extra());
    return e;
}

extern "C" klara_status klara_selftest_rhat(int32_t device, int64_t nchains, int32_t ndims, int64_t nsaved, const double* sum, const double* sumsq,
                                            const double* X, const int64_t* held, int64_t ncols, const double* hist, int32_t nranks, const int64_t* bounds,
                                            double* out, double* ranks_out, double* split_out, double* split_ranks_out, uint64_t* counters)
{
    const bool sums = sum || sumsq || X || held;
    if (!bounds || nchains <= 0 || ndims < 1 || ndims > 1024 || nranks < 1 || (!sums && !hist)) return KLARA_ERR_INVALID_ARG;
    if (sums && (!sum || !sumsq || !X || !held || nsaved < 1)) return KLARA_ERR_INVALID_ARG;
    if (hist && ncols < 2) return KLARA_ERR_INVALID_ARG;
    if (bounds[0] != 0 || bounds[nranks] != nchains) return KLARA_ERR_INVALID_ARG;
    for (int r = 0; r < nranks; ++r) if (bounds[r + 1] <= bounds[r]) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const size_t D = (size_t)ndims, nd = (size_t)nchains * D;
    const long long N = nchains;
    const hipStream_t st = 0;
    const MergeLayout L{ D, D, D };
    DeviceArrays mem;
    double *dsum = nullptr, *dsumsq = nullptr, *dX = nullptr, *partial = nullptr, *one = nullptr;
    long long* dheld = nullptr;
    hipError_t e = mem.alloc(&partial, klara_rhat_partial_elems(ndims));
    if (e == hipSuccess) e = mem.alloc(&one, L.size());
    if (sums) {
        if (e == hipSuccess) e = mem.alloc(&dsum, nd);
        if (e == hipSuccess) e = mem.alloc(&dsumsq, nd);
        if (e == hipSuccess) e = mem.alloc(&dX, nd);
        if (e == hipSuccess) e = mem.alloc(&dheld, (size_t)N);
        if (e == hipSuccess) e = hipMemcpy(dsum, sum, nd * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dsumsq, sumsq, nd * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dX, X, nd * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dheld, held, (size_t)N * sizeof(long long), hipMemcpyHostToDevice);
    }
    klara_status status = KLARA_OK;
    for (int split = 0; split < 2 && e == hipSuccess && status == KLARA_OK; ++split) {
        if (split ? !hist : !sums) continue;
        const unsigned long long n = (unsigned long long)(split ? ncols / 2 : nsaved), per = split ? 2 : 1;     // samples per unit; units per chain
        double* dst[2] = { split ? split_out : out, split ? split_ranks_out : ranks_out };
        uint64_t* cdst = counters ? counters + 4 * split : nullptr;
        std::vector<double> host(L.size());
        // (a) all the chains: one staging buffer, no merge
        unsigned long long cnt[MergeLayout::NCOUNTERS];
        rhat_counters(per * (unsigned long long)N, n, cnt);
        e = selftest_rhat_one(mem, L, split != 0, dsum, dsumsq, dX, dheld, (long long)nsaved, hist, (long long)ncols, N, 0, N, ndims, partial, one, st);
        if (e == hipSuccess) e = hipMemcpy(one + L.counters(), cnt, sizeof(cnt), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(host.data(), one, L.size() * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        uint64_t units = 0; int64_t nper = 0;
        double* o = dst[0];
        status = rhat_finish(D, host.data(), false, o, o ? o + D : nullptr, o ? o + 2 * D : nullptr, o ? o + 3 * D : nullptr, &units, &nper);
        if (cdst) { cdst[0] = units; cdst[1] = (uint64_t)nper; }
        if (status != KLARA_OK) break;
        // (b) every rank's mean_r | Bsum_r | Wsum_r and its counters, then the merge
        SimRanks sim{ L, st };
        e = sim.alloc(mem, nranks);
        for (int r = 0; r < nranks && e == hipSuccess; ++r) {
            const long long Nr = bounds[r + 1] - bounds[r];
            e = selftest_rhat_one(mem, L, split != 0, dsum, dsumsq, dX, dheld, (long long)nsaved, hist, (long long)ncols, N, bounds[r], Nr, ndims, partial,
                                  sim.buf[r], st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e == hipSuccess) e = sim.set_rhat_counters(r, per * (unsigned long long)Nr, n);
        }
        std::vector<double> hr;
        if (e == hipSuccess) e = sim.merge(hr);
        if (e != hipSuccess) break;
        o = dst[1];
        status = rhat_finish(D, hr.data(), true, o, o ? o + D : nullptr, o ? o + 2 * D : nullptr, o ? o + 3 * D : nullptr, &units, &nper);
        if (cdst) { cdst[2] = units; cdst[3] = (uint64_t)nper; }
    }
    const bool clean = mem.release();
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    return status;
}

// The pooled effective sample size on a caller's value history, through the launch functions and the ess_finish of klara_gather_ess.  One shard's chains
// [c0, c0 + Nr) through one path into a staging buffer: path 0 the streamed state fed launch by launch over `splits` (as klara_run feeds the job's), path 1
// the history mode's feed of the stored columns, path 2 the split form's two halves; then the across-chain reduction.  false in *clean: a canary was damaged.
static hipError_t selftest_ess_one(const MergeLayout& L, int path, const double* hist, long long ncols, long long N, long long c0, long long Nr, int D, int W,
                                   int nsplits, const int64_t* splits, double* buf, hipStream_t st, bool* clean)
{
    const int per = path == 2 ? 2 : 1;
    const long long nd = Nr * D, n = per == 2 ? ncols / 2 : ncols;
    DeviceArrays loc;
    double *dh = nullptr, *ws = nullptr;
    EssState s[2];
    hipError_t e = hipMemsetAsync(buf, 0, L.size() * sizeof(double), st);
    if (e == hipSuccess) e = loc.alloc(&dh, (size_t)ncols * (size_t)nd);
    if (e == hipSuccess) e = ess_alloc_states(loc, per, W, nd, s);
    if (e == hipSuccess) e = loc.alloc(&ws, klara_ess_ws_elems((long long)per * nd, D, W));
    // the shard's chains as a history of their own: column t at dh + t Nr D
    if (e == hipSuccess) e = hipMemcpy2D(dh, (size_t)nd * sizeof(double), hist + (size_t)c0 * D, (size_t)N * D * sizeof(double), (size_t)nd * sizeof(double),
                                         (size_t)ncols, hipMemcpyHostToDevice);
    if (e == hipSuccess && path == 0) {
        const size_t wb = (size_t)W * (size_t)nd * sizeof(double);
        e = hipMemsetAsync(s[0].S, 0, wb, st);                               // (what klara_set_state / klara_reset leave)
        if (e == hipSuccess) e = hipMemsetAsync(s[0].head, 0, wb, st);
        if (e == hipSuccess) e = hipMemsetAsync(s[0].tail, 0, wb, st);
        if (e == hipSuccess) e = hipMemsetAsync(s[0].total, 0, (size_t)nd * sizeof(double), st);
        long long col0 = 0;
        for (int j = 0; j < nsplits && e == hipSuccess; ++j) {
            if (splits[j] > 0) e = launch_acov_update(st, dh, s[0].S, s[0].head, s[0].tail, s[0].near, s[0].total, col0, W, nd, col0, (long long)splits[j]);
            col0 += splits[j];
        }
    } else if (e == hipSuccess) e = ess_feed_history_async(st, dh, ncols, nd, W, per, s);
    if (e == hipSuccess) e = ess_reduce_async(st, s, per, n, W, nd, D, ws, buf + L.mean_r(), buf + L.extra());
    const hipError_t es = hipStreamSynchronize(st);
    if (!loc.release()) *clean = false;
    return e != hipSuccess ? e : es;
}

extern "C" klara_status klara_selftest_ess(int32_t device, int64_t nchains, int32_t ndims, int64_t ncols, const double* hist, int32_t maxlag, int32_t nsplits,
                                           const int64_t* splits, int32_t nranks, const int64_t* bounds, double* out, double* rho, double* csum,
                                           int32_t* pairs, uint64_t* counters)
{
    if (!hist || !splits || !bounds || nchains <= 0 || ndims < 1 || ndims > 1024 || ncols < 2 || maxlag < 1 || maxlag > KLARA_ESS_MAXLAG || nsplits <= 0 ||
        nranks < 1)
        return KLARA_ERR_INVALID_ARG;
    long long sum = 0;
    for (int j = 0; j < nsplits; ++j) {
        if (splits[j] < 0 || splits[j] > 0x7fffffffll) return KLARA_ERR_INVALID_ARG;
        sum += splits[j];
    }
    if (sum != ncols) return KLARA_ERR_INVALID_ARG;
    if (bounds[0] != 0 || bounds[nranks] != nchains) return KLARA_ERR_INVALID_ARG;
    for (int r = 0; r < nranks; ++r) if (bounds[r + 1] <= bounds[r]) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    const size_t D = (size_t)ndims, R = (size_t)maxlag + 1;
    const long long N = nchains;
    const int W = maxlag + 1;
    const hipStream_t st = 0;
    klara_status status = KLARA_OK;
    hipError_t e = hipSuccess;
    bool clean = true;
    for (int path = 0; path < 3 && e == hipSuccess && status == KLARA_OK; ++path) {
        if (path == 2 && ncols < 8) continue;                               // (the split form needs 4 samples per half)
        const unsigned long long per = path == 2 ? 2 : 1, n = (unsigned long long)(path == 2 ? ncols / 2 : ncols);
        const int Lg = (int)((long long)maxlag < (long long)n - 1 ? (long long)maxlag : (long long)n - 1);
        const MergeLayout L{ D, D, D + D * ((size_t)Lg + 1) };
        for (int ranks = 0; ranks < 2 && e == hipSuccess && status == KLARA_OK; ++ranks) {
            const int slot = 2 * path + ranks, nr = ranks ? nranks : 1;
            DeviceArrays mem;
            SimRanks sim{ L, st };
            e = sim.alloc(mem, nr);
            for (int r = 0; r < nr && e == hipSuccess; ++r) {
                const long long c0 = ranks ? bounds[r] : 0, Nr = ranks ? bounds[r + 1] - bounds[r] : N;
                e = selftest_ess_one(L, path, hist, (long long)ncols, N, c0, Nr, ndims, W, nsplits, splits, sim.buf[r], st, &clean);
                if (e == hipSuccess) e = sim.set_rhat_counters(r, per * (unsigned long long)Nr, n);
            }
            std::vector<double> host(L.size());
            if (e == hipSuccess && ranks) e = sim.merge(host);              // (b) the between-rank merge; (a) one staging buffer, no merge
            else if (e == hipSuccess) e = hipMemcpy(host.data(), sim.buf[0], L.size() * sizeof(double), hipMemcpyDeviceToHost);
            if (!mem.release()) clean = false;
            if (e != hipSuccess) break;
            uint64_t units = 0; int64_t nper = 0;
            double* o = out ? out + (size_t)slot * 5 * D : nullptr;
            status = ess_finish(D, Lg, host.data(), ranks != 0, o, o ? o + D : nullptr, rho ? rho + (size_t)slot * D * R : nullptr, o ? o + 2 * D : nullptr,
                                o ? o + 3 * D : nullptr, o ? o + 4 * D : nullptr, pairs ? pairs + (size_t)slot * D : nullptr, &units, &nper,
                                csum ? csum + (size_t)slot * D * R : nullptr);
            if (counters) { counters[3 * slot] = units; counters[3 * slot + 1] = (uint64_t)nper; counters[3 * slot + 2] = (uint64_t)Lg; }
        }
    }
    if (e != hipSuccess || !clean) return KLARA_ERR_HIP;
    return status;
}
