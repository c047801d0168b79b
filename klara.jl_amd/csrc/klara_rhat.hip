// klara_rhat.hip — the Gelman–Rubin diagnostic's kernels (klara_rhat.h): every unit's (mean, M2), from the chains' running sums or from the halves of
// the stored history, then one across-unit reduction of fixed shape for both — no floating-point atomics, the same bits for a given unit count.
#include "klara_handle.h"
#include "klara_rhat.h"

// Where stage 1 takes unit u's (mean, M2) of dimension j from: a chain's running sums, formed as the pooled moments form them ...
struct RhatFromSums {
    const double *sum, *sumsq, *X; const long long* held; int D; double nsaved;
    __device__ void get(long long u, int j, double& mean, double& m2) const { chain_moments(sum, sumsq, X, held, u, D, j, nsaved, mean, m2); }
};
// ... or k_rhat_halves' output, unit 2 c + half
struct RhatFromHalves {
    const double *hm, *hq; int D;
    __device__ void get(long long u, int j, double& mean, double& m2) const { mean = hm[u * D + j]; m2 = hq[u * D + j]; }
};

// Stage 1: block b of nb = min(M, 1024) merges the units u = b, b + nb, ... in ascending order, thread j the dimension j (a unit's D values are contiguous:
// coalesced).  It carries (k units, mean of their means, Bsum) by chan_merge at unit weight and Wsum as a plain ascending sum of the non-negative M2.
// The means are merged as mu_u - pivot, pivot = unit 0's mean: the difference is exact or nearly so, and the merges then round at the scale of the
// spread of the means, not at the scale of the means — at an offset of 1e6 sd the u |mean| of every merge would cost Bsum 1e-7 otherwise.
// partial: nb x (mean | Bsum | Wsum), D each; the pivots behind all 1024 rows.
template <class Src>
__global__ __launch_bounds__(256) void k_rhat_stage1(Src src, long long M, int D, int nb, double* __restrict__ partial)
{
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < D; j += 256) {
        double pivot, unused;
        src.get(0, j, pivot, unused);
        double k = 0.0, mean = 0.0, bsum = 0.0, wsum = 0.0;
        for (long long u = b; u < M; u += nb) {
            double mu, m2;
            src.get(u, j, mu, m2);
            chan_merge(k, mean, bsum, 1.0, mu - pivot, 0.0);
            wsum += m2;
        }
        double* row = partial + (long long)b * 3 * D;
        row[j] = mean; row[D + j] = bsum; row[2 * D + j] = wsum;
        if (b == 0) partial[(long long)KLARA_RHAT_POOL_BLOCKS * 3 * D + j] = pivot;
    }
}
// Stage 2, block j: dimension j.  Thread t merges the blocks' partials b = t, t + 256, ... (ascending) with their unit counts, then a fixed tree over the
// threads.  out[j] = pivot + mean of the shifted means, out[D + j] = Bsum, wout[j] = Wsum.
__global__ __launch_bounds__(256) void k_rhat_stage2(const double* __restrict__ partial, long long M, int D, int nb, double* __restrict__ out,
                                                     double* __restrict__ wout)
{
    __shared__ double sn[256], sm[256], sb[256], sw[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double k = 0.0, mean = 0.0, bsum = 0.0, wsum = 0.0;
    for (int b = t; b < nb; b += 256) {
        const long long units = (M - b + nb - 1) / nb;                      // units u = b, b + nb, ... < M
        const double* row = partial + (long long)b * 3 * D;
        chan_merge(k, mean, bsum, (double)units, row[j], row[D + j]);
        wsum += row[2 * D + j];
    }
    sn[t] = k; sm[t] = mean; sb[t] = bsum; sw[t] = wsum;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (t < m) { chan_merge(sn[t], sm[t], sb[t], sn[t + m], sm[t + m], sb[t + m]); sw[t] += sw[t + m]; }
        __syncthreads();
    }
    if (t == 0) { out[j] = partial[(long long)KLARA_RHAT_POOL_BLOCKS * 3 * D + j] + sm[0]; out[D + j] = sb[0]; wout[j] = sw[0]; }
}

// The split form's pass over the history, the hot path: one thread per (chain, dimension) series, consecutive threads consecutive dimensions of one
// chain (coalesced, as k_chain_stats); the two halves [0, h) and [ncols - h, ncols) advance together — two independent streams of loads per thread — and
// every column is read once.  Each half is summed as z = x - (the half's first sample), for the reason written at k_chain_stats: s = sum z, q = sum z^2
// in sample order, and (mean of z, M2) from them by moments_of_sums — the shifted one-pass form with the cancelling subtraction in double-double, the
// very function the chains' running sums go through.  A half that never moves has z = 0 throughout: M2 exactly 0.
__global__ __launch_bounds__(256) void k_rhat_halves(const double* __restrict__ hist, long long ncols, long long N, int D, double* __restrict__ hm,
                                                     double* __restrict__ hq)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const long long stride = N * D, h = ncols / 2;
    const double* va = hist + i;                                            // va[t * stride]: first half
    const double* vb = va + (ncols - h) * stride;                           // second half (odd ncols: the middle sample is dropped)
    const double a0 = va[0], b0 = vb[0];
    double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
#pragma unroll 4
    for (long long t = 0; t < h; ++t) {
        const double za = va[t * stride] - a0, zb = vb[t * stride] - b0;
        sa += za; qa += za * za;
        sb += zb; qb += zb * zb;
    }
    double ma, m2a, mb, m2b;
    moments_of_sums(sa, qa, (double)h, ma, m2a);
    moments_of_sums(sb, qb, (double)h, mb, m2b);
    const long long c = i / D, j = i - c * D, u = 2 * c * D + j;             // units 2 c and 2 c + 1
    hm[u] = a0 + ma; hq[u] = m2a;
    hm[u + D] = b0 + mb; hq[u + D] = m2b;
}

template <class Src>
static hipError_t rhat_reduce_async(hipStream_t stream, const Src& src, long long M, int D, double* partial, double* out, double* wout)
{
    const int nb = (int)(M < KLARA_RHAT_POOL_BLOCKS ? M : KLARA_RHAT_POOL_BLOCKS);
    hipLaunchKernelGGL(k_rhat_stage1<Src>, dim3(nb), dim3(256), 0, stream, src, M, D, nb, partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rhat_stage2, dim3(D), dim3(256), 0, stream, partial, M, D, nb, out, wout);
    return hipGetLastError();
}
hipError_t rhat_sums_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held, long long N, int D,
                           long long nsaved, double* partial, double* out, double* wout)
{
    return rhat_reduce_async(stream, RhatFromSums{ sum, sumsq, X, held, D, (double)nsaved }, N, D, partial, out, wout);
}
hipError_t rhat_split_async(hipStream_t stream, const double* hist, long long ncols, long long N, int D, double* half, double* partial, double* out,
                            double* wout)
{
    double *hm = half, *hq = half + 2 * N * D;
    hipLaunchKernelGGL(k_rhat_halves, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, stream, hist, ncols, N, D, hm, hq);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rhat_reduce_async(stream, RhatFromHalves{ hm, hq, D }, 2 * N, D, partial, out, wout);
}

hipError_t rhat_units_async(hipStream_t stream, const double* mu, const double* m2, long long M, int D, double* partial, double* out, double* wout)
{
    return rhat_reduce_async(stream, RhatFromHalves{ mu, m2, D }, M, D, partial, out, wout);
}

double rhat_value(double wsum, double bsum, double m, double n)
{
    if (m < 2.0 || n < 2.0) return NAN;
    const double W = wsum / (m * (n - 1.0)), Bn = bsum / (m - 1.0);
    const double varplus = ((n - 1.0) / n) * W + Bn;
    return std::sqrt(varplus / W);
}
