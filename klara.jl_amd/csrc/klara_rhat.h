// klara_rhat.h — internal: the Gelman–Rubin diagnostic over all chains (klara_gather_rhat).  Per dimension, over m units (chains,
// or half-chains for the split form) of n samples each with mean mu_u and M2_u = sum_t (x_ut - mu_u)^2:
//   Wsum = sum_u M2_u,  mean = (1 / m) sum_u mu_u,  Bsum = sum_u (mu_u - mean)^2,
//   R-hat = sqrt(((n - 1) / n W + B / n) / W)  with  W = Wsum / (m (n - 1)),  B / n = Bsum / (m - 1)
// — the within / between decomposition of what the pooled moments add together (M2 = Wsum + n Bsum).
#pragma once
#include <hip/hip_runtime.h>

// ---- device: what the pooled moments (klara_monitors.hip) and R-hat (klara_rhat.hip) share, written once
// Chan's update of (n, mean, m2) with (nb, meanb, m2b): sums of non-negative terms only
__device__ inline void chan_merge(double& n, double& mean, double& m2, double nb, double meanb, double m2b)
{
    const double nt = n + nb;
    if (!(nt > 0.0)) return;
    const double delta = meanb - mean, w = nb / nt;
    mean = mean + delta * w;
    m2 = (m2 + m2b) + (delta * delta) * (n * w);
    n = nt;
}
// (mean, M2) of n values from their sum s and sum of squares q: the one cancelling subtraction, q - s^2 / n, carried in double-double (s^2 = p + pe
// exactly by fma, the quotient's remainder by fma), clamped at 0
__device__ inline void moments_of_sums(double s, double q, double n, double& mean, double& m2)
{
    const double p = s * s, pe = fma(s, s, -p);                    // s^2 = p + pe
    const double qh = p / n, r = fma(-qh, n, p);                   // p = qh * n + r
    const double ql = (r + pe) / n;                                // s^2 / n = qh + ql (+ O(2^-105))
    double m2c = (q - qh) - ql;
    if (m2c < 0.0) m2c = 0.0;
    mean = s / n; m2 = m2c;
}
// a chain's sums over its saved steps (sojourn form: part + held * x), then the above — as k_moments_stage1 reads a chain
__device__ inline void chain_moments(const double* __restrict__ sum, const double* __restrict__ sumsq, const double* __restrict__ X,
                                     const long long* __restrict__ held, long long c, int D, int j, double nsaved, double& mean, double& m2)
{
    const long long hd = held[c];
    const double x = X[c * D + j];
    const double s = hd > 0 ? sum[c * D + j] + (double)hd * x : sum[c * D + j];
    const double q = hd > 0 ? sumsq[c * D + j] + (double)hd * (x * x) : sumsq[c * D + j];
    moments_of_sums(s, q, nsaved, mean, m2);
}

// ---- host: the launch functions the job path (klara_gather_rhat) and klara_selftest_rhat both run
#pragma GCC visibility push(hidden)
#define KLARA_RHAT_POOL_BLOCKS 1024                                // = KLARA_POOL_BLOCKS: stage 1's blocks
// doubles of staging for D dimensions: stage 1's (mean, Bsum, Wsum) per block, then the D pivots
static inline size_t klara_rhat_partial_elems(int D) { return (size_t)KLARA_RHAT_POOL_BLOCKS * 3 * (size_t)D + (size_t)D; }
// Unsplit, from the chains' running sums (N x D, held N): out = mean[D] | Bsum[D] and wout = Wsum[D] over the N chains of nsaved samples
// each (two outputs: a gather call stages them at MergeLayout's mean_r | M and extra)
hipError_t rhat_sums_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held, long long N, int D,
                           long long nsaved, double* partial, double* out, double* wout);
// Split, from a stored history (column t at hist + t N D, ncols >= 2 columns): every chain's two halves [0, h) and [ncols - h, ncols), h = ncols / 2,
// become (mean, M2) in half[0, 2 N D) | half[2 N D, 4 N D), unit 2 c + half; then the same reduction over the 2 N units: out, wout as above
hipError_t rhat_split_async(hipStream_t stream, const double* hist, long long ncols, long long N, int D, double* half, double* partial, double* out,
                            double* wout);
// The reduction alone, over M units whose (mean, M2) are given (mu, m2: M x D, unit-major — the layout of `half` above): what the pooled effective
// sample size (klara_ess.hip) hands its units to, so that its mean, Bsum and Wsum come out of R-hat's own code
hipError_t rhat_units_async(hipStream_t stream, const double* mu, const double* m2, long long M, int D, double* partial, double* out, double* wout);
// R-hat of one dimension from (Wsum, Bsum) over m units of n samples: NaN for m < 2 or n < 2, plain IEEE division otherwise
double rhat_value(double wsum, double bsum, double m, double n);
#ifdef KLARA_HIP_H
// ---- klara_comm.hip: the ends of a klara_gather_rhat / klara_selftest_rhat call around the between-rank merge (klara_merge.h; layout MergeLayout{ D, D, D })
// this rank's counters for m units of n samples each, in MergeLayout's R-hat slots
void rhat_counters(unsigned long long m, unsigned long long n, unsigned long long cnt[4]);
// From a staging buffer on the host (merged: after merge_ranks, else one rank's own): KLARA_ERR_STATE unless every rank held the same number of samples
// per unit; else the outputs (any may be null) — before the first sample NaN for rhat and zeros
klara_status rhat_finish(size_t D, const double* host, bool merged, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* units, int64_t* nper);
#endif
#pragma GCC visibility pop
