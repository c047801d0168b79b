// klara_ess.h — internal: the pooled (multi-chain) effective sample size over all chains (klara_gather_ess).  Per dimension, over m
// units (chains, or half-chains for the split form) of n saved samples each, with unit mean mu_u and lagged sums
//   c_u(k) = sum_(t >= k) (x_ut - mu_u)(x_u,t-k - mu_u),  k = 0 .. L,  L = min(maxlag, n - 1)
// the device forms csum[k] = sum_u c_u(k), wsum = sum_u c_u(0), mean = (1 / m) sum_u mu_u, bsum = sum_u (mu_u - mean)^2; the host (ess_finish) turns
// them into rho, Geyer's truncated monotone pair sum, tau and ess = m n / tau.
//
// The order of operations (tests/ess_ref.py restates it).  Everything starts from a streamed autocovariance state (klara_monitors.hip: S, head, tail
// [W][nd] and total [nd] of z = x - pivot, pivot = head[0]); the split form has two such states, the first and the second halves, and unit 2 c + half.
// The unit-series e = u D + j, e < E = m D, is series (u D + j) of the one state, or series ((u >> 1) D + j) of state (u & 1).
//   per unit-series, k ascending from 0, with tot = total, mean = tot / n, hs = ts = 0.0 (the sums of the first / last k values of z):
//     c(k) = (S[k] - mean * ((tot - ts) + (tot - hs))) + ((double)(n - k) * mean) * mean;   hs = hs + (head[k] - pivot);  ts = ts + tail[k]
//     — k_acov_finalize's expression times n.  The unit's (mu, M2) handed to R-hat's reduction (klara_rhat.hip, unchanged) is (pivot + mean, c(0)).
//   stage 1: V = D floor(T / D) lanes, T = 256 nb threads, nb = max(min(ceil(E / 256), KLARA_ESS_BLOCKS), ceil(D / 256)).  Lane g < V adds
//     c(k) of e = g, g + V, g + 2 V, ... (ascending, from 0.0) for every lag: V is a multiple of D, so all of them are dimension g mod D.  The lags go
//     in blocks of 32 accumulators; a unit-series' (hs, ts) at the end of a block is kept in a checkpoint array for the next one: S, head and tail
//     are read once.  partial[k][g].
//   stage 2, lag k: for D <= 256 one workgroup, lane t < V2 = D floor(256 / D) adds partial[k][t], [t + V2], ... (ascending, from 0.0), then thread
//     j < D adds the lanes j, j + D, ... < V2 (ascending, from 0.0); for D > 256 thread j adds partial[k][j], [j + D], ... (ascending, from 0.0).
// No floating-point atomics: the bits depend on (m, D, L, n) and the streamed state only — which does not depend on how the steps were cut into launches.
#pragma once
#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)
#define KLARA_ESS_BLOCKS 512                                       // stage 1's workgroups at most (131,072 lanes: 2 wavefronts per SIMD of 256 CUs)
#define KLARA_ESS_FEED_COLS 256                                    // history / split mode: stored columns per launch_acov_update call
#define KLARA_ESS_MAXLAG 127

// one streamed autocovariance state ([W][nd] each, total [nd]); near: 32 nd of scratch for launch_acov_update, W > 32 only
struct EssState { double *S, *head, *tail, *total, *near; };
// stage 1's lanes for E unit-series of D dimensions
static inline long long klara_ess_lanes(long long E, int D)
{
    long long nb = (E + 255) / 256;
    if (nb > KLARA_ESS_BLOCKS) nb = KLARA_ESS_BLOCKS;
    if (nb < (D + 255) / 256) nb = (D + 255) / 256;
    return (long long)D * ((256 * nb) / D);
}
// doubles of workspace for E unit-series and W lags: the units' (mu, M2) | the checkpoints (hs, ts) | stage 1's partials | R-hat's staging
size_t klara_ess_ws_elems(long long E, int D, int W);
// per = 1: the N chains of st[0]; per = 2: the 2 N half-chains of st[0] (first halves) and st[1] (second halves).  n >= 1 samples per unit, nd = N D.
// meanb = mean[D] | bsum[D];  x = wsum[D] | csum[D][L + 1], L = min(W - 1, n - 1)  (MergeLayout's mean_r | M and extra)
hipError_t ess_reduce_async(hipStream_t stream, const EssState* st, int per, long long n, int W, long long nd, int D, double* ws, double* meanb, double* x);
// The stored history (column t at hist + t nd) through launch_acov_update into zeroed states of W lags, KLARA_ESS_FEED_COLS columns per call:
// per = 1: all ncols columns into st[0]; per = 2: [0, h) into st[0] and [ncols - h, ncols) into st[1], h = ncols / 2
hipError_t ess_feed_history_async(hipStream_t stream, const double* hist, long long ncols, long long nd, int W, int per, const EssState* st);
#ifdef KLARA_HIP_H
struct DeviceArrays;
// allocates `per` zero-initialised-on-feed states of W lags for nd series from mem
hipError_t ess_alloc_states(DeviceArrays& mem, int per, int W, long long nd, EssState* st);
// ---- klara_comm.hip: the host end of klara_gather_ess / klara_selftest_ess.  host: a MergeLayout{ D, D, D + D (L + 1) } staging buffer (merged: after
// merge_ranks).  KLARA_ERR_STATE unless every rank held the same n; else the outputs (any may be null; rho and csum D x (L + 1), row-major)
klara_status ess_finish(size_t D, int L, const double* host, bool merged, double* ess, double* tau, double* rho, double* mean, double* wsum, double* bsum,
                        int32_t* pairs, uint64_t* units, int64_t* nper, double* csum);
// the (L, ~L) words of the ranks' agreement and its verdict on their maxima (as klara_gather_histogram's)
void ess_agreement_words(int L, uint64_t v[2]);
bool ess_words_agree(const uint64_t v[2]);
#endif
#pragma GCC visibility pop
