// klara_marg_host.h — the host-only parts of the pooled marginal histograms: the quantile rule (klara_histogram_quantiles, include/klara_hip.h; returns 0, or 1
// for an invalid argument) and the words by which klara_gather_histogram finds ranks whose bins differ.  Plain C++ with no HIP in it, so that a stand-alone
// program can be built from it with a host compiler and its sanitizers (tests/test_marg_host.py).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef KLARA_MARG_MAX_BINS
#define KLARA_MARG_MAX_BINS 1024
#endif

// Per dimension, n = the row's total, w = (hi - lo) / nbins: k = max(1, ceil(p n)); b = the first slot whose cumulative count reaches k; slot 0: -inf, slot
// nbins + 1: +inf, otherwise (lo + (b - 1) w) + w (k - cum_before) / count_b — every operation a single IEEE one in that order (the library is built with
// -ffp-contract=off; klara_jl_amd.stats.hist_quantiles restates it operation for operation).  ceil(p n) is taken in double: exact while n < 2^53.
static inline int klara_marg_quantiles(const uint64_t* counts, int32_t ndims, int64_t nbins, const double* lo, const double* hi, int32_t nprobs,
                                       const double* probs, double* out)
{
    if (!counts || !lo || !hi || !probs || !out || ndims < 1 || nbins < 1 || nbins > KLARA_MARG_MAX_BINS || nprobs < 1) return 1;
    for (int32_t j = 0; j < nprobs; ++j) if (!(probs[j] > 0.0 && probs[j] <= 1.0)) return 1;
    const int64_t S = nbins + 2;
    for (int32_t d = 0; d < ndims; ++d) {
        const uint64_t* c = counts + (int64_t)d * S;
        uint64_t n = 0;
        for (int64_t s = 0; s < S; ++s) n += c[s];
        const double w = (hi[d] - lo[d]) / (double)nbins;
        for (int32_t j = 0; j < nprobs; ++j) {
            double* o = out + (int64_t)d * nprobs + j;
            if (n == 0) { *o = (double)NAN; continue; }
            const double kd = ceil(probs[j] * (double)n);
            uint64_t k = kd < 1.0 ? 1 : (uint64_t)kd;
            if (k > n) k = n;                                   // (p <= 1 and the product is rounded once: only the rounding can pass n)
            uint64_t cum = 0;
            int64_t b = 0;
            while (cum + c[b] < k) { cum += c[b]; ++b; }        // ends at b <= nbins + 1: the total is n >= k
            if (b == 0) *o = -(double)INFINITY;
            else if (b == nbins + 1) *o = (double)INFINITY;
            else {
                const double left = lo[d] + (double)(b - 1) * w;
                *o = left + w * (double)(k - cum) / (double)c[b];
            }
        }
    }
    return 0;
}

// What klara_gather_histogram compares between ranks: w[0 .. NV) = v = nbins and the bit patterns of lo[D] and hi[D], w[NV .. 2 NV) = ~v, NV = 2 D + 1.
// An integer maximum over the ranks leaves max(v) | max(~v) = ~min(v): every rank held the same v exactly when the two halves are still complements.
static inline void klara_marg_agreement_words(int64_t nbins, const double* lo, const double* hi, int32_t ndims, uint64_t* w)
{
    const size_t D = (size_t)ndims, NV = 2 * D + 1;
    w[0] = (uint64_t)nbins;
    memcpy(w + 1, lo, D * sizeof(double));
    memcpy(w + 1 + D, hi, D * sizeof(double));
    for (size_t i = 0; i < NV; ++i) w[NV + i] = ~w[i];
}
// reduced = the maximum over the ranks of their 2 NV words; 1: all ranks agree
static inline int klara_marg_words_agree(const uint64_t* reduced, size_t NV)
{
    for (size_t i = 0; i < NV; ++i) if (reduced[i] != ~reduced[NV + i]) return 0;
    return 1;
}
