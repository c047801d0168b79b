// klara_dense.hip — instantiates the dense-Gaussian FP64-MFMA kernels for gfx950.
#include "klara_launch.h"
#include "klara_dense.h"

// streamed layouts (NE = 40 .. 64; D = 129 .. 256; HMC, MALA, MH): klara_dense_big.hip
hipError_t klara_launch_dense_big(const KParams* p, const KLaunch& kl, int sampler, bool da, int NE, const double* Pfrag, bool hasmu, dim3 grid, hipStream_t st);
hipError_t klara_launch_dense_init_big(const KParams& p, int NE, const double* Pfrag, bool hasmu, int needgrad, dim3 grid, hipStream_t st);

// the workgroup's dynamic LDS: the precision matrix's fragments + the mean.  (NE = 8 and 16 ask for 8 and 32.5 KB, which every launch gets; 25 and 32 opt in.)
template <int N, bool HASMU> constexpr size_t dense_lds() { return sizeof(double) * (64 * (size_t)N * (size_t)((N + 3) / 4) + (HASMU ? 4 * N : 0)); }

template <int SAMPLER, bool DA, bool PLAIN = false>
static hipError_t launch_dense_s(const KParams* p, const KLaunch& kl, int NE, const double* Pfrag, bool hasmu, dim3 grid, hipStream_t st)
{
    return klara_pick<1, 0>(hasmu, [&](auto m) {
        return klara_pick<8, 16, 25, 32>(NE, [&](auto n) {
            constexpr int N = decltype(n)::value;
            constexpr bool HASMU = decltype(m)::value != 0;
            return klara_go(k_dense_transitions<SAMPLER, N, DA, HASMU, PLAIN>, grid, dim3(512), dense_lds<N, HASMU>(), st, p, kl, Pfrag);
        });
    });
}

hipError_t klara_launch_dense(const KParams* p, const KLaunch& kl, int sampler, int tuner, bool plain, int NE, const double* Pfrag, bool hasmu,
                              dim3 grid, hipStream_t st)
{
    if (NE > 32) return klara_launch_dense_big(p, kl, sampler, tuner == KLARA_TUNER_DUAL_AVERAGING, NE, Pfrag, hasmu, grid, st);
    switch (sampler) {
    case KLARA_SAMPLER_MH: return launch_dense_s<KLARA_SAMPLER_MH, false>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_MALA: return launch_dense_s<KLARA_SAMPLER_MALA, false>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_SLICE: return launch_dense_s<KLARA_SAMPLER_SLICE, false>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_HMC:
        if (tuner == KLARA_TUNER_DUAL_AVERAGING) return launch_dense_s<KLARA_SAMPLER_HMC, true>(p, kl, NE, Pfrag, hasmu, grid, st);
        if (plain) return launch_dense_s<KLARA_SAMPLER_HMC, false, true>(p, kl, NE, Pfrag, hasmu, grid, st);      // nothing counts or tunes: the step is a scalar, no tuner state
        return launch_dense_s<KLARA_SAMPLER_HMC, false>(p, kl, NE, Pfrag, hasmu, grid, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t klara_launch_dense_init(const KParams& p, int NE, const double* Pfrag, bool hasmu, int needgrad, dim3 grid, hipStream_t st)
{
    if (NE > 32) return klara_launch_dense_init_big(p, NE, Pfrag, hasmu, needgrad, grid, st);
    return klara_pick<1, 0>(hasmu, [&](auto m) {
        return klara_pick<8, 16, 25, 32>(NE, [&](auto n) {
            constexpr int N = decltype(n)::value;
            constexpr bool HASMU = decltype(m)::value != 0;
            return klara_start(k_dense_init<N, HASMU>, grid, dim3(512), dense_lds<N, HASMU>(), st, p, Pfrag, needgrad);
        });
    });
}

hipError_t klara_launch_mfma_probe(const double* A, const double* B, const double* C, double* D, hipStream_t st)
{
    return klara_start(k_mfma_f64_probe, dim3(1), dim3(64), 0, st, A, B, C, D);
}

hipError_t klara_launch_mfma4_probe(const double* A, const double* B, const double* C, double* D, hipStream_t st)
{
    return klara_start(k_mfma_f64_4x4x4_probe, dim3(1), dim3(64), 0, st, A, B, C, D);
}
