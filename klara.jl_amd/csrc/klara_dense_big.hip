// klara_dense_big.hip — instantiates the streamed dense-Gaussian kernels (D = 129 .. 256: NE = 40, 48, 56, 64 elements per lane; HMC — also with dual averaging —, MALA, MH, slice) for gfx950.
#include "klara_launch.h"
#define KLARA_DENSE_NO_PROBES 1
#include "klara_dense_big.h"

template <int S, bool DA = false>
static hipError_t go_big_s(const KParams* p, const KLaunch& kl, int NE, const double* Pfrag, bool hasmu, dim3 grid, hipStream_t st)
{
    return klara_pick<40, 48, 56, 64>(NE, [&](auto n) {
        return klara_pick<1, 0>(hasmu, [&](auto m) {
            constexpr int N = decltype(n)::value;
            constexpr bool HASMU = decltype(m)::value != 0;
            // mu, MH's sigma, one column per lane of the 4 wavefronts (HMC: momentum, MALA: the proposal's normals; none for the slice sampler)
            constexpr size_t lds = sizeof(double) * ((HASMU ? 4 * N : 0) + (S == KLARA_SAMPLER_MH ? 4 * N : 0) + (S == KLARA_SAMPLER_SLICE ? 0 : 4 * (size_t)N * 64));
            return klara_go(k_dense_big<S, N, HASMU, DA>, grid, dim3(256), lds, st, p, kl, Pfrag);
        });
    });
}

hipError_t klara_launch_dense_big(const KParams* p, const KLaunch& kl, int sampler, bool da, int NE, const double* Pfrag, bool hasmu, dim3 grid, hipStream_t st)
{
    switch (sampler) {
    case KLARA_SAMPLER_HMC: return da ? go_big_s<KLARA_SAMPLER_HMC, true>(p, kl, NE, Pfrag, hasmu, grid, st) : go_big_s<KLARA_SAMPLER_HMC>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_MALA: return go_big_s<KLARA_SAMPLER_MALA>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_MH: return go_big_s<KLARA_SAMPLER_MH>(p, kl, NE, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_SLICE: return go_big_s<KLARA_SAMPLER_SLICE>(p, kl, NE, Pfrag, hasmu, grid, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t klara_launch_dense_init_big(const KParams& p, int NE, const double* Pfrag, bool hasmu, int needgrad, dim3 grid, hipStream_t st)
{
    return klara_pick<40, 48, 56, 64>(NE, [&](auto n) {
        return klara_pick<1, 0>(hasmu, [&](auto m) {
            constexpr int N = decltype(n)::value;
            constexpr bool HASMU = decltype(m)::value != 0;
            return klara_start(k_dense_init_big<N, HASMU>, grid, dim3(256), sizeof(double) * (HASMU ? 4 * N : 0), st, p, Pfrag, needgrad);
        });
    });
}
