// klara_dense_split.hip — instantiates the workgroup-split dense-Gaussian kernels (layout kind 6: 257 <= D <= 1024; HMC — also with dual averaging —, MALA, MH, slice) for gfx950.
#include "klara_launch.h"
#define KLARA_DENSE_NO_PROBES 1
#include "klara_dense_split.h"

template <int S, bool DA = false>
static hipError_t go_split_s(const KParams* p, const KLaunch& kl, int W, int NEW, int MW, size_t lds, int D, const double* Pfrag, bool hasmu, dim3 grid, hipStream_t st)
{
    if (W > KLARA_SPLIT_WMAX || W * (NEW / 4) < (D + 15) / 16) return hipErrorInvalidValue;
    return klara_pick<32, 24, 16>(NEW, [&](auto n) {
        return klara_pick<2, 3, 4>(MW == 2 || MW == 3 ? MW : 4, [&](auto w) {
            return klara_pick<1, 0>(hasmu, [&](auto m) {
                return klara_go(k_dense_split<S, DA, decltype(m)::value != 0, decltype(w)::value, decltype(n)::value>, grid, dim3(64 * W), lds, st, p, kl, Pfrag);
            });
        });
    });
}

hipError_t klara_launch_dense_split(const KParams* p, const KLaunch& kl, int sampler, bool da, int W, int NEW, int MW, size_t lds, int D, const double* Pfrag, bool hasmu, dim3 grid,
                                   hipStream_t st)
{
    switch (sampler) {
    case KLARA_SAMPLER_HMC: return da ? go_split_s<KLARA_SAMPLER_HMC, true>(p, kl, W, NEW, MW, lds, D, Pfrag, hasmu, grid, st) : go_split_s<KLARA_SAMPLER_HMC>(p, kl, W, NEW, MW, lds, D, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_MALA: return go_split_s<KLARA_SAMPLER_MALA>(p, kl, W, NEW, MW, lds, D, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_MH: return go_split_s<KLARA_SAMPLER_MH>(p, kl, W, NEW, MW, lds, D, Pfrag, hasmu, grid, st);
    case KLARA_SAMPLER_SLICE: return go_split_s<KLARA_SAMPLER_SLICE>(p, kl, W, NEW, MW, lds, D, Pfrag, hasmu, grid, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t klara_launch_dense_split_init(const KParams& p, int W, int NEW, size_t lds, const double* Pfrag, bool hasmu, int needgrad, dim3 grid, hipStream_t st)
{
    if (W > KLARA_SPLIT_WMAX || W * (NEW / 4) < (p.D + 15) / 16) return hipErrorInvalidValue;
    return klara_pick<32, 24, 16>(NEW, [&](auto n) {
        return klara_pick<1, 0>(hasmu, [&](auto m) {
            return klara_start(k_dense_split_init<decltype(m)::value != 0, decltype(n)::value>, grid, dim3(64 * W), lds, st, p, Pfrag, needgrad);
        });
    });
}
