// klara_logit_mfma.hip — instantiates the matrix-core logistic-regression kernels (layout kind 5: 17 <= D <= 256, NE = 8, 16, 24, 32, 40, 48, 56, 64 elements per lane;
// MH, MALA, HMC — also with dual averaging —, slice) for gfx950.
#include "klara_launch.h"
#define KLARA_DENSE_NO_PROBES 1
#include "klara_logit_mfma.h"

template <int S, bool DA = false>
static hipError_t go_logitm_s(const KParams* p, const KLaunch& kl, int NE, const double* F, const double* ypad, int nblocks, dim3 grid, hipStream_t st)
{
    return klara_pick<8, 16, 24, 32, 40, 48, 56, 64>(NE, [&](auto n) {
        constexpr int N = decltype(n)::value;
        // kd_log12's table + MH's sigma + one column per lane of the four wavefronts (momentum / normals / current value)
        constexpr size_t lds = sizeof(double) * (256 + (S == KLARA_SAMPLER_MH ? 4 * N : 0) + 4 * (size_t)N * 64);
        return klara_go(k_logit_mfma<S, N, DA>, grid, dim3(256), lds, st, p, kl, F, ypad, nblocks);
    });
}

hipError_t klara_launch_logit_mfma(const KParams* p, const KLaunch& kl, int sampler, bool da, int NE, const double* F, const double* ypad, int nblocks, dim3 grid, hipStream_t st)
{
    switch (sampler) {
    case KLARA_SAMPLER_HMC: return da ? go_logitm_s<KLARA_SAMPLER_HMC, true>(p, kl, NE, F, ypad, nblocks, grid, st) : go_logitm_s<KLARA_SAMPLER_HMC>(p, kl, NE, F, ypad, nblocks, grid, st);
    case KLARA_SAMPLER_MALA: return go_logitm_s<KLARA_SAMPLER_MALA>(p, kl, NE, F, ypad, nblocks, grid, st);
    case KLARA_SAMPLER_MH: return go_logitm_s<KLARA_SAMPLER_MH>(p, kl, NE, F, ypad, nblocks, grid, st);
    case KLARA_SAMPLER_SLICE: return go_logitm_s<KLARA_SAMPLER_SLICE>(p, kl, NE, F, ypad, nblocks, grid, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t klara_launch_logit_mfma_init(const KParams& p, int NE, const double* F, const double* ypad, int nblocks, int needgrad, dim3 grid, hipStream_t st)
{
    return klara_pick<8, 16, 24, 32, 40, 48, 56, 64>(NE, [&](auto n) {
        return klara_start(k_logit_mfma_init<decltype(n)::value>, grid, dim3(256), 0, st, p, F, ypad, nblocks, needgrad);
    });
}

int klara_logit_mfma_rbt() { return KLARA_LOGITM_RBT; }
