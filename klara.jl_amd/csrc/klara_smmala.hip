// klara_smmala.hip — instantiates the SMMALA transition kernels (group layout, logistic target, D <= 8) for gfx950, and their start-state kernel
// (k_init_smmala, klara_kernels.h).  A user-defined target with a tensor function gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

hipError_t klara_launch_smmala(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st)
{
    if (target != KLARA_TARGET_LOGISTIC) return hipErrorInvalidValue;
    return klara_pick<2, 4, 8>(E, [&](auto e) {
        return launch_transitions<KLARA_SAMPLER_SMMALA, KLARA_TARGET_LOGISTIC, decltype(e)::value, 0>(p, kl, mode, grid, lds, st);
    });
}

hipError_t klara_launch_smmala_init(const KParams& p, int E, dim3 grid, size_t lds, hipStream_t st)
{
    return klara_pick<2, 4, 8>(E, [&](auto e) {
        return klara_start(k_init_smmala<KLARA_TARGET_LOGISTIC, decltype(e)::value, 0>, grid, dim3(256), lds, st, p, 1);
    });
}
