// klara_smmala.hip — instantiates the SMMALA transition kernels (group layout, logistic target, D <= 8) for gfx950, and their start-state kernel
// (k_init_smmala, klara_kernels.h).  A user-defined target with a tensor function gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_SMMALA) { return launch_group<KLARA_SAMPLER_SMMALA>(p, kl, mode, target, E, G, grid, lds, st); }

hipError_t klara_launch_smmala_init(const KParams& p, int E, dim3 grid, size_t lds, hipStream_t st)
{
    return klara_pick<2, 4, 8>(E, [&](auto e) {
        return klara_start(k_init_smmala<KLARA_TARGET_LOGISTIC, decltype(e)::value, 0>, grid, dim3(256), lds, st, p, 1);
    });
}
