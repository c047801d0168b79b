// klara_amwg.hip — instantiates the AMWG transition kernels (group layout, logistic target, D <= 16, one chain per lane or per row-split group) for gfx950.
// The start state is k_init's (the log-target, as for MH); a user-defined target gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

hipError_t klara_launch_amwg(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st)
{
    if (target != KLARA_TARGET_LOGISTIC || G != 1) return hipErrorInvalidValue;
    return klara_pick<2, 4, 8, 16>(E, [&](auto e) {
        return launch_transitions<KLARA_SAMPLER_AMWG, KLARA_TARGET_LOGISTIC, decltype(e)::value, 0>(p, kl, mode, grid, lds, st);
    });
}
