// klara_mh.hip — instantiates the MH transition kernels (group layout) for gfx950.
#include "klara_launch.h"

hipError_t klara_launch_mh(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds,
                            hipStream_t st)
{
    return launch_group<KLARA_SAMPLER_MH>(p, kl, mode, target, E, G, grid, lds, st);
}
