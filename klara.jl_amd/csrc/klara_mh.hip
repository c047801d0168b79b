// klara_mh.hip — instantiates the MH transition kernels (group layout) for gfx950.
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MH) { return launch_group<KLARA_SAMPLER_MH>(p, kl, mode, target, E, G, grid, lds, st); }
