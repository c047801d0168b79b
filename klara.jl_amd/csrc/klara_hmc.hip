// klara_hmc.hip — instantiates the HMC transition kernels (group layout) for gfx950.
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_HMC) { return launch_group<KLARA_SAMPLER_HMC>(p, kl, mode, target, E, G, grid, lds, st); }
