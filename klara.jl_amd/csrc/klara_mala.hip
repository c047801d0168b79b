// klara_mala.hip — instantiates the MALA transition kernels (group layout) for gfx950.
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MALA) { return launch_group<KLARA_SAMPLER_MALA>(p, kl, mode, target, E, G, grid, lds, st); }
