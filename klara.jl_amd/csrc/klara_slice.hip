// klara_slice.hip — instantiates the SLICE transition kernels (group layout) for gfx950.
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_SLICE) { return launch_group<KLARA_SAMPLER_SLICE>(p, kl, mode, target, E, G, grid, lds, st); }
