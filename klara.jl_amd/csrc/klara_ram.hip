// klara_ram.hip — instantiates the RAM transition kernels (group layout, logistic target, D <= 8) for gfx950.  The start state is k_init's (the log-target,
// as for MH); a user-defined target gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_RAM) { return launch_group<KLARA_SAMPLER_RAM>(p, kl, mode, target, E, G, grid, lds, st); }
