// klara_amwg.hip — instantiates the AMWG transition kernels (group layout, logistic target, D <= 16, one chain per lane or per row-split group) for gfx950.
// The start state is k_init's (the log-target, as for MH); a user-defined target gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_AMWG) { return launch_group<KLARA_SAMPLER_AMWG>(p, kl, mode, target, E, G, grid, lds, st); }
