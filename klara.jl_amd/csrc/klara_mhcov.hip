// klara_mhcov.hip — instantiates the MH(Σ) transition kernels (KLARA_SAMPLER_MH_COV: group layout, logistic target, D <= 16, one chain per lane or per
// row-split group) for gfx950.  The start state is k_init's, as for MH; a user-defined target gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MH_COV) { return launch_group<KLARA_SAMPLER_MH_COV>(p, kl, mode, target, E, G, grid, lds, st); }
