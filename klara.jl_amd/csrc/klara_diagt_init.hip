// klara_diagt_init.hip — initialize! for layout kind 3 (lt and gradient at X).
#include "klara_launch.h"

hipError_t KLARA_DIAGT_FN(klara_launch_diagt_init)(const KParams& p, int NP, int needgrad, dim3 grid, hipStream_t st)
{
    return klara_pick<KLARA_DIAGT_NP_MENU>(NP, [&](auto np) {
        return klara_start(k_diagt_init<decltype(np)::value, KLARA_DIAGT_Q>, grid, dim3(256), 0, st, p, needgrad);
    });
}
