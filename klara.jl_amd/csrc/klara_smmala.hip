// klara_smmala.hip — instantiates the SMMALA transition kernels (group layout, logistic target, D <= 8) for gfx950, and their start-state kernel
// (k_init_smmala, klara_kernels.h).  A user-defined target with a tensor function gets the same kernels from the run-time compiler (klara_jit.hip).
#include "klara_launch.h"

hipError_t klara_launch_smmala(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st)
{
    const dim3 blk(256);
    if (target != KLARA_TARGET_LOGISTIC) return hipErrorInvalidValue;
    if (E == 2) KLARA_LAUNCH_T(KLARA_SAMPLER_SMMALA, KLARA_TARGET_LOGISTIC, 2, 0);
    else if (E == 4) KLARA_LAUNCH_T(KLARA_SAMPLER_SMMALA, KLARA_TARGET_LOGISTIC, 4, 0);
    else if (E == 8) KLARA_LAUNCH_T(KLARA_SAMPLER_SMMALA, KLARA_TARGET_LOGISTIC, 8, 0);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t klara_launch_smmala_init(const KParams& p, int E, dim3 grid, size_t lds, hipStream_t st)
{
#define KLARA_SMMALA_INIT(E_)                                                                                                          \
    do {                                                                                                                               \
        if (lds > KLARA_LDS_DEFAULT_DYNAMIC) {                                                                                         \
            const hipError_t e_ = hipFuncSetAttribute((const void*)k_init_smmala<KLARA_TARGET_LOGISTIC, E_, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e_ != hipSuccess) return e_;                                                                                           \
        }                                                                                                                              \
        hipLaunchKernelGGL((k_init_smmala<KLARA_TARGET_LOGISTIC, E_, 0>), grid, dim3(256), lds, st, p, 1);                                                          \
    } while (0)
    if (E == 2) KLARA_SMMALA_INIT(2);
    else if (E == 4) KLARA_SMMALA_INIT(4);
    else if (E == 8) KLARA_SMMALA_INIT(8);
    else return hipErrorInvalidValue;
#undef KLARA_SMMALA_INIT
    return hipGetLastError();
}
