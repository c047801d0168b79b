// klara_diagt_slice.hip — instantiates the pair-transposed slice-sampler kernels (layout kind 3) for gfx950.
#include "klara_launch.h"
#include "klara_diagt_slice.h"

hipError_t KLARA_DIAGT_FN(klara_launch_diagt_slice)(const KParams* p, const KLaunch& kl, int NP, bool unitw, bool mon, bool tune, const KAuto& ka, long long nwaves, hipStream_t st)
{
    return klara_pick<KLARA_DIAGT_NP_MENU>(NP, [&](auto np) {
        constexpr int NP_ = decltype(np)::value;
        if (tune) return diagt_row<KLARA_SAMPLER_SLICE, NP_, false, true, true>(p, kl, unitw, ka, nwaves, st);
        if (mon) return diagt_row<KLARA_SAMPLER_SLICE, NP_, false, true>(p, kl, unitw, ka, nwaves, st);
        return diagt_row<KLARA_SAMPLER_SLICE, NP_, false, false>(p, kl, unitw, ka, nwaves, st);
    });
}

// untuned jobs without a history monitor: every lane takes its element pairs through the whole launch on its own (klara_diagt_slice.h), nm = 1 or 2 machines each
hipError_t KLARA_DIAGT_FN(klara_launch_diagt_slice_free)(const KParams* p, const KLaunch& kl, int NP, bool unitw, bool mon, const KAuto& ka, long long nwaves, int nm, hipStream_t st)
{
    const bool sums = mon;      // (template flag SUMS: a saved-sample monitor — running sums and / or value history — is on)
    if (NP < 1 || NP > KLARA_SLICEF_MAXNP) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nwaves + 3) / 4)), blk(256);
    // dynamic LDS: the widths of the job's 2 NP Q element slots, and weights + means for a non-unit diagonal
    const size_t lds = (size_t)(unitw ? 1 : 3) * 2 * NP * KLARA_DIAGT_Q * sizeof(double);
    const hipError_t e = klara_pick<1, 0>(unitw, [&](auto u) {
        return klara_pick<1, 0>(sums, [&](auto s) {
            return klara_pick<1, 2>(nm == 1 ? 1 : 2, [&](auto m) {
                return klara_go(k_diagt_slice_free<KLARA_DIAGT_Q, decltype(u)::value != 0, decltype(s)::value != 0, decltype(m)::value>, grid, blk, lds, st, p, kl, ka, NP);
            });
        });
    });
    if (e != hipSuccess || klara_attr_query != nullptr) return e;
    // the new state's log-target in the layout's order (the kernel above deals the elements to the lanes round robin): one wavefront per chain group
    return unitw ? klara_go(k_diagt_hist_lt<KLARA_DIAGT_Q, true, true>, grid, blk, 0, st, p, kl, NP, 0LL, 1)
                 : klara_go(k_diagt_hist_lt<KLARA_DIAGT_Q, false, true>, grid, blk, 0, st, p, kl, NP, 0LL, 1);
}

// log-target history of the `ncols` states a launch of the kernel above saved (columns col0 ...), from their saved values
hipError_t KLARA_DIAGT_FN(klara_launch_diagt_hist_lt)(const KParams* p, const KLaunch& kl, int NP, bool unitw, long long col0, int ncols, long long ngroups, hipStream_t st)
{
    if (ncols <= 0 || ngroups <= 0) return hipSuccess;
    const long long nwaves = ngroups * ncols;
    const dim3 grid((unsigned)((nwaves + 3) / 4)), blk(256);
    return unitw ? klara_go(k_diagt_hist_lt<KLARA_DIAGT_Q, true>, grid, blk, 0, st, p, kl, NP, col0, ncols)
                 : klara_go(k_diagt_hist_lt<KLARA_DIAGT_Q, false>, grid, blk, 0, st, p, kl, NP, col0, ncols);
}
