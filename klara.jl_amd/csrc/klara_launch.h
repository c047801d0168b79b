// klara_launch.h — launcher prototypes implemented by the per-sampler translation units
#pragma once
#include <stdlib.h>
#include <string.h>
#include "klara_kernels.h"
#include "klara_diagt.h"

// How a kernel is launched — the one place.  Two entry points over one body, klara_launch_kernel<QUERY>:
//   klara_go     every transition (step) kernel.  When klara_attr_query points at a hipFuncAttributes (klara_get_kernel_attributes, klara_monitors.hip)
//                it reports the kernel's registers / scratch / LDS instead of launching it — the dispatch code that picks an instantiation for a job
//                is then the one source of truth for "which kernel does this handle run".
//   klara_start  the init / start-state kernels (and the self test): never queried, always launched.
// The opt-in rule: a launch gets 64 KB of LDS — 8 KB of math tables + KLARA_LDS_DEFAULT_DYNAMIC = 56 KB of dynamic — without asking; a launch that asks
// for more dynamic LDS opts in first (raises the kernel's limit), on every such launch (nothing remembers that the attribute is set), and BEFORE the query,
// so a queried kernel reports the attributes it is launched with.  Both return the first error: the opt-in's, the query's or the launch's.
#ifndef KLARA_LDS_DEFAULT_DYNAMIC
#define KLARA_LDS_DEFAULT_DYNAMIC 57344u
#endif
extern thread_local hipFuncAttributes* klara_attr_query;
template <bool QUERY, class... KArgs, class... Args>
static inline hipError_t klara_launch_kernel(void (*kern)(KArgs...), dim3 grid, dim3 blk, size_t lds, hipStream_t st, Args... args)
{
    if (lds > KLARA_LDS_DEFAULT_DYNAMIC) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (QUERY && klara_attr_query != nullptr) return hipFuncGetAttributes(klara_attr_query, (const void*)kern);
    hipLaunchKernelGGL(kern, grid, blk, lds, st, args...);
    return hipGetLastError();
}
template <class K, class... Args>
static inline hipError_t klara_go(K kern, dim3 grid, dim3 blk, size_t lds, hipStream_t st, Args... args)
{
    return klara_launch_kernel<true>(kern, grid, blk, lds, st, args...);
}
template <class K, class... Args>
static inline hipError_t klara_start(K kern, dim3 grid, dim3 blk, size_t lds, hipStream_t st, Args... args)
{
    return klara_launch_kernel<false>(kern, grid, blk, lds, st, args...);
}

// A run-time integer as a template argument: calls f(KInt<N>()) for the N of the menu Ns... equal to v (a bool: the menu <1, 0>); a value that is
// not on the menu is hipErrorInvalidValue.  Every launcher's "which instantiation" ladder is one of these; the menu says what is instantiated.
template <int... Ns, class F>
static inline hipError_t klara_pick(int v, F&& f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)(... || (v == Ns ? (e = f(KInt<Ns>()), true) : false));     // (a left fold: the menu is instantiated in its order)
    return e;
}

// Forward-mode autodiff of a user-defined target (klara_autodiff.h): the value of the source's `#define KLARA_USER_AUTODIFF n` marker — 1: the gradient,
// 2: also the SMMALA metric (minus the Hessian) — or 0 for a source without it.  (KLARA_USER_AUTODIFF_CHUNK is another name.)
static inline int klara_autodiff_order(const char* src)
{
    static const char name[] = "KLARA_USER_AUTODIFF";
    for (const char* s = src ? strstr(src, name) : nullptr; s != nullptr; s = strstr(s + 1, name)) {
        const char* t = s + sizeof(name) - 1;
        if (*t != ' ' && *t != '\t') continue;
        while (*t == ' ' || *t == '\t') ++t;
        return *t == '2' ? 2 : 1;
    }
    return 0;
}

// group-layout transition kernels: one specialisation per sampler, each defined in a translation unit of its own (klara_{mh,mala,hmc,slice,smmala,ram,am,amwg,mhcov}.hip)
// as launch_group<S> below; G = lanes per chain
template <int S>
hipError_t klara_launch_sampler(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st);
#define KLARA_LAUNCH_SAMPLER(S) \
    template <> hipError_t klara_launch_sampler<S>(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st)
KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MH); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MALA); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_HMC); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_SLICE);
KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_SMMALA); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_RAM); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_AM); KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_AMWG);
KLARA_LAUNCH_SAMPLER(KLARA_SAMPLER_MH_COV);
// SMMALA's start-state kernel on the logistic target (log-target, gradient, metric check); RAM, AM, AMWG and MH(Σ) start from k_init
hipError_t klara_launch_smmala_init(const KParams& p, int E, dim3 grid, size_t lds, hipStream_t st);
// dense (MFMA) kernels; NE in {8,16,25,32}
// (Pfrag: the fragment-ordered precision matrix, followed — hasmu — by the 4 NE zero-padded entries of the mean)
hipError_t klara_launch_dense(const KParams* p, const KLaunch& kl, int sampler, int tuner, bool plain, int NE, const double* Pfrag, bool hasmu,
                              dim3 grid, hipStream_t st);
hipError_t klara_launch_dense_init(const KParams& p, int NE, const double* Pfrag, bool hasmu, int needgrad, dim3 grid,
                                   hipStream_t st);
hipError_t klara_launch_mfma_probe(const double* A, const double* B, const double* C, double* D,
                                   hipStream_t st);
hipError_t klara_launch_mfma4_probe(const double* A, const double* B, const double* C, double* D, hipStream_t st);

// logistic regression beyond 16 parameters on the matrix cores (layout kind 5, klara_logit_mfma.h); NE in {8, 16, 24, 32}; F: the fragment stream of both
// passes in the order of consumption, ypad: the responses zero-padded to the blocks' rows (klara_create.hip pack_logit_stream)
hipError_t klara_launch_logit_mfma(const KParams* p, const KLaunch& kl, int sampler, bool da, int NE, const double* F, const double* ypad, int nblocks,
                                   dim3 grid, hipStream_t st);
hipError_t klara_launch_logit_mfma_init(const KParams& p, int NE, const double* F, const double* ypad, int nblocks, int needgrad, dim3 grid, hipStream_t st);
int klara_logit_mfma_rbt();
// dense Gaussian on a workgroup of W wavefronts per tile of 16 chains (layout kind 6, klara_dense_split.h): 257 <= D <= 1024; MH, MALA, HMC, slice.
// W, NEW (elements per lane and wavefront), MW (registers for MW wavefronts per SIMD) and the workgroup's dynamic LDS bytes come from the job's plan (klara_plan.h)
hipError_t klara_launch_dense_split(const KParams* p, const KLaunch& kl, int sampler, bool da, int W, int NEW, int MW, size_t lds, int D, const double* Pfrag, bool hasmu, dim3 grid,
                                   hipStream_t st);
hipError_t klara_launch_dense_split_init(const KParams& p, int W, int NEW, size_t lds, const double* Pfrag, bool hasmu, int needgrad, dim3 grid, hipStream_t st);

// pair-transposed diagonal-Gaussian kernels (layout kind 3, klara_diagt.h).  The translation units klara_diagt_*.hip are
// compiled four times: Q = 8 lanes per chain (17 <= D <= 128, NP = ceil(D/16) in 2..8), Q = 16 (129 <= D <= 256), Q = 32
// (257 <= D <= 512) and (round 6) Q = 64 (513 <= D <= 1024: north_star's one chain per wavefront), the latter three with NP in 5..8; the launchers of the
// wider variants carry a _q16 / _q32 / _q64 suffix.
#if KLARA_DIAGT_Q == 8
#define KLARA_DIAGT_FN(name) name
#elif KLARA_DIAGT_Q == 4
#define KLARA_DIAGT_FN(name) name##_q4
#elif KLARA_DIAGT_Q == 16
#define KLARA_DIAGT_FN(name) name##_q16
#elif KLARA_DIAGT_Q == 32
#define KLARA_DIAGT_FN(name) name##_q32
#elif KLARA_DIAGT_Q == 64
#define KLARA_DIAGT_FN(name) name##_q64
#else
#define KLARA_DIAGT_FN(name) name          // (experimental lane counts replace the Q = 8 set)
#endif
#define KLARA_DIAGT_DECLARE(SUFFIX)                                                                                                                       \
    hipError_t klara_launch_diagt_mh##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st);   \
    hipError_t klara_launch_diagt_mala##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st); \
    hipError_t klara_launch_diagt_hmc##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st);  \
    hipError_t klara_launch_diagt_slice##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool unitw, bool mon, bool tune, const KAuto& ka, long long nwaves, hipStream_t st);                      \
    hipError_t klara_launch_diagt_slice_free##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool unitw, bool mon, const KAuto& ka, long long nwaves, int nm, hipStream_t st);                   \
    hipError_t klara_launch_diagt_hist_lt##SUFFIX(const KParams* p, const KLaunch& kl, int NP, bool unitw, long long col0, int ncols, long long ngroups, hipStream_t st);                              \
    hipError_t klara_launch_diagt_init##SUFFIX(const KParams& p, int NP, int needgrad, dim3 grid, hipStream_t st);
KLARA_DIAGT_DECLARE()
KLARA_DIAGT_DECLARE(_q16)
KLARA_DIAGT_DECLARE(_q32)
KLARA_DIAGT_DECLARE(_q64)
// Q = 4 lanes per chain, 16 chains per wavefront, NP = ceil(D/8) in 3..13 (17 <= D <= 104): jobs in which nothing counts or tunes
// (VanillaMCTuner, not verbose) with the MH or the MALA sampler — D = 100 occupies 50 of 52 pair slots instead of 50 of 56, the
// per-wavefront work (reductions, accept test, addressing) is shared by 16 chains, and the running sums are folded with atomic
// adds instead of living in registers (klara_diagt.h diagt_fold_atomic).  Only klara_diagt_{mh,mala,init}.hip are built for it.
hipError_t klara_launch_diagt_mh_q4(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st);
hipError_t klara_launch_diagt_mala_q4(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st);
hipError_t klara_launch_diagt_hmc_q4(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves, hipStream_t st);
hipError_t klara_launch_diagt_init_q4(const KParams& p, int NP, int needgrad, dim3 grid, hipStream_t st);
// pairs per lane the kernels are instantiated for; a job takes NP = ceil(ceil(D/2) / Q) exactly (only the LAST pair of a lane
// can be padding)
// (a klara_pick menu)
#if KLARA_DIAGT_Q == 4
#define KLARA_DIAGT_NP_MENU 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
#elif KLARA_DIAGT_Q == 8
#define KLARA_DIAGT_NP_MENU 2, 3, 4, 5, 6, 7, 8
#else                      // Q = 16 / 32 start where the narrower variant ends: NP = 5..8
#define KLARA_DIAGT_NP_MENU 5, 6, 7, 8
#endif
#define KLARA_DIAGT_NP_MAX 8

// one launch of a pair-transposed kernel over `nwaves` chain groups: one wavefront each, four per workgroup.  The kernels that read the angle's
// remainder terms from an LDS table (klara_diagt.h SCTAB) get the table's 64 KB of dynamic LDS; a launch too short to amortise the fill
// runs the arithmetic instantiation (the same bits).
static_assert(KD_SCREM_BYTES > KLARA_LDS_DEFAULT_DYNAMIC, "the table is more than a launch gets without asking: klara_go opts in");
template <int S, int NP_, int Q_, bool ONESTEP, bool UNITW, bool MON, bool TUNE = false, bool DA = false>
static hipError_t diagt_go(const KParams* p, const KLaunch& kl, const KAuto& ka, long long nwaves, hipStream_t st)
{
    const dim3 grid((unsigned)((nwaves + 3) / 4)), blk(256);
    if constexpr (diagt_sctab<S, NP_, Q_, ONESTEP, UNITW, MON, TUNE>()) {
        if (kl.nsteps >= KLARA_SCTAB_MIN_STEPS) {
            constexpr int WPG = diagt_wg_threads<Q_, true>() / 64;       // wavefronts (chain groups) per workgroup of the table kernel
            return klara_go(k_diagt<S, NP_, Q_, ONESTEP, UNITW, MON, TUNE, DA, false, true>, dim3((unsigned)((nwaves + WPG - 1) / WPG)), dim3(64 * WPG),
                            (size_t)KD_SCREM_BYTES, st, p, kl, ka);
        }
    }
    return klara_go(k_diagt<S, NP_, Q_, ONESTEP, UNITW, MON, TUNE, DA>, grid, blk, 0, st, p, kl, ka);
}
// ... both forms of the diagonal (unit weights or not) of one (ONESTEP, MON, TUNE, DA) row of the flag ladders
template <int S, int NP_, bool ONESTEP, bool MON, bool TUNE = false, bool DA = false>
static hipError_t diagt_row(const KParams* p, const KLaunch& kl, bool unitw, const KAuto& ka, long long nwaves, hipStream_t st)
{
    return unitw ? diagt_go<S, NP_, KLARA_DIAGT_Q, ONESTEP, true, MON, TUNE, DA>(p, kl, ka, nwaves, st)
                 : diagt_go<S, NP_, KLARA_DIAGT_Q, ONESTEP, false, MON, TUNE, DA>(p, kl, ka, nwaves, st);
}
// the MH / MALA / HMC launchers of klara_diagt_{mh,mala,hmc}.hip: NP, then the flag ladder — dual averaging (its kernel state only in HMC),
// a tuner, a monitor, one transition per launch, plain
template <int S>
static hipError_t launch_diagt(const KParams* p, const KLaunch& kl, int NP, bool onestep, bool unitw, bool mon, bool tune, bool da, const KAuto& ka, long long nwaves,
                               hipStream_t st)
{
    return klara_pick<KLARA_DIAGT_NP_MENU>(NP, [&](auto np) {
        constexpr int NP_ = decltype(np)::value;
        if constexpr (KLARA_DIAGT_Q == 4) {     // (no tuned / dual-averaging instantiations: those jobs take the 8-lane form)
            if (tune || da) return hipErrorInvalidValue;
        } else {
            if (da) return diagt_row<S, NP_, false, true, true, (S == KLARA_SAMPLER_HMC)>(p, kl, unitw, ka, nwaves, st);
            if (tune) return diagt_row<S, NP_, false, true, true>(p, kl, unitw, ka, nwaves, st);
        }
        if (mon) return diagt_row<S, NP_, false, true>(p, kl, unitw, ka, nwaves, st);
        if (onestep) return diagt_row<S, NP_, true, false>(p, kl, unitw, ka, nwaves, st);
        return diagt_row<S, NP_, false, false>(p, kl, unitw, ka, nwaves, st);
    });
}

// MH / MALA / HMC on the hierarchical target, 8 lanes per chain (layout kind 4, klara_hiert.h); RPL = 4 units per lane, NT = 5
hipError_t klara_launch_hiert(const KParams* p, const KLaunch& kl, int sampler, int RPL, int NT, bool mon, bool tune, bool da, dim3 grid,
                              hipStream_t st);
hipError_t klara_launch_hiert_init(const KParams& p, int RPL, int NT, int needgrad, dim3 grid, hipStream_t st);

// user-defined targets (KLARA_TARGET_CUSTOM): run-time compiled instantiations of k_init / k_transitions (klara_jit.hip);
// `modes` are the k_transitions MODE values the job can launch; load = false only compiles (no GPU needed); softabs: the SMMALA kernels with
// the softabs transform of the metric (klara_desc.smmala_softabs > 0, klara_softabs.h) — a code object of its own
struct KlaraJit;
klara_status klara_jit_create(const char* src, int sampler, int D, int E, int G, const int* modes, int nmodes, bool load, KlaraJit** out,
                              bool softabs = false);
// pair closures (`#define KLARA_USER_PAIR_TARGET 1` + klara_user_pair, klara_diagt.h USERPAIR): k_diagt_init / k_diagt instantiated
// for the job's NP pairs per lane, Q lanes per chain and monitor / tuner flags; modes: 0 = fused launches, 1 = one transition per launch
klara_status klara_jit_create_pair(const char* src, int sampler, int D, int NP, int Q, bool mon, bool tune, bool da, const int* modes, int nmodes,
                                   bool load, KlaraJit** out);
hipError_t klara_jit_launch_pair(KlaraJit* j, int mode, const KParams* p, const KLaunch& kl, long long nwaves, hipStream_t st);
void klara_jit_destroy(KlaraJit* j);
hipError_t klara_jit_launch_init(KlaraJit* j, const KParams& p, int needgrad, dim3 grid, size_t lds, hipStream_t st, int block = 256);
hipError_t klara_jit_launch(KlaraJit* j, int mode, const KParams* p, const KLaunch& kl, dim3 grid, size_t lds, hipStream_t st, int block = 256);
const char* klara_jit_log();
// derived quantities (klara_desc.derived_nout > 0, klara_derived.h): k_derived_update compiled with the user's klara_user_derived for (D, K, staging on / off)
// — a second module beside the target's, for any target family; load = false only compiles (klara_check_derived).  The launch is one piece of at most
// KLARA_DERIVED_MAX_COLS columns.
struct KDerivedGeom;
klara_status klara_jit_create_derived(const char* src, int D, int K, bool stage, bool load, KlaraJit** out);
hipError_t klara_jit_launch_derived(KlaraJit* j, const KDerivedGeom& g, const double* hist, long long col0, int m, const double* data, long long ndata,
                                    double* dsum, double* dsumsq, double* stage, hipStream_t st);

// the group-layout transition kernels' MODE — 7: mode 3 with exactly one transition per launch; 3: nothing counts/tunes and nothing is monitored;
// 1: nothing counts/tunes; 0: general — from the launch's mode bits.  (The logistic target's data rows may need more LDS than a launch gets without asking.)
template <int S, int T, int E_, int G_>
static hipError_t launch_transitions(const KParams* p, const KLaunch& kl, int mode, dim3 grid, size_t lds, hipStream_t st)
{
    return klara_pick<7, 3, 1, 0>(mode == 7 ? 7 : (mode & 3) == 3 ? 3 : (mode & 1), [&](auto m) {
        return klara_go(k_transitions<S, T, E_, G_, decltype(m)::value>, grid, dim3(256), lds, st, p, kl);
    });
}

// every group-layout launcher: E = 2 and 4 for every target, 8 for all but the hierarchical one, 16 for the logistic regression alone — of those, what the
// sampler is built for (SamplerOf<S>::built_in; anything else is hipErrorInvalidValue); G != 0 names the diagonal target's one chain per wavefront
// (2, 64) and per half (4, 32).  (The logistic and hierarchical targets have one instantiation per E: the plan gives them G = 1 — RAM, AM, AMWG and MH(Σ), one chain
// per lane, rely on that — so G is not looked at there.)
template <int S>
static hipError_t launch_group(const KParams* p, const KLaunch& kl, int mode, int target, int E, int G, dim3 grid, size_t lds, hipStream_t st)
{
    const auto go = [&](auto t, auto e, auto g) {
        if constexpr (SamplerOf<S>::built_in(decltype(t)::value, decltype(e)::value))
            return launch_transitions<S, decltype(t)::value, decltype(e)::value, decltype(g)::value>(p, kl, mode, grid, lds, st);
        else return hipErrorInvalidValue;
    };
    using G0 = KInt<0>;
    if (target == KLARA_TARGET_GAUSS_DIAG) {
        using T = KInt<KLARA_TARGET_GAUSS_DIAG>;
        if (E == 2) return G == 64 ? go(T(), KInt<2>(), KInt<64>()) : go(T(), KInt<2>(), G0());
        if (E == 4) return G == 32 ? go(T(), KInt<4>(), KInt<32>()) : go(T(), KInt<4>(), G0());
        if (E == 8) return go(T(), KInt<8>(), G0());
        return hipErrorInvalidValue;
    }
    if (target == KLARA_TARGET_LOGISTIC) return klara_pick<2, 4, 8, 16>(E, [&](auto e) { return go(KInt<KLARA_TARGET_LOGISTIC>(), e, G0()); });
    if (target == KLARA_TARGET_HIER_NORMAL) return klara_pick<2, 4>(E, [&](auto e) { return go(KInt<KLARA_TARGET_HIER_NORMAL>(), e, G0()); });
    return hipErrorInvalidValue;
}
