// klara_plan.h — host only: which kernels run a job, on which layout, grid and LDS.  klara_create plans a job once (klara_plan_job) and the
// handle keeps the plan; klara_check_custom_target and klara_selftest_plan plan through the same function.  No device calls, no globals.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include "klara_launch.h"

// user-defined targets keep the whole vector in one lane (klara_custom.h): pow2ceil(D) elements per lane
#ifndef KLARA_CUSTOM_MAXD
#define KLARA_CUSTOM_MAXD 1024           // (round 6: 64 lanes x 16 elements of the staged form; 256 before)
#endif
// element machines per lane of the free-running slice kernels (klara_diagt_slice.h)
#ifndef KLARA_SLICEF_DEFAULT_NM
#define KLARA_SLICEF_DEFAULT_NM 1     // (same box, 65,536 x 100: 9.7e10 coordinate updates/s with one machine per lane, 9.5e10 with two: profiles/r5_ab_slice.txt)
#endif

// The switches of INTEGRATION.md that choose layouts, kernels and launch geometry (not the run-time compiler's, not KLARA_DEBUG_CANARY), read at once: named
// without KLARA_, in lower case; *_set: present at all; numbers are 0 where unset, and the library's own choice stands wherever a value is out of range.
struct KlaraOverrides {
    bool layout_kind0, layout_e_set, logit_no_mfma, dense_no_stream, dense_slice_no_stream, dense_split, dense_no_split, slice_lockstep,
         diagt_no_q4, diagt_no_q4_hmc, pair_slice_as_whole, custom_wpb_set, auto_threshold_set;
    int layout_e, logit_rowsplit, split_mw, split_w, split_new, slice_machines, custom_lanes, custom_wpb;
    long long groups_per_wave; double auto_threshold;
};

static KlaraOverrides klara_read_overrides()
{
    const auto has = [](const char* name) { return getenv(name) != nullptr; };
    const auto num = [](const char* name) { const char* s = getenv(name); return s ? atoi(s) : 0; };
    KlaraOverrides o = {};
    o.layout_kind0 = has("KLARA_LAYOUT_KIND") && num("KLARA_LAYOUT_KIND") == 0; o.layout_e_set = has("KLARA_LAYOUT_E"); o.layout_e = num("KLARA_LAYOUT_E");
    o.logit_no_mfma = has("KLARA_LOGIT_NO_MFMA"); o.logit_rowsplit = num("KLARA_LOGIT_ROWSPLIT");
    o.dense_no_stream = has("KLARA_DENSE_NO_STREAM"); o.dense_slice_no_stream = has("KLARA_DENSE_SLICE_NO_STREAM");
    o.dense_split = num("KLARA_DENSE_SPLIT") != 0; o.dense_no_split = has("KLARA_DENSE_NO_SPLIT");
    o.split_mw = num("KLARA_SPLIT_MW"); o.split_w = num("KLARA_SPLIT_W"); o.split_new = num("KLARA_SPLIT_NEW");
    o.slice_lockstep = has("KLARA_SLICE_LOCKSTEP"); o.slice_machines = !has("KLARA_SLICE_MACHINES") ? KLARA_SLICEF_DEFAULT_NM : num("KLARA_SLICE_MACHINES") == 1 ? 1 : 2;
    o.diagt_no_q4 = has("KLARA_DIAGT_NO_Q4"); o.diagt_no_q4_hmc = has("KLARA_DIAGT_NO_Q4_HMC"); o.pair_slice_as_whole = has("KLARA_PAIR_SLICE_AS_WHOLE");
    o.custom_lanes = num("KLARA_CUSTOM_LANES"); o.custom_wpb_set = has("KLARA_CUSTOM_WPB"); o.custom_wpb = num("KLARA_CUSTOM_WPB");
    const char* gpw = getenv("KLARA_GROUPS_PER_WAVE"); const char* thr = getenv("KLARA_AUTO_THRESHOLD");
    o.groups_per_wave = gpw ? atoll(gpw) : 0; o.auto_threshold = thr ? atof(thr) : -1.0; o.auto_threshold_set = o.auto_threshold >= 0.0 && o.auto_threshold <= 1.0;
    return o;
}

// the closure forms klara_create runs a job in (it assembles the data block their closures read): the logistic regression beyond the row-split kernels
// and the matrix cores, the dense Gaussian beyond the matrix-core layouts, a pair closure the pair-transposed kernels do not serve (klara_custom_compose.h)
enum KlaraRewrite { KLARA_REWRITE_NONE = 0, KLARA_REWRITE_LOGIT_WIDE, KLARA_REWRITE_DENSE_WIDE, KLARA_REWRITE_PAIR_AS_WHOLE };

struct KlaraPlan {
    // layout (klara_get_layout).  kind 0: group layout (G lanes x E elems); 1: MFMA (E = NE); 2: logistic row split (RS lanes share a chain's rows, G = 1);
    // 3: pair-transposed (G = Q lanes, E / 2 pairs each); 4: hierarchical; 5: logistic on the matrix cores; 6: split dense (G = W wavefronts, E = NEW)
    int kind = 0, G = 1, E = 2, RS = 1;
    int rewrite = KLARA_REWRITE_NONE, custom_lanes = 0;       // the closure form and the lanes per chain it forces (1: one chain per lane; 0: free)
    bool jit_pair = false, plain = false;                      // a pair closure on the pair-transposed layout (run-time compiled k_diagt); nothing counts or tunes
    int custom_wpb = 4, custom_rows = 2;   // staged closures: wavefronts per workgroup (2 where four wavefronts' rows do not fit the LDS), vectors per chain in LDS (3: likelihood + prior)
    int modes[2] = { 0, 0 }, nmodes = 1;                       // the k_transitions MODE values the job launches (see launch_steps)
    bool q4_ok = false; int np4 = 0;                           // kind 3: the 4-lanes-per-chain kernels run the job too, np4 pairs per lane
    bool slice_free = false; int slice_machines = KLARA_SLICEF_DEFAULT_NM;   // kind 3 slice sampler: lanes out of lockstep, element machines per lane
    bool cov = false;                      // KLARA_MON_COVARIANCE: a consumer of the saved samples (klara_cov.h); stripped from the monitor word the kernels get
    int nparts = 1, family = 1;            // kind 3: chain partitions on streams of their own; kernel family of launches of several transitions (0: 4 lanes, 1: G, -1: KAuto)
    double auto_threshold = 0.06;   // acceptance above which a device-decided launch keeps resident sums (8 lanes) — the measured crossover: the 4-lane kernels' folds are atomic
                                    // adds since round 4 (flat to ~4.5 % acceptance: profiles/r4_acceptance_cost_atomic.txt; round 3's folds crossed at 0.12, r3_acceptance_cost_probe.txt)
    int split_mw = 2; size_t lds = 0;                          // kind 6: registers for MW wavefronts per SIMD; dynamic LDS bytes of the transition and init kernels
    long long groups_per_wave = 1, steps_per_launch = 0;       // group layout: chain groups a persistent wavefront walks over; transitions per launch at most
    unsigned grid_init = 0, grid_steps = 0;                    // workgroups of the init kernels (and the MFMA / kind 3-6 kernels); of the group-layout transitions
};

static int cnt_predicate(const klara_desc& d)
{
    if (d.sampler == KLARA_SAMPLER_MH || d.sampler == KLARA_SAMPLER_SLICE || d.sampler == KLARA_SAMPLER_RAM || d.sampler == KLARA_SAMPLER_AM || d.sampler == KLARA_SAMPLER_MH_COV) return d.verbose != 0;   // (iterate/RAM.jl:68, iterate/AM.jl:80: tuner.verbose)
    if (d.sampler == KLARA_SAMPLER_AMWG) return 0;        // (its window counts are per coordinate and travel with the chain: KParams::amwg_acc; the step-size tuners' state is not used)
    return (d.tuner == KLARA_TUNER_VANILLA && d.verbose) || d.tuner == KLARA_TUNER_ACCEPT_RATE ||
           (d.tuner == KLARA_TUNER_DUAL_AVERAGING && d.verbose);
}

// per-sampler facts: the ids the library serves (0..4, 6, 8, 10 and 12; 5, 7, 9 and 11 are reserved), which samplers carry a gradient, and the tuner's first step
// (tuner_state, samplers.jl:29-45: the slice sampler has none)
static bool sampler_valid(int s) { return (s >= KLARA_SAMPLER_MH && s <= KLARA_SAMPLER_SMMALA) || s == KLARA_SAMPLER_RAM || s == KLARA_SAMPLER_AM || s == KLARA_SAMPLER_AMWG || s == KLARA_SAMPLER_MH_COV; }
static bool sampler_needs_gradient(int s) { return s == KLARA_SAMPLER_MALA || s == KLARA_SAMPLER_HMC || s == KLARA_SAMPLER_SMMALA; }
static double sampler_step0(const klara_desc& d)
{
    return (d.sampler == KLARA_SAMPLER_MH || d.sampler == KLARA_SAMPLER_RAM || d.sampler == KLARA_SAMPLER_AM || d.sampler == KLARA_SAMPLER_AMWG || d.sampler == KLARA_SAMPLER_MH_COV) ? 1.0 : (d.sampler == KLARA_SAMPLER_MALA || d.sampler == KLARA_SAMPLER_SMMALA) ? d.driftstep
         : d.sampler == KLARA_SAMPLER_HMC ? d.leapstep : (double)NAN;
}

static int pow2ceil(int v){ int p = 1; while (p < v) p <<= 1; return p; }

// lanes per chain of the pair-transposed layout (8 to D = 128, then 16, 32, 64)
static int diagt_lanes(int D) { return D <= 128 ? 8 : (D <= 256 ? 16 : (D <= 512 ? 32 : 64)); }

// layout kind 3 serves the jobs whose transition is pure elementwise work plus three sums (see klara_diagt.h):
// diagonal Gaussian, every sampler, every tuner, any monitor
// (D <= 16: the group layout already puts a chain on <= 4 lanes, 16..64 chains per wavefront; Q = 8, 16, 32 or 64 lanes per chain beyond)
static bool diagt_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    return d.target == KLARA_TARGET_GAUSS_DIAG && d.ndims >= 17 && d.ndims <= 2 * 64 * KLARA_DIAGT_NP_MAX && !o.layout_kind0 && !o.layout_e_set;
}

// the slice sampler on the pair-transposed layout with nothing counting: every lane takes its elements through a whole launch on
// its own (klara_diagt_slice.h); a wavefront only waits for its slowest lane once per element slot and launch, so longer launches waste less
// (nothing counts AND nothing tunes — a pooled or dual-averaging tuner setting, verbose or not, runs k_diagt<SLICE> at its 32 transitions per
// launch: the launch length and the kernel choice come from this one predicate)
static bool slice_free_eligible(const klara_desc& d, const KlaraOverrides& o, bool plain)
{
    const uint32_t lane_local = KLARA_MON_ACCEPT | KLARA_MON_SUMMARIES | KLARA_MON_HISTORY | KLARA_MON_HIST_LT | KLARA_MON_COVARIANCE;       // (the last one: a consumer's flag, no kernel sees it)
    const bool values_kept = (d.monitor & KLARA_MON_HISTORY) != 0 || d.acov_maxlag > 0 || (d.monitor & KLARA_MON_COVARIANCE) != 0 || d.marg_nbins > 0 || d.derived_nout > 0;       // (the log-target history is formed from the saved values)
    return diagt_eligible(d, o) && d.sampler == KLARA_SAMPLER_SLICE && plain && !o.slice_lockstep &&
           (d.monitor & ~lane_local) == 0 && (!(d.monitor & KLARA_MON_HIST_LT) || values_kept);
}

// untuned MH / MALA on the pair-transposed layout up to D = 104: 4 lanes per chain, 16 chains per wavefront, NP = ceil(D/8) in 3..13
// (klara_launch.h) — kernels that keep no resident running sums (a moving chain's sums are folded into memory by atomic adds)
static bool q4_eligible(const klara_desc& d, const KlaraOverrides& o, bool plain)
{
    // (round 5: HMC too while no saved-sample monitor is on — 12.5 of 13 pair slots real at D = 100 instead of 6.25 of 7, the reductions in the 8-lane order as
    // for MH / MALA; with running sums or a history the 8-lane kernels keep it: at HMC's acceptance every transition would fold)
    // (a non-unit diagonal beyond 9 pairs per lane spills: those stay on 8 lanes)
    const bool hmc_ok = d.sampler == KLARA_SAMPLER_HMC && (d.monitor & ~(uint32_t)KLARA_MON_ACCEPT) == 0 && d.acov_maxlag == 0 &&
                        ((d.gauss_w == nullptr && d.gauss_mu == nullptr) || d.ndims <= 72) && !o.diagt_no_q4_hmc;
    return diagt_eligible(d, o) && plain && (d.sampler == KLARA_SAMPLER_MH || d.sampler == KLARA_SAMPLER_MALA || hmc_ok) && d.ndims <= 104 &&
           !o.diagt_no_q4;
}

// layout kind 4 (klara_hiert.h): MH / MALA / HMC on the hierarchical target, 8 lanes per chain, 4 units per lane
static bool hiert_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    return d.target == KLARA_TARGET_HIER_NORMAL && d.sampler != KLARA_SAMPLER_SLICE && d.hier_nunits >= 9 && d.hier_nunits <= 32 && !o.layout_kind0 && !o.layout_e_set;
}

// a user target given as a pair closure (`#define KLARA_USER_PAIR_TARGET 1` + klara_user_pair, include/klara_hip.h)
static bool pair_source(const char* src) { return src != nullptr && strstr(src, "KLARA_USER_PAIR_TARGET") != nullptr && strstr(src, "KLARA_PAIR_AS_WHOLE") == nullptr; }
static bool pair_form(const klara_desc& d) { return d.target == KLARA_TARGET_CUSTOM && pair_source(d.custom_src); }
// ... that the pair-transposed kernels do not serve (fewer than 9 pairs, the slice sampler): it runs as a whole-vector closure, the sum over its pairs
// formed by klara_custom_compose.h (round 5; these jobs used to be refused)
// (round 6: the slice sampler takes pair closures on the few-lanes kernels too — k_diagt<SLICE, .., USERPAIR> —; KLARA_PAIR_SLICE_AS_WHOLE=1 keeps the whole-vector form of round 5)
static bool pair_as_whole(const klara_desc& d, const KlaraOverrides& o)
{
    return pair_form(d) && (d.ndims < 17 || (d.sampler == KLARA_SAMPLER_SLICE && o.pair_slice_as_whole));
}
static bool custom_lik_prior(const char* src) { return src != nullptr && strstr(src, "KLARA_USER_LIKELIHOOD_PRIOR") != nullptr; }
// forward-mode autodiff (klara_autodiff.h): the source's marker.  Pair closures are not differentiated; second order (the SMMALA metric as minus the
// Hessian) is the plain whole-vector form's within smmala_eligible's limits, and with any other sampler the marker's 2 means 1.
static int custom_autodiff(const klara_desc& d) { return d.target == KLARA_TARGET_CUSTOM ? klara_autodiff_order(d.custom_src) : 0; }

// Whole-vector closures (klara_custom.h).  Up to 32 dimensions a lane keeps the whole vector in registers (one chain per lane); beyond,
// the chain is spread over G lanes with E = 2 ceil(D / 2G) <= 16 elements each and evaluations read the vector from the chain's row of
// LDS (STAGED).  G: enough lanes for 16 elements per lane, and a workgroup's rows (4 wavefronts x 64 / G chains) within the 56 KB of
// dynamic LDS a launch gets without asking.  `lanes` = 1 keeps one chain per lane at any D (the library's own heavy closures — the
// logistic regression beyond 8 parameters, the dense Gaussian beyond 128 dimensions — cost O(n D) / O(D^2) per evaluation, and the
// G identical evaluations of the staged form would multiply exactly that part; KLARA_CUSTOM_LANES=1 in the environment for a user's).
static size_t custom_stage_bytes(int D, int G, int nrows, int wpb)        // (klara_custom.h klara_custom_stage_stride)
{
    int s = nrows * ((D + 1) & ~1) + 2;
    if ((2 * s) % 64 == 0) s += 2;
    return (size_t)wpb * (size_t)(64 / G) * (size_t)s * sizeof(double);
}
// wpb: wavefronts per workgroup of the staged kernels — 4, or 2 where four wavefronts' rows would not fit and force more lanes per chain.
// One chain per lane (G = 1, E = pow2ceil(D)) where the staged form would hold more than 16 elements per lane or overflow the LDS.
static void custom_layout(int D, int lanes, int nrows, const KlaraOverrides& o, int* G, int* E, int* wpb)
{
    *wpb = 4;
    if (o.custom_lanes >= 1 && o.custom_lanes <= 64 && (o.custom_lanes & (o.custom_lanes - 1)) == 0) lanes = o.custom_lanes;
    if (lanes == 1 || (lanes == 0 && D <= 32)) { *G = 1; *E = pow2ceil(D < 2 ? 2 : D); return; }
    int g = lanes > 1 ? lanes : 4;
    while (g < 64 && (D + 2 * g - 1) / (2 * g) > 8) g *= 2;                      // at most 16 elements per lane (round 6: up to 64 lanes — one chain per wavefront —: D <= 1024)
    int w = 4;
    if (o.custom_wpb_set) { if (o.custom_wpb == 2 || o.custom_wpb == 4) w = o.custom_wpb; }
    else if (g >= 8 && custom_stage_bytes(D, g, nrows, 4) > KLARA_LDS_DEFAULT_DYNAMIC) w = 2;     // (measured: D = 128 +20 %, D = 256 +21 %; at 4 lanes x 16 elements the kernels spill and 8 x 8 on four wavefronts is faster)
    while (g < 64 && custom_stage_bytes(D, g, nrows, w) > KLARA_LDS_DEFAULT_DYNAMIC) g *= 2;
    *G = g; *E = 2 * ((D + 2 * g - 1) / (2 * g)); *wpb = w;
    if (*E > 16 || custom_stage_bytes(D, *G, nrows, w) > KLARA_LDS_DEFAULT_DYNAMIC) { *G = 1; *E = pow2ceil(D); *wpb = 4; }
}

// the dense Gaussian beyond the LDS-resident layouts (D = 129 .. 256) stays on the matrix cores for every sampler — HMC (every tuner), MALA, MH
// and (round 5) the slice sampler (klara_dense_big.h); beyond D = 256 the split layout, or the closure form
static bool dense_streamed(const klara_desc& d, const KlaraOverrides& o)
{
    return d.target == KLARA_TARGET_GAUSS_DENSE && d.ndims > 128 && d.ndims <= 256 && !o.dense_no_stream &&
           (d.sampler != KLARA_SAMPLER_SLICE || !o.dense_slice_no_stream);
}

// the dense Gaussian beyond D = 256 (round 6): the tile of 16 chains on a WORKGROUP of W = 4, 8, 12 or 16 wavefronts that deal the ceil(D / 16) row tiles
// of P evenly, 2 .. 4 each (klara_dense_split.h, layout kind 6; MH, MALA, HMC with every tuner; 257 <= D <= 1024).  KLARA_DENSE_SPLIT=1 in the environment puts the smaller
// dense targets on it as well (measurements, tests).
static bool dense_split(const klara_desc& d, const KlaraOverrides& o)
{
    return d.target == KLARA_TARGET_GAUSS_DENSE && d.ndims <= 64 * 16 && !o.dense_no_split && (d.ndims > 256 || o.dense_split);
}
// elements per lane and wavefront of the split dense layout (4 per row tile of P a wavefront can own): 16, 24 or 32 — whichever puts the FEWEST wavefronts on a
// tile (the smaller one on a tie): the fewest wavefronts that hold the tile measured fastest at every size (profiles/r6_dense_split.txt), as long as their
// registers are not short — so 257 <= D <= 384: 24 (4 wavefronts), 385 .. 512: 32 (4), 513 .. 768: 24 (8), 769 .. 1024: 32 (8; 24 there would be 12 wavefronts at
// 168 registers with scratch: measured slower than 16).  KLARA_SPLIT_NEW=16|24|32 forces one.
static int klara_split_new(int D, const KlaraOverrides& o)
{
    const int MT = (D + 15) / 16;
    if (o.split_new == 16 || o.split_new == 24 || o.split_new == 32) return o.split_new;
    int best = 16, wbest = 4 * ((MT + 15) / 16);
    for (int n = 24; n <= 32; n += 8) { const int w = 4 * ((MT + n - 1) / n); if (w < wbest && w <= 8) { best = n; wbest = w; } }
    return best;
}

// the logistic regression beyond the row-split kernels: more than 16 parameters, or more than 8 whose rows, padded to 16 columns, do not fit the LDS
static bool logit_beyond_rowsplit(const klara_desc& d) { return d.ndims > 16 || (d.ndims > 8 && (size_t)d.logit_ndata * 17 > KLARA_LOGIT_MAX_LDS_DOUBLES); }
// ... on the matrix cores (klara_logit_mfma.h, layout kind 5): X p and X' (y - 1/(1+exp(-Xp))) of 16 chains per wavefront as two MFMA passes over
// streamed fragments of X; every sampler, every tuner, the monitors of the dense layouts.  A job with the likelihood / prior history is refused
// (klara_plan_job; only a likelihood + prior user target has the two parts).
static bool logit_mfma_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    // (the kernels address the fragment stream with 32-bit byte offsets: 2 x 16 ceil(n / 16) x 4 NE doubles stay below 2 GB — 2 million rows at 128 parameters)
    const size_t stream_bytes = 2 * 16 * (((size_t)d.logit_ndata + 31) / 32 * 2) * 4 * (8 * (((size_t)d.ndims + 31) / 32)) * sizeof(double);
    if (stream_bytes >= ((size_t)1 << 31)) return false;
    return d.target == KLARA_TARGET_LOGISTIC && logit_beyond_rowsplit(d) && d.ndims <= 256 && d.logit_ndata >= 1 &&
           !(d.monitor & KLARA_MON_HIST_LLLP) && !o.logit_no_mfma;
}

// SMMALA (KLARA_SAMPLER_SMMALA), D <= 8 on the group layout (E = 2 / 4 / 8): the logistic target (kinds 0 / 2) and a user-defined target in the
// plain whole-vector form, one chain per lane, whose source defines klara_user_tensorlogtarget (the likelihood + prior form and pair closures are not taken)
static bool smmala_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    if (d.target == KLARA_TARGET_LOGISTIC) return d.ndims <= 8 && !logit_mfma_eligible(d, o);
    return d.ndims <= 8 && d.target == KLARA_TARGET_CUSTOM && d.custom_src != nullptr && !pair_source(d.custom_src) && !custom_lik_prior(d.custom_src);
}

// RAM (KLARA_SAMPLER_RAM), D <= 8 on the group layout (E = 2 / 4 / 8), one chain per lane: the logistic target (kinds 0 / 2, never the matrix cores) and a
// user-defined target as a whole-vector closure (plain or likelihood + prior form; pair closures are not taken).  No gradient is evaluated.
static bool ram_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    if (d.ndims > 8) return false;
    if (d.target == KLARA_TARGET_LOGISTIC) return !logit_mfma_eligible(d, o);
    return d.target == KLARA_TARGET_CUSTOM && d.custom_src != nullptr && strstr(d.custom_src, "KLARA_USER_PAIR_TARGET") == nullptr;
}

// AM (KLARA_SAMPLER_AM): RAM's scope — its covariance and running means are per-chain register state of the same kernels
static bool am_eligible(const klara_desc& d, const KlaraOverrides& o) { return ram_eligible(d, o); }

// AMWG (KLARA_SAMPLER_AMWG), one chain per lane, its 2 D scales and counts in registers: the logistic target wherever MH's row-split kernels serve it (up to 16
// parameters whose rows fit the LDS, kinds 0 / 2, never the matrix cores) and a user-defined target as a whole-vector closure with D <= 32 (plain,
// likelihood + prior and autodiff forms; pair closures and, beyond 32 dimensions, staged closures are not taken).  No gradient is evaluated.
static bool amwg_eligible(const klara_desc& d, const KlaraOverrides& o)
{
    if (d.target == KLARA_TARGET_LOGISTIC) return !logit_mfma_eligible(d, o) && !logit_beyond_rowsplit(d);
    return d.ndims <= 32 && d.target == KLARA_TARGET_CUSTOM && d.custom_src != nullptr && strstr(d.custom_src, "KLARA_USER_PAIR_TARGET") == nullptr;
}

// MH(Σ) (KLARA_SAMPLER_MH_COV), one chain per lane, the job's factor read as scalars: AMWG's scope
static bool mhcov_eligible(const klara_desc& d, const KlaraOverrides& o) { return amwg_eligible(d, o); }

// kind, G, E (and a staged closure's wavefronts per workgroup) of the job as it runs (a closure-form rewrite has made it a user-defined target)
static klara_status select_layout(const klara_desc& d, const KlaraOverrides& o, KlaraPlan& p)
{
    const int D = d.ndims;
    if (logit_mfma_eligible(d, o)) { p.kind = 5; p.G = 4; p.E = 8 * ((D + 31) / 32); return KLARA_OK; }
    if (hiert_eligible(d, o)) { p.kind = 4; p.G = 8; p.E = 8; return KLARA_OK; }
    if (dense_split(d, o)) {
        // W = G wavefronts per tile of 16 chains: whole SIMD rounds, at most NEW / 4 row tiles of P each (KLARA_SPLIT_W: more wavefronts, fewer tiles each)
        p.kind = 6; p.E = klara_split_new(D, o);
        const int w = 4 * (((D + 15) / 16 + p.E - 1) / p.E), v = o.split_w;
        p.G = v >= w && v <= 16 && v % 4 == 0 ? v : w;
        return KLARA_OK;
    }
    if (d.target == KLARA_TARGET_GAUSS_DENSE) {
        p.kind = 1; p.G = 4;
        if (D <= 32) p.E = 8; else if (D <= 64) p.E = 16; else if (D <= 100) p.E = 25; else if (D <= 128) p.E = 32;
        else if (dense_streamed(d, o)) p.E = 8 * ((D + 31) / 32);       // HMC to D = 256 (NE = 40, 48, 56, 64): P streamed from memory, momentum in LDS (klara_dense_big.h)
        else return KLARA_ERR_UNSUPPORTED;
        return KLARA_OK;
    }
    p.kind = 0;
    if (p.jit_pair) {
        // pair closure (klara_diagt.h USERPAIR): the pair-transposed layout, Q = 8 / 16 / 32 / 64 lanes per chain
        if (D < 17 || D > 2 * 64 * KLARA_DIAGT_NP_MAX) return KLARA_ERR_UNSUPPORTED;       // (fewer than 9 pairs: the whole-vector form)
        const int Q = diagt_lanes(D);
        p.kind = 3; p.G = Q; p.E = 2 * ((D + 2 * Q - 1) / (2 * Q));
        return KLARA_OK;
    }
    if (d.target == KLARA_TARGET_CUSTOM) {       // whole-vector closure: one chain per lane, or staged through LDS on G lanes (klara_custom.h)
        if (D > KLARA_CUSTOM_MAXD) return KLARA_ERR_UNSUPPORTED;
        custom_layout(D, p.custom_lanes, p.custom_rows, o, &p.G, &p.E, &p.custom_wpb);
        return KLARA_OK;
    }
    if (d.target == KLARA_TARGET_LOGISTIC) {
        p.G = 1;   // every lane holds the whole parameter vector; klara_plan_job may turn on the row split (kind 2)
        if (D <= 2) p.E = 2; else if (D <= 4) p.E = 4; else if (D <= 8) p.E = 8; else if (D <= 16) p.E = 16; else return KLARA_ERR_UNSUPPORTED;
        return KLARA_OK;
    }
    // diagonal Gaussian: the pair-transposed layout (klara_diagt.h), Q lanes per chain, NP element pairs per lane — the summation order
    // klara_get_layout reports.  (Untuned MH / MALA up to D = 104 also run on 4-lane kernels that reproduce the 8-lane order: q4_eligible.)
    if (diagt_eligible(d, o)) {
        const int Q = diagt_lanes(D);
        const int np = (D + 2 * Q - 1) / (2 * Q);                                 // NP = ceil(D/2 / Q) exactly (see klara_diagt.h)
        if (np >= 2 && np <= KLARA_DIAGT_NP_MAX) { p.kind = 3; p.G = Q; p.E = 2 * np; return KLARA_OK; }
    }
    // diagonal Gaussian: E elements per lane, G lanes; optional override for layout experiments
    // D <= 128: E = 2 or 4, whichever wastes fewer lanes; on a tie E = 4 (twice the chains per wavefront
    // amortise the per-wave fixed work — measured 80 us vs 90 us per launch at D = 100, 65,536 chains)
    int e = (D <= 256) ? 4 : (D <= 512) ? 8 : 0;
    if (D <= 128 && pow2ceil((D + 1) / 2) * 2 < pow2ceil((D + 3) / 4) * 4) e = 2;
    const int v = o.layout_e;
    if (o.layout_e_set && (v == 2 || v == 4 || v == 8) && (D + v - 1) / v <= 64) e = v;
    if (e == 0 || (d.target == KLARA_TARGET_HIER_NORMAL && e > 4)) return KLARA_ERR_UNSUPPORTED;
    p.E = e; p.G = pow2ceil((D + e - 1) / e);
    return KLARA_OK;
}

// Plans the job of a validated descriptor: the closure form it runs in, its layout, kernels, grids and LDS, and its launch length.  The launch
// length is planned first, so that a job klara_create refuses (any status but KLARA_OK) still has one (klara_selftest_plan).
static klara_status klara_plan_job(const klara_desc& desc, const KlaraOverrides& o, KlaraPlan* out)
{
    KlaraPlan& p = *out;
    p = KlaraPlan();
    klara_desc d = desc;
    p.cov = (d.monitor & KLARA_MON_COVARIANCE) != 0;
    d.monitor &= ~(uint32_t)KLARA_MON_COVARIANCE;                // (a consumer's flag: the kernels and the run-time compiler never see it)
    if (d.acov_maxlag > 0 || p.cov || d.marg_nbins > 0 || d.derived_nout > 0) d.monitor |= KLARA_MON_HISTORY;       // (the streaming autocovariances and the pooled covariance keep values: klara_create turns the value history on)
    const int D = d.ndims;
    p.plain = !cnt_predicate(d) && d.tuner_mode == KLARA_TUNE_PER_CHAIN && d.tuner != KLARA_TUNER_DUAL_AVERAGING;
    // plain and nothing monitored -> MODE 3 and its one-transition-per-launch form 7; plain -> 1; general -> 0
    if (p.plain && d.monitor == 0) { p.modes[0] = 3; p.modes[1] = 7; p.nmodes = 2; }
    else p.modes[0] = p.plain ? 1 : 0;
    p.slice_free = slice_free_eligible(d, o, p.plain);
    p.slice_machines = o.slice_machines;
    p.steps_per_launch = d.steps_per_launch > 0 ? d.steps_per_launch : p.slice_free ? KLARA_DEFAULT_STEPS_PER_LAUNCH_SLICE : KLARA_DEFAULT_STEPS_PER_LAUNCH;
    if (p.cov && D > KLARA_COV_MAX_DIMS) return KLARA_ERR_UNSUPPORTED;

    if (d.sampler == KLARA_SAMPLER_SMMALA && !smmala_eligible(d, o)) return KLARA_ERR_UNSUPPORTED;
    if (d.sampler == KLARA_SAMPLER_RAM && !ram_eligible(d, o)) return KLARA_ERR_UNSUPPORTED;
    if (d.sampler == KLARA_SAMPLER_AM && !am_eligible(d, o)) return KLARA_ERR_UNSUPPORTED;
    if (d.sampler == KLARA_SAMPLER_AMWG && !amwg_eligible(d, o)) return KLARA_ERR_UNSUPPORTED;
    if (d.sampler == KLARA_SAMPLER_MH_COV && !mhcov_eligible(d, o)) return KLARA_ERR_UNSUPPORTED;
    if (custom_autodiff(d) > 0 && d.custom_src != nullptr && strstr(d.custom_src, "KLARA_USER_PAIR_TARGET") != nullptr) return KLARA_ERR_UNSUPPORTED;
    if (d.target == KLARA_TARGET_LOGISTIC && !logit_mfma_eligible(d, o) && logit_beyond_rowsplit(d)) p.rewrite = KLARA_REWRITE_LOGIT_WIDE;
    else if (pair_as_whole(d, o)) p.rewrite = KLARA_REWRITE_PAIR_AS_WHOLE;
    else if (d.target == KLARA_TARGET_GAUSS_DENSE && D > 128 && !dense_streamed(d, o) && !dense_split(d, o)) p.rewrite = KLARA_REWRITE_DENSE_WIDE;
    if (p.rewrite == KLARA_REWRITE_LOGIT_WIDE || p.rewrite == KLARA_REWRITE_DENSE_WIDE) {
        if (D > KLARA_CUSTOM_MAXD || (d.monitor & KLARA_MON_HIST_LLLP)) return KLARA_ERR_UNSUPPORTED;
        d.target = KLARA_TARGET_CUSTOM; d.custom_src = "";      // (the library's closures: neither pair nor likelihood + prior form)
        p.custom_lanes = 1;                                     // (one chain per lane: an evaluation costs O(n D) / O(D^2))
    }
    p.jit_pair = p.rewrite == KLARA_REWRITE_NONE && pair_form(d);
    p.custom_rows = d.target == KLARA_TARGET_CUSTOM && custom_lik_prior(d.custom_src) ? 3 : 2;
    klara_status st = select_layout(d, o, p);
    if (st != KLARA_OK) return st;
    if (d.tuner_mode == KLARA_TUNE_POOLED && d.sampler == KLARA_SAMPLER_SLICE) return KLARA_ERR_UNSUPPORTED;
    if (d.sampler == KLARA_SAMPLER_SMMALA && p.G != 1) return KLARA_ERR_UNSUPPORTED;     // (one chain per lane: KLARA_CUSTOM_LANES may ask for more)
    if ((d.sampler == KLARA_SAMPLER_RAM || d.sampler == KLARA_SAMPLER_AM || d.sampler == KLARA_SAMPLER_AMWG || d.sampler == KLARA_SAMPLER_MH_COV) && (p.G != 1 || p.kind == 5)) return KLARA_ERR_UNSUPPORTED;
    // the logistic kernels keep the data rows (padded to E columns, + the responses) in LDS next to the 8 KB of math tables: up to
    // 144 KB of the CU's 160 (swiss: 200 x 5 doubles = 8 KB); beyond the 56 KB a launch gets by default the launchers raise the
    // kernel's limit, and fewer workgroups share a CU
    const bool logit_rows = d.target == KLARA_TARGET_LOGISTIC && p.kind != 5;
    if (logit_rows && (size_t)d.logit_ndata * (size_t)(p.E + 1) > KLARA_LOGIT_MAX_LDS_DOUBLES) return KLARA_ERR_UNSUPPORTED;
    if (logit_rows) {
        // D <= 8 parameters cannot fill a wavefront's lanes usefully, the ndata-row likelihood can: RS lanes share a chain
        // and each takes every RS-th row (fixed by ndata alone, so results do not depend on how chains are sharded)
        // 4 lanes from 64 rows on (round 4; rounds 1-3: 8 from 128 rows).  With the rows of an evaluation going through their stages in batches
        // a wavefront no longer needs partners to cover its LDS round trips, so the kernels run at 2 wavefronts per SIMD with the registers
        // of a 4-row batch, and 16 chains per wavefront share the sampler's per-wavefront work instead of 8: swiss (200 rows), 32,768 chains,
        // same box, running sums on: 2.10e9 transitions/s at 4 lanes against 1.88e9 at 8 (gpurun_out/r4_gpu3/ab_logit.txt; profiles/README.md)
        const int v = o.logit_rowsplit;
        p.RS = (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) ? v : d.logit_ndata >= 64 ? 4 : 1;
        if (p.RS > 1) p.kind = 2;
    }
    if (p.kind == 3) {
        p.q4_ok = q4_eligible(d, o, p.plain); p.np4 = (D + 7) / 8;
        const long long cpw = p.q4_ok ? 16 : 64 / p.G, groups = (d.nchains + cpw - 1) / cpw;
        int np = groups >= 4096 ? 2 : 1;                       // >= one full round of wavefronts (4 per SIMD) per partition
        if (d.nstreams >= 1 && d.nstreams <= 4) np = d.nstreams;
        if (d.tuner_mode == KLARA_TUNE_POOLED) np = 1;         // the pooled tuner update sits between launches, on one stream
        if (d.acov_maxlag > 0 || p.cov || d.marg_nbins > 0 || d.derived_nout > 0) np = 1;                // ... and so does the consumer of the launch's saved samples
        if (np > groups) np = (int)groups;
        p.nparts = np;
        // which kernel family runs a launch (q4_ok jobs: same bits either way); with running sums and no klara_desc.sparse_moves, the device decides
        const bool sums = (d.monitor & KLARA_MON_SUMMARIES) != 0;
        p.family = !p.q4_ok ? 1 : !sums ? 0 : d.sparse_moves == 1 ? 0 : d.sparse_moves == 2 ? 1 : -1;
        if (o.auto_threshold_set) p.auto_threshold = o.auto_threshold;
    }
    if (p.kind == 6) {
        // a workgroup's LDS: xb (4 MT rows of 64 doubles) + the partial sums of its W = G wavefronts (the 8 KB of detmath tables are static); registers for as
        // many wavefronts per SIMD as the LDS lets a compute unit hold (160 KB, 8 KB of them the detmath tables of every workgroup): W = 4: three workgroups
        // = 3 per SIMD (168 registers); W = 8: two = 4 (128); W = 12: one = 3; W = 16: one = 4; a lone workgroup of 8, or two of 4: 2 (256)
        p.lds = sizeof(double) * (4 * (((size_t)D + 15) / 16) * 64 + 2 * 3 * (size_t)p.G * 16);
        const int nwg = std::max(1, (int)((size_t)160 * 1024 / (p.lds + 8192)));
        p.split_mw = std::min(4, std::max(2, (nwg * p.G + 3) / 4));
        if (o.split_mw >= 2 && o.split_mw <= 4 && 4 * o.split_mw >= p.G) p.split_mw = o.split_mw;
    } else if (logit_rows) {        // data rows + responses + the kernel's copy of kd_log12's table (LogisticTarget::lds_bytes)
        p.lds = sizeof(double) * (((size_t)d.logit_ndata * (size_t)(p.E + 1) + 1) / 2 * 2 + 256);
    } else if (p.kind == 0 && d.target == KLARA_TARGET_CUSTOM && p.G > 1) {  // staged closure: the rows of a workgroup's chains
        p.lds = custom_stage_bytes(D, p.G, p.custom_rows, p.custom_wpb);
    }
    // init kernels and the MFMA / kind 3-6 kernels: one wavefront per chain group, workgroups of wpb (kind 6: one workgroup of G wavefronts per tile of 16 chains)
    const long long cpw = (p.kind == 1 || p.kind == 5) ? 16 : 64 / (p.G * p.RS), waves = (d.nchains + cpw - 1) / cpw;
    const long long wpb = p.kind == 5 ? 4 : p.kind == 1 ? (p.E > 32 ? 4 : 8) : p.custom_wpb;      // (streamed layouts: one wavefront per SIMD, workgroups of 4)
    p.grid_init = (unsigned)(p.kind == 6 ? (d.nchains + 15) / 16 : (waves + wpb - 1) / wpb);
    // group-layout transition kernels are persistent over `groups_per_wave` chain groups (prefetch of the
    // next group's state overlaps the current group's compute); keep >= ~8 waves per SIMD of work for balance
    const long long gcpw = 64 / (p.G * p.RS), groups = (d.nchains + gcpw - 1) / gcpw;
    long long gpw = 4;
    while (gpw > 1 && groups / gpw < 8192) gpw >>= 1;
    if (o.groups_per_wave >= 1 && o.groups_per_wave <= 1024) gpw = o.groups_per_wave;
    p.groups_per_wave = gpw;
    p.grid_steps = (unsigned)(((groups + gpw - 1) / gpw + p.custom_wpb - 1) / p.custom_wpb);
    return KLARA_OK;
}
