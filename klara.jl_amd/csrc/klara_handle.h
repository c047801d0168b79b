// klara_handle.h — internal, host only: the handle behind the C ABI, the owner of its device arrays, and the functions the host translation
// units share (klara_devmem / klara_create / klara_run / klara_monitors / klara_comm / klara_zv_api / klara_selftest .hip).
// The ABI and the reference lines each entry point replaces are documented in include/klara_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "klara_plan.h"
#include "klara_cov.h"
#include "klara_marg.h"
#include "klara_derived.h"

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) return (e__ == hipErrorOutOfMemory) ? KLARA_ERR_NOMEM : KLARA_ERR_HIP; \
    } while (0)
#define KCHK(expr) do { const klara_status s__ = (expr); if (s__ != KLARA_OK) return s__; } while (0)

#pragma GCC visibility push(hidden)     // (shared between the library's own translation units, not exported)

// ---- klara_devmem.hip: device allocations, between canaries under KLARA_DEBUG_CANARY=1
hipError_t dalloc_bytes(void** p, size_t bytes);
bool dfree(void* p);                    // false when the array's canaries were found damaged (always true without KLARA_DEBUG_CANARY)
template <class T>
static hipError_t dalloc(T** p, size_t n) { return dalloc_bytes((void**)p, n * sizeof(T)); }

// The device arrays of one handle, or of one call's workspace: what alloc() hands out, release() frees — and checks: an array that is not
// in this list would neither be freed nor have its canaries looked at.
struct DeviceArrays {
    std::vector<void*> owned;
    template <class T>
    hipError_t alloc(T** p, size_t n)
    {
        const hipError_t e = dalloc(p, n);
        if (e == hipSuccess) owned.push_back(*p);
        return e;
    }
    bool release()                      // false: a kernel wrote outside one of the arrays (KLARA_DEBUG_CANARY=1)
    {
        bool ok = true;
        for (void* p : owned) ok &= dfree(p);
        owned.clear();
        return ok;
    }
};

struct klara_handle {
    klara_desc d;
    KlaraPlan plan;            // layout, kernels, grids and LDS of the job, planned once by klara_create (klara_plan.h)
    DeviceArrays mem;          // owns every device array below; the typed pointers are what the kernels' parameter block is filled from
    double *X = nullptr, *GR = nullptr, *LT = nullptr;
    double* tune_step = nullptr;
    long long *tune_acc = nullptr, *tune_prop = nullptr, *tune_tot = nullptr;
    double *da_epsbar = nullptr, *da_hbar = nullptr;
    unsigned long long* pooled_acc = nullptr;
    uint8_t* accept = nullptr; long long accept_cap = 0;
    unsigned long long* naccept = nullptr;
    double *sum = nullptr, *sumsq = nullptr;
    long long* held = nullptr;      // running sums in sojourn form: saved steps at the current state not yet in sum / sumsq (KParams::held)
    double* hist = nullptr; long long hist_cols = 0;     // hist_cols: columns of the history buffers (= ring when > 0 and ring is set)
    bool ring = false;                                   // the history buffers hold the last hist_cols saved steps only
    // streaming autocovariances (acov_maxlag > 0): W = maxlag + 1 lags; [k][series] layouts
    int acov_W = 0; double *acov_S = nullptr, *acov_head = nullptr, *acov_tail = nullptr, *acov_total = nullptr, *acov_near = nullptr; long long acov_n = 0;
    // pooled covariance (KLARA_MON_COVARIANCE, klara_cov.h): the slabs' cross-products and sums, the pivot, the finalized mean | M; saved steps consumed
    KCovGeom cov = {}; double *cov_S = nullptr, *cov_T = nullptr, *cov_pivot = nullptr, *cov_out = nullptr; long long cov_n = 0;
    // pooled marginal histograms (klara_desc.marg_nbins > 0, klara_marg.h): lo | hi | inv_w, the uint64 [D][nbins + 2] table; saved steps consumed
    KMargGeom marg = {}; double* marg_par = nullptr; unsigned long long* marg_counts = nullptr; long long marg_n = 0;
    std::vector<double> marg_host;  // lo | hi as given at create: what klara_gather_histogram compares between ranks
    // derived quantities (klara_desc.derived_nout > 0, klara_derived.h): the kernel compiled with the user's closure (a second run-time module beside `jit`), its
    // geometry and data block, the chains' sums [N][K]; N zeros that stand where the coordinate reductions read `held` and `naccept`; the reductions' workspaces
    // (moments: stage-1 partials and mean | M2 | accept word; R-hat: allocated at its first call); with derived_nbins > 0 the staging array [32][N][K], the
    // histogram's geometry over (N, K, nbins), lo | hi | inv_w, the uint64 [K][nbins + 2] table and lo | hi as given at create; saved steps consumed
    KlaraJit* der_jit = nullptr; KDerivedGeom der = {}; double* der_data = nullptr; long long der_ndata = 0;
    double *der_sum = nullptr, *der_sumsq = nullptr; long long* der_zero = nullptr;
    double *der_partial = nullptr, *der_out = nullptr, *der_rhat_ws = nullptr;
    double* der_stage = nullptr; KMargGeom der_marg = {}; double* der_marg_par = nullptr; unsigned long long* der_counts = nullptr;
    std::vector<double> der_marg_host; long long der_n = 0;
    double *hist_lt = nullptr, *hist_g = nullptr, *hist_ll = nullptr, *hist_lp = nullptr;
    unsigned long long* clock_probe = nullptr;        // pair-transposed kernels: (s_memtime, s_memrealtime) at the end / start of one workgroup of the last launch
    bool pair_enqueued = false;                       // a launch of this handle has enqueued both kernel families (their one-time scratch set-up is behind us)
    int* err = nullptr; int* flag_host = nullptr;     // error flag as the kernels address it; the same word as the host reads it (null: err is device memory)
    double *vecparam = nullptr, *gw = nullptr, *gmu = nullptr, *lX = nullptr, *ly = nullptr, *Pfrag = nullptr,
           *hY = nullptr, *hxc = nullptr;
    double* pooled_out = nullptr;   // 2*D doubles + 1 u64 scratch for pooled summaries
    double* pool_partial = nullptr; // KLARA_POOL_BLOCKS x (2 D doubles + 1 u64): stage-1 partials of the pooled summaries
    double *rhat_ws = nullptr, *rhat_half = nullptr;   // klara_gather_rhat's workspace, allocated at its first call: stage-1 partials and the staging buffer; the halves' (mean, M2) of the split form
    double* ess_ws = nullptr;       // klara_gather_ess in streamed mode: its workspace and staging buffer, allocated at its first call (klara_ess.h)
    double* cdata = nullptr; KlaraJit* jit = nullptr;  // user-defined target: data block, run-time compiled kernels
    // RAM: the chains' factors (D (D + 1) / 2 planes of nchains doubles, KParams::ram_S), the packed lower triangle of klara_desc.ram_S0 they restart from, the skipped-update counter
    double *ram_S = nullptr, *ram_S0 = nullptr; unsigned long long* ram_skipped = nullptr;
    // AM: the chains' covariances (D (D + 1) / 2 planes, KParams::am_C), their running means (2 D planes, KParams::am_mean), the packed upper triangle of
    // klara_desc.am_C0 they restart from, the counter of transitions that fell back to the minor component
    double *am_C = nullptr, *am_C0 = nullptr, *am_mean = nullptr; unsigned long long* am_fallbacks = nullptr;
    // AMWG: the chains' log proposal scales, window counts and accepted proposals per coordinate (D planes of nchains each, KParams::amwg_*), the D scales of
    // klara_desc.amwg_logsigma0 they restart from, the coordinate masks of the transitions (KLARA_MON_ACCEPT: nsteps x nchains)
    double *amwg_logsig = nullptr, *amwg_logsig0 = nullptr; int* amwg_acc = nullptr; unsigned long long* amwg_nacc = nullptr; uint32_t* amwg_mask = nullptr;
    // MH(Σ) (KLARA_SAMPLER_MH_COV): the job's proposal factor as the kernels read it (KParams::mh_factor, KLARA_MHCOV_TRI doubles), and the packed triangle of
    // klara_desc.mh_factor that klara_reset puts back
    double* mh_factor = nullptr; std::vector<double> mh_factor0;
    // streaming batch means (bm_batchlen > 0): running sum at the last batch boundary, Welford mean / M2 of the batch means
    double *bm_prev = nullptr, *bm_mean = nullptr, *bm_m2 = nullptr; long long bm_count = 0;
    KParams* d_params = nullptr;    // device copy of the handle's static kernel parameters
    double lpconst = 0.0;
    bool dense_mu = false;          // dense target with a mean: Pfrag carries mu behind the matrix fragments
    int logit_nblocks = 0;          // layout kind 5 (klara_logit_mfma.h): row blocks of the fragment stream in Pfrag; ly holds the zero-padded responses
    // run state
    bool have_state = false;
    unsigned long long epoch = 0;   // klara_reset calls so far: the Philox key of the job is seed + epoch * KLARA_EPOCH_KEY_STRIDE
    long long steps_done = 0;       // transitions since set_state/reset (= global transition index)
    long long nsaved = 0;           // postrange steps passed so far
    // host mirror of the pooled tuner counters (decides where launches must end)
    long long m_prop = 0, m_tot = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr; long long last_launches = 0; bool timed = false;
    // layout kind 3: the chain groups are cut into plan.nparts contiguous partitions, partition j > 0 runs on its own
    // internal stream.  Chains are independent, so partition j's transition t+1 only follows its own transition t; the
    // streams drift apart and one partition's kernel fills the SIMDs while the other's drains / ramps up.
    hipStream_t side[3] = { nullptr, nullptr, nullptr }; hipEvent_t fork_ev = nullptr, join_ev[3] = { nullptr, nullptr, nullptr };
    // layout kind 3, untuned MH / MALA with 17 <= D <= 104: the 4-lanes-per-chain kernels are available as well (plan.np4 pairs per lane).
    // They sum in the 8-lane order, so which of the two kernel families runs a launch changes no bit; with running sums on, the
    // choice is taken on the device launch by launch (KAuto, klara_diagt.h): auto_cells = [partition][launch parity] decision,
    // auto_ctr = [partition] launch counter, auto_mirror = host-visible {mode, accepted} per partition (may be null).
    int* auto_cells = nullptr; unsigned long long* auto_ctr = nullptr; int* auto_mirror = nullptr; int* auto_mirror_dev = nullptr;
    long long launch_idx = 0;
    int query_lanes = 4;            // klara_get_kernel_attributes: which of the two kernel families to report
    long long n_launch_mode[3] = { 0, 0, 0 };   // launches issued as: forced / single 4-lane, forced / single 8-lane, device-decided pair
};

// ---- klara_create.hip
klara_status validate(const klara_desc* d);                 // every check a descriptor can fail without a device
std::string pair_as_whole_source(const char* src);
KParams make_params(klara_handle* h);
// MH(Σ): the D x D row-major factor L (its lower triangle) as KParams::mh_factor holds it — packed by rows, the rows from D on the identity's; false where a
// read entry is not finite or a diagonal entry is not positive
bool pack_mh_factor(const double* L, int D, std::vector<double>& tri);

// ---- klara_run.hip
void part_range(const klara_handle* h, int nparts, int j, long long* c0, long long* c1);
hipError_t launch_steps(klara_handle* h, const KLaunch& kl, int nparts);

// ---- klara_monitors.hip: what klara_run_async enqueues behind a launch, and the pooled sums the gather calls reduce over the ranks
hipError_t launch_bm_close(klara_handle* h, int nparts);
// streaming autocovariances on plain buffers (the job path and klara_selftest_chain_stats run the same kernels): columns [col0, col0 + m) of hist update
// S / head / tail ([W][nd]) and total ([nd]) after n_before samples (near: 32 nd scratch, W > 32 only); then Geyer's estimators from them
hipError_t launch_acov_update(hipStream_t stream, const double* hist, double* S, double* head, double* tail, double* near, double* total,
                              long long n_before, int W, long long nd, long long col0, long long m);
hipError_t launch_acov_finalize(hipStream_t stream, const double* S, const double* head, const double* tail, const double* total,
                                long long n, int W, long long nd, double* imse, double* ipse);
// the post-hoc estimators over a stored history (k_chain_stats), every output optional (device, N * D each)
hipError_t launch_chain_stats(hipStream_t stream, const double* hist, long long ncols, long long N, int D, long long batchlen, long long maxlag,
                              double* iid, double* bm, double* imse, double* ipse);
// the across-chain reductions on plain buffers (the job path and klara_selftest_pooled run the same kernels): sum / sumsq / X are N x D, held and
// naccept N, partial 1024 (2 D + 1) doubles of staging; out = 2 D doubles and the u64 accept total (sum, sumsq — untouched when sum is null — or mean, M2)
hipError_t pool_summaries_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held,
                                const unsigned long long* naccept, long long N, int D, double* partial, double* out);
hipError_t pool_moments_async(hipStream_t stream, const double* sum, const double* sumsq, const double* X, const long long* held,
                              const unsigned long long* naccept, long long N, int D, long long nsaved, double* partial, double* out);
hipError_t pool_summaries_async(klara_handle* h, bool with_sums, double* out);      // ... with the handle's arrays, on its stream
hipError_t pool_moments_async(klara_handle* h, double* out);

// ---- klara_derived.hip: the derived-quantity update on plain buffers (the job path and klara_selftest_derived run the same function): columns
// [col0, col0 + m) of hist through k_derived_update in pieces of at most KLARA_DERIVED_MAX_COLS; with a staging array each piece's outputs then go through
// klara_marg_launch_update (marg, par, counts; skipped when counts is null) and, when values_out is not null, to values_out + (piece's first column) N K
hipError_t klara_derived_launch_update(KlaraJit* jit, const KDerivedGeom& g, const double* hist, long long col0, long long m, const double* data, long long ndata,
                                       double* dsum, double* dsumsq, double* stage, const KMargGeom* marg, const double* par, unsigned long long* counts,
                                       double* values_out, hipStream_t st);

// ---- klara_comm.hip: the bodies of klara_gather_moments, klara_gather_rhat and klara_gather_histogram over arrays of any width W (the coordinates: W = ndims,
// the handle's own arrays; the derived quantities: W = derived_nout) — per-chain sums N x W, the state and sojourn counts the reductions read, workspaces
struct klara_comm;
klara_status gather_moments_arrays(klara_handle* h, klara_comm* c, int W, const double* sum, const double* sumsq, const double* X, const long long* held,
                                   const unsigned long long* naccept, long long nsaved, double* partial, double* out, double* mean, double* m2,
                                   uint64_t* nsamples, uint64_t* naccept_out, uint64_t* ntransitions, uint64_t* nchains);
klara_status gather_rhat_arrays(klara_handle* h, klara_comm* c, int32_t split, int W, const double* sum, const double* sumsq, const double* X,
                                const long long* held, long long nsaved, double** ws, double* rhat, double* mean, double* wsum, double* bsum, uint64_t* nchains, int64_t* nper);
klara_status gather_histogram_arrays(klara_handle* h, klara_comm* c, int W, const KMargGeom& geom, const unsigned long long* table, long long nsaved,
                                     const double* lohi, uint64_t* counts, uint64_t* nsamples, uint64_t* nchains);

// ---- klara_comm.hip: the between-rank merge of the pooled moments, the pooled covariance and R-hat — its staging layout, its rank-local steps and the one
// sequence of reductions that the gather calls and the simulated-rank self tests both run
#include "klara_merge.h"

#pragma GCC visibility pop
