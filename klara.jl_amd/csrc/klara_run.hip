// klara_run.hip — start states, the launch dispatcher, launch planning and klara_run.
#include "klara_handle.h"

// device-decided kernel choice (KAuto): launches shorter than this are issued as one kernel chosen on the host
#ifndef KLARA_AUTO_PAIR_MIN_STEPS
#define KLARA_AUTO_PAIR_MIN_STEPS 4
#endif

thread_local hipFuncAttributes* klara_attr_query = nullptr;     // see klara_launch.h klara_go

// ---- init kernels (group layout) instantiated here: E = 2 and 4 for every target, 8 for all but the hierarchical one, 16 for the logistic regression alone
template <int TARGET>
static hipError_t launch_init_t(const KParams& p, int E, int G, int needgrad, dim3 grid, size_t lds, hipStream_t st)
{
    const auto go = [&](auto e, auto g) { return klara_start(k_init<TARGET, decltype(e)::value, decltype(g)::value>, grid, dim3(256), lds, st, p, needgrad); };
    // (one chain per wavefront: diagonal-Gaussian jobs only — a run-time condition, so every target keeps the <2, 64> instantiation it has always had)
    if (E == 2 && G == 64 && TARGET == KLARA_TARGET_GAUSS_DIAG) return go(KInt<2>(), KInt<64>());
    const auto go0 = [&](auto e) { return go(e, KInt<0>()); };
    if constexpr (TARGET == KLARA_TARGET_HIER_NORMAL) return klara_pick<2, 4>(E, go0);
    else if constexpr (TARGET == KLARA_TARGET_LOGISTIC) return klara_pick<2, 4, 8, 16>(E, go0);
    else return klara_pick<2, 4, 8>(E, go0);
}

__global__ void k_fill_tune(double* step, long long* acc, long long* prop, long long* tot, long long n,
                            double step0, long long period)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { step[i] = step0; acc[i] = 0; prop[i] = 0; tot[i] = period; }
}

// The samplers' per-chain adaptive arrays are planes (plane k holds entry k of every chain): plane k of every chain <- entry k of a short vector.  RAM's
// factors restart from S0 (RAM.jl:155-162, 201-211), AM's covariances from C0 (AM.jl:238-246), AMWG's log proposal scales from logsigma0 (AMWG.jl:165-170)
__global__ void k_fill_planes(double* planes, const double* entries, long long n, int nplanes)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) for (int k = 0; k < nplanes; ++k) planes[(long long)k * n + i] = entries[k];
}

// AM: both running means restart from the chain's start value (AM.jl:292-304)
__global__ void k_fill_am_means(double* mean, const double* X, long long n, int D)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < D; ++k) { const double v = X[i * D + k]; mean[(long long)k * n + i] = v; mean[(long long)(D + k) * n + i] = v; }
}

__global__ void k_fill2(double* a, double* b, long long n, double va, double vb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { a[i] = va; b[i] = vb; }
}

// pooled tuner update after a launch of `k` transitions: tuners.jl:27-32, AcceptanceRateMCTuner.jl:46
// with the rate pooled over the GPU's chains (KLARA_TUNE_POOLED; SURVEY §7 hard part 5).
__global__ void k_pooled_tune(KParams p, int k)
{
    kd_tables_to_lds();            // rate_score -> kd_exp reads its table from LDS
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!p.cnt) return;
    long long prop = p.tune_proposed[0] + k;
    long long acc = p.tune_accepted[0] + (long long)(*p.pooled_accepted);
    long long tot = p.tune_totproposed[0];
    double step = p.tune_step[0];
    *p.pooled_accepted = 0ull;
    if (tot <= p.burnin && (prop % p.period) == 0) {
        const double rate = (double)acc / (double)(prop * p.nchains);
        if (p.tuner == KLARA_TUNER_ACCEPT_RATE && !p.is_mh) {
            const double xr = rate - p.targetrate;
            step *= rate_score(p, xr);
        }
        tot += prop; acc = 0; prop = 0;
    }
    p.tune_step[0] = step; p.tune_accepted[0] = acc; p.tune_proposed[0] = prop; p.tune_totproposed[0] = tot;
}

// ---- the pair-transposed kernels' launchers (layout kind 3; klara_diagt_*.hip, built once per lane count): one table entry per lanes-per-chain;
// the 4-lane build has the MH / MALA / HMC and init kernels only
struct DiagtLaunchers {
    using Step = hipError_t (*)(const KParams*, const KLaunch&, int, bool, bool, bool, bool, bool, const KAuto&, long long, hipStream_t);
    Step mh, mala, hmc;
    hipError_t (*slice)(const KParams*, const KLaunch&, int, bool, bool, bool, const KAuto&, long long, hipStream_t);
    hipError_t (*slice_free)(const KParams*, const KLaunch&, int, bool, bool, const KAuto&, long long, int, hipStream_t);
    hipError_t (*hist_lt)(const KParams*, const KLaunch&, int, bool, long long, int, long long, hipStream_t);
    hipError_t (*init)(const KParams&, int, int, dim3, hipStream_t);
};
#define KLARA_DIAGT_ROW(SUFFIX) { klara_launch_diagt_mh##SUFFIX, klara_launch_diagt_mala##SUFFIX, klara_launch_diagt_hmc##SUFFIX, klara_launch_diagt_slice##SUFFIX, \
                                  klara_launch_diagt_slice_free##SUFFIX, klara_launch_diagt_hist_lt##SUFFIX, klara_launch_diagt_init##SUFFIX }
static const DiagtLaunchers diagt_table[5] = {
    { klara_launch_diagt_mh_q4, klara_launch_diagt_mala_q4, klara_launch_diagt_hmc_q4, nullptr, nullptr, nullptr, klara_launch_diagt_init_q4 },
    KLARA_DIAGT_ROW(), KLARA_DIAGT_ROW(_q16), KLARA_DIAGT_ROW(_q32), KLARA_DIAGT_ROW(_q64) };
#undef KLARA_DIAGT_ROW
static const DiagtLaunchers& diagt_launchers(int lanes) { return diagt_table[lanes == 4 ? 0 : lanes == 8 ? 1 : lanes == 16 ? 2 : lanes == 32 ? 3 : 4]; }

// waits for the handle's stream and reads the kernels' error flag: they store into a word of host memory themselves, or it is copied behind them
static klara_status sync_read_flag(klara_handle* h, int* flag)
{
    if (!h->flag_host) HIPCHK(hipMemcpyAsync(flag, h->err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->flag_host) *flag = __atomic_load_n(h->flag_host, __ATOMIC_ACQUIRE);
    return KLARA_OK;
}

static klara_status init_common(klara_handle* h)
{
    const klara_desc& d = h->d;
    const size_t N = (size_t)d.nchains, D = (size_t)d.ndims;
    const bool pooled = d.tuner_mode == KLARA_TUNE_POOLED;
    const long long NT = pooled ? 1 : (long long)N;
    hipStream_t st = h->stream;
    HIPCHK(hipMemsetAsync(h->err, 0, sizeof(int), st));
    HIPCHK(hipMemsetAsync(h->naccept, 0, N * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(h->pooled_acc, 0, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(h->GR, 0, N * D * sizeof(double), st));
    if (h->sum) {
        HIPCHK(hipMemsetAsync(h->sum, 0, N * D * sizeof(double), st)); HIPCHK(hipMemsetAsync(h->sumsq, 0, N * D * sizeof(double), st));
        HIPCHK(hipMemsetAsync(h->held, 0, N * sizeof(long long), st));
    }
    if (h->bm_prev) {
        HIPCHK(hipMemsetAsync(h->bm_prev, 0, N * D * sizeof(double), st)); HIPCHK(hipMemsetAsync(h->bm_mean, 0, N * D * sizeof(double), st));
        HIPCHK(hipMemsetAsync(h->bm_m2, 0, N * D * sizeof(double), st));
    }
    h->bm_count = 0;
    if (h->auto_cells) {             // first launch of a job: resident sums (flat cost whatever the acceptance turns out to be)
        const int ones[8] = { 1, 1, 1, 1, 1, 1, 1, 1 };
        HIPCHK(hipMemcpyAsync(h->auto_cells, ones, sizeof(ones), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(h->auto_ctr, 0, 4 * sizeof(unsigned long long), st));
    }
    if (h->acov_S) {
        const size_t ws = (size_t)h->acov_W * N * D * sizeof(double);
        HIPCHK(hipMemsetAsync(h->acov_S, 0, ws, st)); HIPCHK(hipMemsetAsync(h->acov_head, 0, ws, st)); HIPCHK(hipMemsetAsync(h->acov_tail, 0, ws, st));
        HIPCHK(hipMemsetAsync(h->acov_total, 0, N * D * sizeof(double), st));
    }
    h->acov_n = 0;
    if (h->cov_S) {
        HIPCHK(hipMemsetAsync(h->cov_S, 0, klara_cov_S_elems(h->cov) * sizeof(double), st)); HIPCHK(hipMemsetAsync(h->cov_T, 0, klara_cov_T_elems(h->cov) * sizeof(double), st));
        HIPCHK(hipMemsetAsync(h->cov_pivot, 0, D * sizeof(double), st));
    }
    h->cov_n = 0;
    if (h->marg_counts) HIPCHK(hipMemsetAsync(h->marg_counts, 0, klara_marg_count_elems(h->marg) * sizeof(unsigned long long), st));
    h->marg_n = 0;
    if (h->der_sum) {
        const size_t NK = N * (size_t)h->der.K * sizeof(double);
        HIPCHK(hipMemsetAsync(h->der_sum, 0, NK, st)); HIPCHK(hipMemsetAsync(h->der_sumsq, 0, NK, st));
        if (h->der_counts) HIPCHK(hipMemsetAsync(h->der_counts, 0, klara_marg_count_elems(h->der_marg) * sizeof(unsigned long long), st));
    }
    h->der_n = 0;
    // tuner_state: samplers.jl:29-45 — step per sampler, accepted = proposed = 0, totproposed = period
    const double step0 = sampler_step0(d);
    hipLaunchKernelGGL(k_fill_tune, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, st, h->tune_step,
                       h->tune_acc, h->tune_prop, h->tune_tot, NT, step0, (long long)d.period);
    HIPCHK(hipGetLastError());
    if (h->da_epsbar) {
        hipLaunchKernelGGL(k_fill2, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, st, h->da_epsbar, h->da_hbar, NT,
                           d.da_eps0bar, d.da_h0bar);
        HIPCHK(hipGetLastError());
    }
    const dim3 fill_grid((unsigned)((N + 255) / 256));
    if (h->ram_S) {
        hipLaunchKernelGGL(k_fill_planes, fill_grid, dim3(256), 0, st, h->ram_S, h->ram_S0, (long long)N, (int)(D * (D + 1) / 2));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(h->ram_skipped, 0, sizeof(unsigned long long), st));
    }
    if (h->am_C) {
        hipLaunchKernelGGL(k_fill_planes, fill_grid, dim3(256), 0, st, h->am_C, h->am_C0, (long long)N, (int)(D * (D + 1) / 2));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_fill_am_means, fill_grid, dim3(256), 0, st, h->am_mean, h->X, (long long)N, (int)D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(h->am_fallbacks, 0, sizeof(unsigned long long), st));
    }
    if (h->amwg_logsig) {                // (the counts restart from zero: AMWG.jl:205-214)
        hipLaunchKernelGGL(k_fill_planes, fill_grid, dim3(256), 0, st, h->amwg_logsig, h->amwg_logsig0, (long long)N, (int)D);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(h->amwg_acc, 0, N * D * sizeof(int), st));
        HIPCHK(hipMemsetAsync(h->amwg_nacc, 0, N * D * sizeof(unsigned long long), st));
    }
    const int needgrad = sampler_needs_gradient(d.sampler);
    KParams p = make_params(h);
    const KlaraPlan& P = h->plan;
    const dim3 grid(P.grid_init);
    hipError_t e;
    if (P.kind == 1) e = klara_launch_dense_init(p, P.E, h->Pfrag, h->dense_mu, needgrad, grid, st);
    else if (P.kind == 5) e = klara_launch_logit_mfma_init(p, P.E, h->Pfrag, h->ly, h->logit_nblocks, needgrad, grid, st);
    else if (P.kind == 6) e = klara_launch_dense_split_init(p, P.G, P.E, P.lds, h->Pfrag, h->dense_mu, needgrad, grid, st);
    else if (P.kind == 3 && P.jit_pair) e = klara_jit_launch_init(h->jit, p, needgrad, grid, 0, st);
    else if (P.kind == 3) e = diagt_launchers(P.G).init(p, P.E / 2, needgrad, grid, st);
    else if (P.kind == 4) e = klara_launch_hiert_init(p, P.E / 2, d.hier_ntimes, needgrad, grid, st);
    else if (d.sampler == KLARA_SAMPLER_SMMALA && d.target == KLARA_TARGET_LOGISTIC) e = klara_launch_smmala_init(p, P.E, grid, P.lds, st);
    else if (d.target == KLARA_TARGET_CUSTOM) e = klara_jit_launch_init(h->jit, p, needgrad, grid, P.lds, st, 64 * P.custom_wpb);
    else if (d.target == KLARA_TARGET_GAUSS_DIAG)
        e = launch_init_t<KLARA_TARGET_GAUSS_DIAG>(p, P.E, P.G, needgrad, grid, P.lds, st);
    else if (d.target == KLARA_TARGET_HIER_NORMAL)
        e = launch_init_t<KLARA_TARGET_HIER_NORMAL>(p, P.E, P.G, needgrad, grid, P.lds, st);
    else e = launch_init_t<KLARA_TARGET_LOGISTIC>(p, P.E, P.G, needgrad, grid, P.lds, st);
    HIPCHK(e);
    int flag = 0;
    KCHK(sync_read_flag(h, &flag));
    // (host mirror of the decision cells, written once nothing is in flight)
    if (h->auto_mirror) for (int i = 0; i < 16; ++i) h->auto_mirror[i] = (i & 3) == 0 ? 1 : ((i & 3) == 2 ? (int)(h->launch_idx - 1) : 0);
    h->steps_done = 0; h->nsaved = 0; h->m_prop = 0; h->m_tot = d.period; h->timed = false;
    if (flag != 0) { h->have_state = false; return (klara_status)flag; }
    h->have_state = true;
    return KLARA_OK;
}

extern "C" klara_status klara_set_state(klara_handle* h, const double* x_host)
{
    if (!h || !x_host) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    const size_t n = (size_t)h->d.nchains * (size_t)h->d.ndims;
    HIPCHK(hipMemcpyAsync(h->X, x_host, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return init_common(h);
}

extern "C" klara_status klara_init_state_normal(klara_handle* h)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    // the stream is layout-free (element i <- slot i>>1), so any group layout draws the same x0:
    // use the handle's own (kind 0) or a group layout that fits the wavefront for the other kinds
    KParams p = make_params(h);
    const int D = h->d.ndims;
    int E = D <= 128 ? 2 : (D <= 256 ? 4 : (D <= 512 ? 8 : 16)), G = pow2ceil((D + E - 1) / E);       // (at most 64 lanes per chain: D <= 1024)
    if ((h->plan.kind == 0 || h->plan.kind == 2) && h->d.target != KLARA_TARGET_CUSTOM) { E = h->plan.E; G = h->plan.G; }
    p.G = G; p.rs = 1;     // the init stream is drawn without the row split (same values, any layout)
    const long long cpw = 64 / G, waves = (h->d.nchains + cpw - 1) / cpw;
    const dim3 grid((unsigned)((waves + 3) / 4)), blk(256);
    const hipError_t e0 = klara_pick<2, 4, 8, 16>(E, [&](auto e) { return klara_start(k_init_normal<decltype(e)::value, 0>, grid, blk, 0, h->stream, p); });
    HIPCHK(e0);
    return init_common(h);
}

// Self test of the stream's normals, kept in the translation unit of k_init_normal: the compiler narrows the pair-index arithmetic of the stream functions
// by the callers it sees in one unit, and this kernel's code is the same as before only next to the start states' draws.
// the normals of one transition as the samplers draw them: one thread per (chain, element pair)
__global__ __launch_bounds__(256) void k_transition_normals(unsigned long long seed, unsigned long long first_chain, long long nchains,
                                                            unsigned long long t, int D, double* __restrict__ z, double* __restrict__ accept_u)
{
    kd_tables_to_lds();
    const int npairs = (D + 1) / 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = i < nchains * (long long)(npairs + 1);
    const long long c = ok ? i / (npairs + 1) : 0;
    const int p = ok ? (int)(i % (npairs + 1)) : 0;
    const unsigned long long chain = first_chain + (unsigned long long)c;
    if (p < npairs) {
        double z0, z1, u1, lg;
        kd_normal_pair_at(seed, chain, t, (uint32_t)p, (uint32_t)npairs, &z0, &z1, &u1, &lg);
        if (ok) {
            z[c * D + 2 * p] = z0;
            if (2 * p + 1 < D) z[c * D + 2 * p + 1] = z1;
        }
    } else if (ok && accept_u != nullptr) {
        accept_u[c] = kd_accept_uniform(kd_stream_block(seed, chain, t, (uint32_t)npairs));
    }
}

extern "C" klara_status klara_selftest_transition_normals(int32_t device, uint64_t seed, uint64_t first_chain, int64_t nchains,
                                                          uint64_t transition, int32_t ndims, double* z, double* accept_u)
{
    if (!z || nchains <= 0 || ndims <= 0 || ndims > 4096) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    double* dz = nullptr; double* du = nullptr;
    hipError_t e = dalloc(&dz, (size_t)nchains * (size_t)ndims);
    if (e == hipSuccess) e = dalloc(&du, (size_t)nchains);
    if (e == hipSuccess) {
        const long long nthreads = (long long)nchains * ((ndims + 1) / 2 + 1);
        hipLaunchKernelGGL(k_transition_normals, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, 0, (unsigned long long)seed,
                           (unsigned long long)first_chain, (long long)nchains, (unsigned long long)transition, (int)ndims, dz, du);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(z, dz, sizeof(double) * (size_t)nchains * (size_t)ndims, hipMemcpyDeviceToHost);
    if (e == hipSuccess && accept_u) e = hipMemcpy(accept_u, du, sizeof(double) * (size_t)nchains, hipMemcpyDeviceToHost);
    (void)dfree(dz); (void)dfree(du);
    return e == hipSuccess ? KLARA_OK : KLARA_ERR_HIP;
}

// reset(job[, x]) rewinds the sampler / tuner state and the counters; the reference's random generator keeps advancing, so the
// next run is an independent replicate (BasicMCJob.jl:187-201).  The counter-based stream restarts its transition index at 0, so
// the job moves on to a fresh Philox key instead: seed + epoch * KLARA_EPOCH_KEY_STRIDE (klara_stream_key reports it).
// klara_set_state alone keeps the key: it is the way to replay a job from chosen values.
extern "C" klara_status klara_reset(klara_handle* h, const double* x_host)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!x_host && !h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    // the job moves to its next key only if the reset succeeds: a failed one — non-finite initial values, a device
    // error — leaves the epoch, the key and the device copy of the parameters as they were
    const auto put_params = [&]() -> klara_status {
        const KParams hp = make_params(h);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(h->d_params, &hp, sizeof(KParams), hipMemcpyHostToDevice));
        return KLARA_OK;
    };
    h->epoch += 1;
    klara_status st = put_params();
    if (st == KLARA_OK) st = x_host ? klara_set_state(h, x_host) : init_common(h);
    if (st != KLARA_OK) { h->epoch -= 1; (void)put_params(); }
    // MH(Σ): the descriptor's factor again (klara_set_state alone keeps what klara_set_mh_factor gave: the factor is the job's, not a chain's)
    if (st == KLARA_OK && h->mh_factor) HIPCHK(hipMemcpy(h->mh_factor, h->mh_factor0.data(), h->mh_factor0.size() * sizeof(double), hipMemcpyHostToDevice));
    return st;
}

extern "C" klara_status klara_stream_key(klara_handle* h, uint64_t* key, uint64_t* epoch)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (key) *key = h->d.seed + h->epoch * KLARA_EPOCH_KEY_STRIDE;
    if (epoch) *epoch = h->epoch;
    return KLARA_OK;
}

// layout kind 3: the chains [c0, c1) of partition j of nparts — cut in blocks of 16 chains (64 / G for the wider layouts), i.e. whole
// chain groups of every kernel that may run the job
void part_range(const klara_handle* h, int nparts, int j, long long* c0, long long* c1)
{
    const long long N = h->d.nchains, blk = 16;
    const long long blocks = (N + blk - 1) / blk, per = (blocks + nparts - 1) / nparts;
    *c0 = j * per * blk; *c1 = (j + 1) * per * blk;
    if (*c0 > N) *c0 = N;
    if (*c1 > N) *c1 = N;
}

static long long saved_upto(const klara_desc& d, long long steps);       // (launch planning, below)

// ---- layout kind 3: which pair-transposed kernels run partition j of a launch (jobs both families can run: the same bits either way)
struct DiagtChoice {
    int n = 0, lanes[2] = { 0, 0 }; KAuto ka[2] = { KLARA_AUTO_NONE, KLARA_AUTO_NONE };     // one kernel, or both families
    int counter = -1;            // the n_launch_mode entry the launch counts in (klara_get_launch_modes: which family ran); -1: none
    bool pair = false;           // both families are enqueued (klara_handle::pair_enqueued)
    void add(int l, const KAuto& k) { lanes[n] = l; ka[n] = k; ++n; }
};
// force: 0: 4 lanes per chain; 1: the plan's lanes; -1: decided on the device.  `nchains` chains in the partition, launch `idx` of the job.  Reads the handle —
// the host's mirror of the device's decisions with it — and changes nothing: launch_steps applies `counter` and `pair`.
static DiagtChoice diagt_choose(const klara_handle* h, const KLaunch& kl, int nparts, int j, long long nchains, int force, long long idx)
{
    const KlaraPlan& P = h->plan;
    const bool sums = (h->d.monitor & KLARA_MON_SUMMARIES) != 0;
    DiagtChoice c;
    if (force >= 0 && !(P.q4_ok && sums)) {
        c.add(force == 0 ? 4 : P.G, KLARA_AUTO_NONE);
        if (P.q4_ok) c.counter = force == 0 ? 0 : 1;
        return c;
    }
    // running sums on a job both kernel families can run: every launch counts its accepted proposals and leaves the
    // decision for the next one in the partition's cell of the other parity (KAuto)
    KAuto ka;
    ka.cell_in = nullptr;
    ka.cell_out = h->auto_cells + 2 * j + (int)((idx + 1) & 1);
    ka.acc_ctr = h->auto_ctr + j;
    ka.mirror = h->auto_mirror_dev ? h->auto_mirror_dev + 4 * j : nullptr;
    ka.thr_work = (unsigned long long)(P.auto_threshold * 65536.0 * (double)nchains * (double)kl.nsteps);
    ka.fanout = nparts == 1 ? 4 : 1;             // a whole-job launch decides for every partition
    ka.launch_idx = (int)idx;
    if (force >= 0) {
        ka.my_mode = force;
        c.add(force == 0 ? 4 : 8, ka);
        c.counter = force;
    } else if (kl.nsteps < KLARA_AUTO_PAIR_MIN_STEPS) {
        // a short launch is not worth an idle sibling: the host picks from the last decision it has seen (stale at worst),
        // and only every 16th such launch counts its accepted proposals and renews the decision (the workgroups of a
        // one-transition launch all finish together: their counter updates on one address are ~20 % of such a launch)
        ka.my_mode = h->auto_mirror ? (__atomic_load_n(h->auto_mirror + 4 * j, __ATOMIC_RELAXED) != 0) : 1;
        c.add(ka.my_mode == 0 ? 4 : 8, (idx & 15) == 0 ? ka : KLARA_AUTO_NONE);
        c.counter = ka.my_mode;
    } else if (nparts == 1 && h->pair_enqueued && h->auto_mirror
               && __atomic_load_n(h->auto_mirror + 4 * j + 2, __ATOMIC_ACQUIRE) == (int)(idx - 1)) {
        // a synchronous caller (one launch per run, the previous one complete): the decision for this launch is already on the
        // host — one kernel, unconditional, no idle sibling (~5 us of a 20-transition launch).  Only after a launch has enqueued both
        // families: a kernel family's first dispatch on a queue sets up its scratch (~120 us, once).
        // (klara_get_kernel_attributes never gets here: it names the family it asks about)
        ka.my_mode = __atomic_load_n(h->auto_mirror + 4 * j, __ATOMIC_RELAXED) != 0;
        c.add(ka.my_mode == 0 ? 4 : 8, ka);
        c.counter = 2;
    } else {
        // both kernels, each subject to the decision the previous launch left (an idle sibling costs ~3 us of a launch that
        // takes hundreds: 17.9 against 17.7 us per transition for 20-transition launches, nothing measurable on two streams)
        c.pair = true;
        ka.cell_in = h->auto_cells + 2 * j + (int)(idx & 1);
        ka.my_mode = 0; c.add(4, ka);
        ka.my_mode = 1; c.add(8, ka);
        c.counter = 2;
    }
    return c;
}

// one pair-transposed kernel of `lanes` lanes per chain over the chains [c0, c1), on stream st
static hipError_t diagt_launch(klara_handle* h, const KLaunch& kl, int lanes, const KAuto& ka, long long c0, long long c1, hipStream_t st)
{
    const klara_desc& d = h->d;
    const KParams* p = h->d_params;
    const KlaraPlan& P = h->plan;
    const bool unitw = h->gw == nullptr && h->gmu == nullptr, onestep = kl.nsteps == 1;   // (device copies; the host pointers are dropped at create)
    const bool mon = (d.monitor & ~(uint32_t)KLARA_MON_ACCEPT) != 0;                      // a saved-sample monitor is on
    const bool da = d.tuner == KLARA_TUNER_DUAL_AVERAGING;                                 // (HMC only: validate())
    const bool tune = !P.plain || da;                                                      // something counts proposals / tunes
    KLaunch kp = kl;
    const long long cpw = 64 / lanes;
    kp.group0 = c0 / cpw; kp.group_end = (c1 + cpw - 1) / cpw;
    const long long nw = kp.group_end - kp.group0;               // one wavefront per group of cpw chains
    const int np = lanes == 4 ? P.np4 : P.E / 2;
    if (P.jit_pair) return klara_jit_launch_pair(h->jit, (onestep && !tune && !mon && d.sampler != KLARA_SAMPLER_SLICE) ? 1 : 0, p, kp, nw, st);
    const DiagtLaunchers& L = diagt_launchers(lanes);
    switch (d.sampler) {
    case KLARA_SAMPLER_MH: return L.mh(p, kp, np, onestep && !tune, unitw, mon, tune, da, ka, nw, st);
    case KLARA_SAMPLER_MALA: return L.mala(p, kp, np, onestep && !tune, unitw, mon, tune, da, ka, nw, st);
    case KLARA_SAMPLER_SLICE: {
        if (!P.slice_free) return L.slice(p, kp, np, unitw, mon, tune, ka, nw, st);
        const hipError_t e = L.slice_free(p, kp, np, unitw, mon, ka, nw, P.slice_machines, st);
        if (e != hipSuccess || h->hist_lt == nullptr || klara_attr_query != nullptr) return e;
        // the saved states' log-targets, from their saved values (klara_diagt_slice.h)
        const long long nsaved = saved_upto(d, (long long)kl.t0 + kl.nsteps) - saved_upto(d, (long long)kl.t0);
        return L.hist_lt(p, kp, np, unitw, kl.save_col0, (int)nsaved, nw, st);
    }
    default: return L.hmc(p, kp, np, lanes != 4 && onestep && !tune, unitw, mon, tune, da, ka, nw, st);    // (4 lanes: no one-transition HMC kernel)
    }
}

hipError_t launch_steps(klara_handle* h, const KLaunch& kl, int nparts)
{
    const klara_desc& d = h->d;
    const KParams* p = h->d_params;
    const KlaraPlan& P = h->plan;
    const int mode = (P.nmodes == 2 && kl.nsteps == 1) ? P.modes[1] : P.modes[0];     // (7: one iterate! per launch)
    const dim3 grid(P.grid_init), grid_steps(P.grid_steps);
    if (P.kind == 1) return klara_launch_dense(p, kl, d.sampler, d.tuner, P.plain, P.E, h->Pfrag, h->dense_mu, grid, h->stream);
    if (P.kind == 5) return klara_launch_logit_mfma(p, kl, d.sampler, d.tuner == KLARA_TUNER_DUAL_AVERAGING, P.E, h->Pfrag, h->ly, h->logit_nblocks, grid, h->stream);
    if (P.kind == 6) return klara_launch_dense_split(p, kl, d.sampler, d.tuner == KLARA_TUNER_DUAL_AVERAGING, P.G, P.E, P.split_mw, P.lds, d.ndims, h->Pfrag, h->dense_mu, grid, h->stream);
    if (P.kind == 3) {
        // which kernel family runs the launch (q4_ok jobs: same bits either way): 0: 4 lanes per chain; 1: 8 lanes; -1: decided on the device
        // (one transition per launch of HMC: the 8-lane single-transition kernel measured 5 % faster)
        int force = d.sampler == KLARA_SAMPLER_HMC && kl.nsteps == 1 ? 1 : P.family;
        const bool query = klara_attr_query != nullptr;       // klara_get_kernel_attributes: which kernel, not a launch
        if (query && P.q4_ok) force = h->query_lanes == 8 ? 1 : 0;
        const long long idx = h->launch_idx;
        if (!query) ++h->launch_idx;
        for (int j = 0; j < nparts; ++j) {
            long long c0, c1;
            part_range(h, nparts, j, &c0, &c1);
            if (c0 >= c1) break;
            const DiagtChoice c = diagt_choose(h, kl, nparts, j, c1 - c0, force, idx);
            if (!query) {
                if (c.pair) h->pair_enqueued = true;
                if (c.counter >= 0 && j == 0) ++h->n_launch_mode[c.counter];
            }
            for (int i = 0; i < c.n; ++i) {
                const hipError_t e = diagt_launch(h, kl, c.lanes[i], c.ka[i], c0, c1, j == 0 ? h->stream : h->side[j - 1]);
                if (e != hipSuccess) return e;
            }
        }
        return hipSuccess;
    }
    if (P.kind == 4) {
        const bool mon = (d.monitor & ~(uint32_t)KLARA_MON_ACCEPT) != 0;
        const bool da = d.tuner == KLARA_TUNER_DUAL_AVERAGING;
        return klara_launch_hiert(p, kl, d.sampler, P.E / 2, d.hier_ntimes, mon, !P.plain || da, da, grid, h->stream);
    }
    if (d.target == KLARA_TARGET_CUSTOM) return klara_jit_launch(h->jit, mode, p, kl, grid_steps, P.lds, h->stream, 64 * P.custom_wpb);
    return klara_pick<KLARA_SAMPLER_MH, KLARA_SAMPLER_MALA, KLARA_SAMPLER_HMC, KLARA_SAMPLER_SLICE, KLARA_SAMPLER_SMMALA, KLARA_SAMPLER_RAM, KLARA_SAMPLER_AM,
                      KLARA_SAMPLER_AMWG, KLARA_SAMPLER_MH_COV>(d.sampler, [&](auto s) {
        return klara_launch_sampler<decltype(s)::value>(p, kl, mode, d.target, P.E, P.G, grid_steps, P.lds, h->stream);
    });
}

// ---- launch planning: pure host logic (no device), shared by klara_run_async and klara_selftest_plan ------------------------
// Where the next launch of a run ends: after steps_per_launch transitions (library default KLARA_DEFAULT_STEPS_PER_LAUNCH), at the next event of the pooled
// tuner (tuners.jl:27-32 — the rate is pooled over the GPU's chains between launches) or where the next batch of saved samples
// closes (streaming batch means), whichever comes first; plus the save-rule bookkeeping the kernels take from the host
// (BasicMCRange.jl:36 postrange = (burnin+1):thinning:nsteps), so that they carry no 64-bit division.
struct RunCursor { long long steps_done, m_prop, m_tot, bm_count; };
struct PlannedLaunch { long long k; int save_phase0; long long save_col0; bool tune_after, bm_close_after; long long saved; };

// columns of the history ring of a job (0: every saved step is kept) — klara_desc.hist_ring_cols, or the 32-column value ring the
// streaming autocovariances, the pooled covariance, the pooled marginal histograms and the derived quantities keep for themselves when no value history was asked for
static long long ring_cols(const klara_desc& d)
{
    long long r = d.hist_ring_cols;
    if ((d.acov_maxlag > 0 || (d.monitor & KLARA_MON_COVARIANCE) || d.marg_nbins > 0 || d.derived_nout > 0) && !(d.monitor & KLARA_MON_HISTORY) && r == 0) r = 32;
    const long long npost = (d.nsteps - d.burnin - 1) / d.thinning + 1;
    return (r > 0 && r < npost) ? r : 0;
}
// saved (post-burn-in, thinned) steps among the first `steps` transitions
static long long saved_upto(const klara_desc& d, long long steps)
{
    const long long sd = steps < d.nsteps ? steps : d.nsteps;
    return sd > d.burnin ? (sd - d.burnin - 1) / d.thinning + 1 : 0;
}

static PlannedLaunch plan_launch(const klara_desc& d, long long spl, const RunCursor& c, long long remaining)
{
    PlannedLaunch pl;
    const bool pooled_cnt = d.tuner_mode == KLARA_TUNE_POOLED && cnt_predicate(d);
    long long k = remaining < spl ? remaining : spl;
    if (pooled_cnt && c.m_tot <= d.burnin) {
        const long long to_boundary = d.period - (c.m_prop % d.period);
        if (k > to_boundary) k = to_boundary;
    }
    // saved sample number S is transition burnin + (S - 1) * thinning + 1
    long long bm_close_at = -1;
    if (d.bm_batchlen > 0) {
        bm_close_at = d.burnin + ((c.bm_count + 1) * d.bm_batchlen - 1) * d.thinning + 1;
        if (bm_close_at > d.nsteps) bm_close_at = -1;
        else if (bm_close_at > c.steps_done && k > bm_close_at - c.steps_done) k = bm_close_at - c.steps_done;
    }
    // phase of the first post-burn-in step of this launch and the number of columns already saved
    pl.save_phase0 = c.steps_done >= d.burnin ? (int)((c.steps_done - d.burnin) % d.thinning) : 0;
    pl.save_col0 = c.steps_done > d.burnin ? (c.steps_done - d.burnin - 1) / d.thinning + 1 : 0;
    // history ring: a launch never wraps — it ends with the last column of the ring at the latest, the kernels get the ring
    // column of their first saved step (saved sample number S is transition burnin + (S - 1) * thinning + 1)
    const long long ring = ring_cols(d);
    if (ring > 0) {
        const long long room = ring - pl.save_col0 % ring;
        const long long next = d.burnin + (pl.save_col0 + room) * d.thinning + 1;              // transition of the first sample that would wrap
        if (c.steps_done + k >= next) k = next - 1 - c.steps_done;
        if (k < 1) k = 1;
    }
    pl.k = k;
    pl.saved = saved_upto(d, c.steps_done + k) - saved_upto(d, c.steps_done);
    if (ring > 0) pl.save_col0 %= ring;
    pl.tune_after = pooled_cnt;
    pl.bm_close_after = bm_close_at >= 0 && c.steps_done + k == bm_close_at;
    return pl;
}

static void advance_cursor(const klara_desc& d, RunCursor& c, const PlannedLaunch& pl)
{
    if (pl.tune_after) {
        c.m_prop += pl.k;
        if (c.m_tot <= d.burnin && (c.m_prop % d.period) == 0) { c.m_tot += c.m_prop; c.m_prop = 0; }
    }
    c.steps_done += pl.k;
    if (pl.bm_close_after) ++c.bm_count;
}

extern "C" klara_status klara_run_async(klara_handle* h, int64_t nsteps)
{
    if (!h || nsteps < 0) return KLARA_ERR_INVALID_ARG;
    if (!h->have_state) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    const klara_desc& d = h->d;
    if ((d.monitor & KLARA_MON_ACCEPT) && h->steps_done + nsteps > h->accept_cap) return KLARA_ERR_STATE;
    KParams p = make_params(h);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // Chain partitions on internal streams pay off when a run issues several launches per partition (the streams drift apart and
    // one partition's kernel fills the SIMDs while the other's ramps up or drains: 12.9 vs 14.1 us per transition at 65,536 x 100).
    // A run that is a single launch is issued whole on the caller's stream: two half-size kernels that start together only split
    // the machine unevenly (16.7 vs 17.8 us per transition for 20-transition runs).
    const int nparts = nsteps > h->plan.steps_per_launch ? h->plan.nparts : 1;
    if (nparts > 1) {                                      // fork: the partition streams start after everything queued so far
        HIPCHK(hipEventRecord(h->fork_ev, h->stream));
        for (int j = 0; j + 1 < nparts; ++j) HIPCHK(hipStreamWaitEvent(h->side[j], h->fork_ev, 0));
    }
    long long remaining = nsteps, launches = 0;
    RunCursor cur = { h->steps_done, h->m_prop, h->m_tot, h->bm_count };
    hipError_t err = hipSuccess;
    while (remaining > 0 && err == hipSuccess) {
        const PlannedLaunch pl = plan_launch(d, h->plan.steps_per_launch, cur, remaining);
        KLaunch kl;
        kl.group0 = 0; kl.group_end = 0x7fffffffffffffffll;
        kl.t0 = (unsigned long long)cur.steps_done;
        kl.nsteps = (int)pl.k;                                             // (plan_launch keeps k <= steps_per_launch <= INT_MAX)
        kl.save_phase0 = pl.save_phase0;
        kl.save_col0 = pl.save_col0;
        err = launch_steps(h, kl, nparts);
        if (err == hipSuccess && pl.tune_after) {
            hipLaunchKernelGGL(k_pooled_tune, dim3(1), dim3(64), 0, h->stream, p, (int)pl.k);
            err = hipGetLastError();
        }
        if (err == hipSuccess && pl.bm_close_after) err = launch_bm_close(h, nparts);   // (reads h->bm_count: batches closed before this one)
        if (err == hipSuccess && h->acov_S && pl.saved > 0) {                   // streaming autocovariances consume the launch's samples
            err = launch_acov_update(h->stream, h->hist, h->acov_S, h->acov_head, h->acov_tail, h->acov_near, h->acov_total, h->acov_n, h->acov_W,
                                     (long long)d.nchains * d.ndims, pl.save_col0, pl.saved);
            h->acov_n += pl.saved;
        }
        if (err == hipSuccess && h->cov_S && pl.saved > 0) {                    // ... and so does the pooled covariance (klara_cov.h)
            if (h->cov_n == 0)                                                  // the pivot: local chain 0's first saved sample, before the ring overwrites it
                err = hipMemcpyAsync(h->cov_pivot, h->hist + (size_t)pl.save_col0 * (size_t)d.nchains * (size_t)d.ndims, (size_t)d.ndims * sizeof(double),
                                     hipMemcpyDeviceToDevice, h->stream);
            if (err == hipSuccess) err = klara_cov_launch_update(h->cov, h->hist, pl.save_col0, pl.saved, h->cov_pivot, h->cov_S, h->cov_T, h->stream);
            h->cov_n += pl.saved;
        }
        if (err == hipSuccess && h->marg_counts && pl.saved > 0) {              // ... and the pooled marginal histograms (klara_marg.h)
            err = klara_marg_launch_update(h->marg, h->hist, pl.save_col0, pl.saved, h->marg_par, h->marg_counts, h->stream);
            h->marg_n += pl.saved;
        }
        if (err == hipSuccess && h->der_jit && pl.saved > 0) {                  // ... and the derived quantities (klara_derived.h)
            err = klara_derived_launch_update(h->der_jit, h->der, h->hist, pl.save_col0, pl.saved, h->der_data, h->der_ndata, h->der_sum, h->der_sumsq,
                                              h->der_stage, &h->der_marg, h->der_marg_par, h->der_counts, nullptr, h->stream);
            h->der_n += pl.saved;
        }
        if (err != hipSuccess) break;
        advance_cursor(d, cur, pl);
        h->steps_done = cur.steps_done; h->m_prop = cur.m_prop; h->m_tot = cur.m_tot; h->bm_count = cur.bm_count;
        remaining -= pl.k; ++launches;
    }
    // join — also when a launch failed: the partition streams may still have work in flight on X / GR / LT, and every later
    // call (get_state, reset, destroy) synchronises the caller's stream only
    for (int j = 0; j + 1 < nparts; ++j) {
        const hipError_t e1 = hipEventRecord(h->join_ev[j], h->side[j]);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(h->stream, h->join_ev[j], 0) : e1;
        if (e2 != hipSuccess) { hipStreamSynchronize(h->side[j]); if (err == hipSuccess) err = e2; }
    }
    HIPCHK(err);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->last_launches = launches; h->timed = true;
    h->nsaved = saved_upto(d, h->steps_done);       // saved-sample bookkeeping: count of i in postrange with i <= steps_done
    return KLARA_OK;
}

extern "C" klara_status klara_synchronize(klara_handle* h)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(h->d.device));
    int flag = 0;
    KCHK(sync_read_flag(h, &flag));
    return (klara_status)flag;
}

extern "C" klara_status klara_run(klara_handle* h, int64_t nsteps)
{
    klara_status s = klara_run_async(h, nsteps);
    if (s != KLARA_OK) return s;
    return klara_synchronize(h);
}

extern "C" klara_status klara_last_run_ms(klara_handle* h, double* kernel_ms, int64_t* nlaunches)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    if (!h->timed) return KLARA_ERR_STATE;
    HIPCHK(hipSetDevice(h->d.device));
    HIPCHK(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    if (kernel_ms) *kernel_ms = (double)ms;
    if (nlaunches) *nlaunches = h->last_launches;
    return KLARA_OK;
}

extern "C" klara_status klara_selftest_plan(const klara_desc* desc, int32_t nruns, const int64_t* run_lengths, int64_t capacity,
                                            int64_t* k, int64_t* save_col0, int32_t* save_phase0, int32_t* flags, int64_t* nlaunches)
{
    if (!run_lengths || nruns <= 0 || !nlaunches) return KLARA_ERR_INVALID_ARG;
    const klara_status st = validate(desc);
    if (st != KLARA_OK) return st;
    KlaraPlan plan;
    (void)klara_plan_job(*desc, klara_read_overrides(), &plan);     // (the launch length of a job klara_create would refuse is planned too)
    RunCursor cur = { 0, 0, desc->period, 0 };           // tuner_state: totproposed starts at period (samplers.jl:39-45)
    long long n = 0;
    for (int r = 0; r < nruns; ++r) {
        long long remaining = run_lengths[r];
        if (remaining < 0) return KLARA_ERR_INVALID_ARG;
        while (remaining > 0) {
            const PlannedLaunch pl = plan_launch(*desc, plan.steps_per_launch, cur, remaining);
            if (n < capacity) {
                if (k) k[n] = pl.k;
                if (save_col0) save_col0[n] = pl.save_col0;
                if (save_phase0) save_phase0[n] = pl.save_phase0;
                if (flags) flags[n] = (pl.tune_after ? 1 : 0) | (pl.bm_close_after ? 2 : 0) | (remaining == pl.k ? 4 : 0);
            }
            advance_cursor(*desc, cur, pl);
            remaining -= pl.k; ++n;
        }
    }
    *nlaunches = n;
    return KLARA_OK;
}
