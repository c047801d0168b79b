// klara_create.hip — descriptor validation, klara_create / klara_destroy and the kernels' parameter block.
#include <new>
#include "klara_handle.h"

std::string pair_as_whole_source(const char* src) { return std::string("#define KLARA_PAIR_AS_WHOLE 1\n") + src; }

bool pack_mh_factor(const double* L, int D, std::vector<double>& tri)
{
    tri.assign(KLARA_MHCOV_TRI + 16, 0.0);      // (16 doubles behind the triangle: a scalar load of 16 dwords that starts at its last entries stays inside the array)
    for (int i = 0; i < 32; ++i) tri[(size_t)i * (i + 1) / 2 + i] = 1.0;
    for (int i = 0; i < D && i < 32; ++i) {
        if (!(L[(size_t)i * D + i] > 0.0)) return false;
        for (int k = 0; k <= i; ++k) {
            if (!std::isfinite(L[(size_t)i * D + k])) return false;
            tri[(size_t)i * (i + 1) / 2 + k] = L[(size_t)i * D + k];
        }
    }
    return true;
}

static klara_status validate_fields(const klara_desc* d)
{
    if (!d) return KLARA_ERR_INVALID_ARG;
    if (d->struct_size != sizeof(klara_desc) || d->abi_version != KLARA_ABI_VERSION) return KLARA_ERR_INVALID_ARG;
    if (d->nchains <= 0 || d->ndims <= 0 || d->chain_offset < 0) return KLARA_ERR_INVALID_ARG;
    if (!sampler_valid(d->sampler)) return KLARA_ERR_INVALID_ARG;
    if (d->target < KLARA_TARGET_GAUSS_DIAG || d->target > KLARA_TARGET_CUSTOM) return KLARA_ERR_INVALID_ARG;
    if (d->tuner < KLARA_TUNER_VANILLA || d->tuner > KLARA_TUNER_ROBERTS_ROSENTHAL) return KLARA_ERR_INVALID_ARG;
    if (d->tuner == KLARA_TUNER_DUAL_AVERAGING) {                // DualAveragingMCTuner.jl:65-70
        if (!(d->targetrate > 0.0 && d->targetrate < 1.0) || d->da_nadapt <= 0 || !(d->da_eps0bar > 0.0) || d->da_t0 <= 0 ||
            !(d->da_gamma > 0.0))
            return KLARA_ERR_INVALID_ARG;
        if (d->sampler != KLARA_SAMPLER_HMC || d->tuner_mode != KLARA_TUNE_PER_CHAIN) return KLARA_ERR_UNSUPPORTED;
    }
    if (d->tuner_mode != KLARA_TUNE_PER_CHAIN && d->tuner_mode != KLARA_TUNE_POOLED) return KLARA_ERR_INVALID_ARG;
    // BasicMCRange.jl:22-24
    if (d->burnin < 0 || d->thinning < 1 || d->thinning > 0x7fffffff || d->nsteps <= d->burnin) return KLARA_ERR_INVALID_ARG;
    // VanillaMCTuner / AcceptanceRateMCTuner.jl:32-33
    if (d->period <= 0) return KLARA_ERR_INVALID_ARG;
    if (d->nstreams < 0 || d->nstreams > 4) return KLARA_ERR_INVALID_ARG;
    if (d->tuner == KLARA_TUNER_ACCEPT_RATE && !(d->targetrate > 0.0 && d->targetrate < 1.0)) return KLARA_ERR_INVALID_ARG;
    switch (d->sampler) {
    case KLARA_SAMPLER_MH:
        if (!d->mh_sigma) return KLARA_ERR_INVALID_ARG;
        for (int i = 0; i < d->ndims; ++i) if (!(d->mh_sigma[i] > 0.0)) return KLARA_ERR_INVALID_ARG;
        break;
    case KLARA_SAMPLER_MALA:                                     // MALA.jl:65
    case KLARA_SAMPLER_SMMALA:                                   // SMMALA.jl:132 "Drift step is not positive"
        if (!(d->driftstep > 0.0)) return KLARA_ERR_INVALID_ARG;
        break;
    case KLARA_SAMPLER_HMC:                                      // HMC.jl:94-95
        if (!(d->leapstep > 0.0) || d->nleaps <= 0) return KLARA_ERR_INVALID_ARG;
        break;
    case KLARA_SAMPLER_RAM:                                      // RAM.jl:100-102
        if (!d->ram_S0) return KLARA_ERR_INVALID_ARG;
        if (d->ndims <= 8) {                                     // (beyond: KLARA_ERR_UNSUPPORTED from the planner, whatever the factor)
            for (int i = 0; i < d->ndims; ++i) {
                if (!(d->ram_S0[i * d->ndims + i] > 0.0)) return KLARA_ERR_INVALID_ARG;
                for (int j = 0; j <= i; ++j) if (!std::isfinite(d->ram_S0[i * d->ndims + j])) return KLARA_ERR_INVALID_ARG;
            }
        }
        if (!(d->ram_targetrate > 0.0 && d->ram_targetrate < 1.0) || !(d->ram_gamma > 0.5 && d->ram_gamma <= 1.0)) return KLARA_ERR_INVALID_ARG;
        // the tuner only counts proposals (iterate/RAM.jl:68-69, 107-121): VanillaMCTuner, per chain
        if (d->tuner != KLARA_TUNER_VANILLA || d->tuner_mode != KLARA_TUNE_PER_CHAIN) return KLARA_ERR_UNSUPPORTED;
        break;
    case KLARA_SAMPLER_AM:                                       // AM.jl:138-143, AM.jl:107-109 (w[1] = 1 - c > 0)
        if (!d->am_C0) return KLARA_ERR_INVALID_ARG;
        if (d->ndims <= 8) {                                     // (beyond: KLARA_ERR_UNSUPPORTED from the planner, whatever the matrix)
            for (int i = 0; i < d->ndims; ++i)
                for (int j = i; j < d->ndims; ++j) if (!std::isfinite(d->am_C0[i * d->ndims + j])) return KLARA_ERR_INVALID_ARG;
        }
        if (!(d->am_corescale > 0.0) || !std::isfinite(d->am_corescale) || !(d->am_minorscale > 0.0) || !std::isfinite(d->am_minorscale)) return KLARA_ERR_INVALID_ARG;
        if (!(d->am_c >= 0.0 && d->am_c < 1.0) || d->am_t0 <= 0) return KLARA_ERR_INVALID_ARG;
        if (d->am_t0 == 1) return KLARA_ERR_UNSUPPORTED;         // k = count - 2 = 0 at the first update: a division by zero
        // the tuner only counts proposals (iterate/AM.jl:80-82, 123-125, 137-151): VanillaMCTuner, per chain
        if (d->tuner != KLARA_TUNER_VANILLA || d->tuner_mode != KLARA_TUNE_PER_CHAIN) return KLARA_ERR_UNSUPPORTED;
        break;
    case KLARA_SAMPLER_AMWG:                                     // AMWG.jl:139-151, RobertsRosenthalMCTuner.jl:89-93
        if (!d->amwg_logsigma0) return KLARA_ERR_INVALID_ARG;
        if (d->ndims <= 32) {                                    // (beyond: KLARA_ERR_UNSUPPORTED from the planner, whatever the scales)
            for (int i = 0; i < d->ndims; ++i) if (!std::isfinite(d->amwg_logsigma0[i])) return KLARA_ERR_INVALID_ARG;
        }
        if (d->tuner != KLARA_TUNER_ROBERTS_ROSENTHAL || d->tuner_mode != KLARA_TUNE_PER_CHAIN) return KLARA_ERR_UNSUPPORTED;
        if (!(d->targetrate > 0.0 && d->targetrate < 1.0) || d->period > 0x7fffffff) return KLARA_ERR_INVALID_ARG;
        break;
    case KLARA_SAMPLER_MH_COV: {                                 // MH.jl:63-66, the matrix form: the factor of Σ; mh_sigma is not read
        if (!d->mh_factor) return KLARA_ERR_INVALID_ARG;
        std::vector<double> tri;
        if (d->ndims <= 32 && !pack_mh_factor(d->mh_factor, d->ndims, tri)) return KLARA_ERR_INVALID_ARG;     // (beyond: KLARA_ERR_UNSUPPORTED from the planner, whatever the factor)
        // the tuner only counts proposals, as for MH: VanillaMCTuner, per chain
        if (d->tuner != KLARA_TUNER_VANILLA || d->tuner_mode != KLARA_TUNE_PER_CHAIN) return KLARA_ERR_UNSUPPORTED;
        break;
    }
    default:                                                     // SliceSampler.jl:27
        if (!d->slice_widths) return KLARA_ERR_INVALID_ARG;
        for (int i = 0; i < d->ndims; ++i) if (!(d->slice_widths[i] > 0.0)) return KLARA_ERR_INVALID_ARG;
        break;
    }
    if (d->target == KLARA_TARGET_GAUSS_DENSE && !d->gauss_prec) return KLARA_ERR_INVALID_ARG;
    if (d->target == KLARA_TARGET_HIER_NORMAL &&
        (!d->hier_Y || !d->hier_xc || d->hier_nunits <= 0 || d->hier_ntimes <= 0 || d->hier_ntimes > 16 ||
         d->ndims != 2 * d->hier_nunits + 5 || !(d->hier_prior_prec >= 0.0) || !(d->hier_gamma_a >= 0.0) ||
         !(d->hier_gamma_b >= 0.0)))
        return KLARA_ERR_INVALID_ARG;
    if (d->target == KLARA_TARGET_LOGISTIC &&
        (!d->logit_X || !d->logit_y || d->logit_ndata <= 0 || !(d->logit_lambda > 0.0)))
        return KLARA_ERR_INVALID_ARG;
    if (d->target == KLARA_TARGET_CUSTOM && (!d->custom_src || d->custom_ndata < 0 || (d->custom_ndata > 0 && !d->custom_data)))
        return KLARA_ERR_INVALID_ARG;
    if (d->hist_ring_cols < 0 || d->acov_maxlag < 0 || d->acov_maxlag > 127 || d->sparse_moves < 0 || d->sparse_moves > 2) return KLARA_ERR_INVALID_ARG;
    if (d->bm_batchlen < 0 || (d->bm_batchlen > 0 && !(d->monitor & KLARA_MON_SUMMARIES))) return KLARA_ERR_INVALID_ARG;
    // softabs(G, a) of the SMMALA metric (samplers/SMMALA.jl:129 transform): a finite a >= 0, 0 = none; the logistic target's metric is positive
    // definite by construction (X' diag(r (1 - r)) X + I / lambda) and is not transformed
    if (!(d->smmala_softabs >= 0.0) || !std::isfinite(d->smmala_softabs)) return KLARA_ERR_INVALID_ARG;
    if (d->smmala_softabs > 0.0 && d->sampler != KLARA_SAMPLER_SMMALA) return KLARA_ERR_INVALID_ARG;
    if (d->smmala_softabs > 0.0 && d->target != KLARA_TARGET_CUSTOM) return KLARA_ERR_UNSUPPORTED;
    if (d->sampler != KLARA_SAMPLER_RAM && (d->ram_S0 != nullptr || d->ram_targetrate != 0.0 || d->ram_gamma != 0.0)) return KLARA_ERR_INVALID_ARG;
    if (d->sampler != KLARA_SAMPLER_AMWG && d->amwg_logsigma0 != nullptr) return KLARA_ERR_INVALID_ARG;
    if (d->sampler != KLARA_SAMPLER_AMWG && d->tuner == KLARA_TUNER_ROBERTS_ROSENTHAL) return KLARA_ERR_UNSUPPORTED;
    if (d->sampler != KLARA_SAMPLER_MH_COV && d->mh_factor != nullptr) return KLARA_ERR_INVALID_ARG;
    if (d->sampler != KLARA_SAMPLER_AM && (d->am_C0 != nullptr || d->am_corescale != 0.0 || d->am_minorscale != 0.0 || d->am_c != 0.0 || d->am_t0 != 0))
        return KLARA_ERR_INVALID_ARG;
    // pooled marginal histograms: 0 = off and no pointers; 1 .. KLARA_MARG_MAX_BINS with finite lo[d] < hi[d]
    if (d->marg_nbins < 0 || d->marg_nbins > KLARA_MARG_MAX_BINS) return KLARA_ERR_INVALID_ARG;
    if (d->marg_nbins == 0 ? (d->marg_lo != nullptr || d->marg_hi != nullptr) : (!d->marg_lo || !d->marg_hi)) return KLARA_ERR_INVALID_ARG;
    for (int i = 0; d->marg_nbins > 0 && i < d->ndims; ++i)
        if (!std::isfinite(d->marg_lo[i]) || !std::isfinite(d->marg_hi[i]) || !(d->marg_lo[i] < d->marg_hi[i])) return KLARA_ERR_INVALID_ARG;
    // derived quantities: 0 = off and nothing else set; a source and 1 .. KLARA_DERIVED_MAX_OUT outputs; histograms of the outputs as the marginals' fields
    if (d->derived_nout < 0 || d->derived_nout > KLARA_DERIVED_MAX_OUT || (d->derived_src != nullptr) != (d->derived_nout > 0)) return KLARA_ERR_INVALID_ARG;
    if (d->derived_ndata < 0 || (d->derived_ndata > 0) != (d->derived_data != nullptr) || (d->derived_ndata > 0 && d->derived_nout == 0)) return KLARA_ERR_INVALID_ARG;
    if (d->derived_nbins < 0 || d->derived_nbins > KLARA_MARG_MAX_BINS || (d->derived_nbins > 0 && d->derived_nout == 0)) return KLARA_ERR_INVALID_ARG;
    if (d->derived_nbins == 0 ? (d->derived_lo != nullptr || d->derived_hi != nullptr) : (!d->derived_lo || !d->derived_hi)) return KLARA_ERR_INVALID_ARG;
    for (int64_t i = 0; d->derived_nbins > 0 && i < d->derived_nout; ++i)
        if (!std::isfinite(d->derived_lo[i]) || !std::isfinite(d->derived_hi[i]) || !(d->derived_lo[i] < d->derived_hi[i])) return KLARA_ERR_INVALID_ARG;
    if (d->steps_per_launch < 0 || d->tuner_score < 0 || d->tuner_score > 1) return KLARA_ERR_INVALID_ARG;   // (int32: a launch length always fits KLaunch::nsteps)
    return KLARA_OK;
}

// the monitors a job cannot have, whatever its layout: the likelihood / prior history needs a likelihood + prior user target (no other target
// has the two parts, a pair closure neither); no gradient is carried by MH / slice / RAM
static klara_status validate_monitors(const klara_desc& d)
{
    if ((d.monitor & KLARA_MON_HIST_LLLP) && (d.target != KLARA_TARGET_CUSTOM || !custom_lik_prior(d.custom_src) || pair_source(d.custom_src)))
        return KLARA_ERR_INVALID_ARG;
    if ((d.monitor & KLARA_MON_HIST_GRAD) && !sampler_needs_gradient(d.sampler)) return KLARA_ERR_INVALID_ARG;
    return KLARA_OK;
}

klara_status validate(const klara_desc* d)
{
    const klara_status st = validate_fields(d);
    return st != KLARA_OK ? st : validate_monitors(*d);
}

static klara_status upload(DeviceArrays& mem, double** dst, const double* src, size_t n)
{
    HIPCHK(mem.alloc(dst, n));
    HIPCHK(hipMemcpy(*dst, src, n * sizeof(double), hipMemcpyHostToDevice));
    return KLARA_OK;
}

// the device arrays (false: one of them had damaged canaries), then what is not memory: pinned host words, the run-time compiled kernels, events, streams
static bool free_all(klara_handle* h)
{
    const bool ok = h->mem.release();
    if (h->auto_mirror) hipHostFree(h->auto_mirror);
    if (h->flag_host) hipHostFree(h->flag_host);
    klara_jit_destroy(h->jit);
    klara_jit_destroy(h->der_jit);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    for (int j = 0; j < 3; ++j) { if (h->side[j]) hipStreamDestroy(h->side[j]); if (h->join_ev[j]) hipEventDestroy(h->join_ev[j]); }
    if (h->fork_ev) hipEventDestroy(h->fork_ev);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    return ok;
}

// The logistic-regression target beyond D = 8 (the row-split kernels hold the whole parameter vector of a chain in every lane's
// registers and the data rows in LDS): the same closures — doc/examples/swiss/MALA/analytical.jl:11-18, operation for operation what
// LogisticTarget::eval and the oracle's ko_logistic_eval compute with all rows on one lane — as source text for the run-time compiled
// path (klara_custom.h): one chain per lane, E = pow2ceil(D) <= 256 elements, the data block [lambda, D log(2 pi lambda), X, y] read
// from global memory, any number of rows.
static const char* const KLARA_LOGIT_WIDE_SRC = R"SRC(
KLARA_USER_FN double klara_user_logtarget(const double* p, int D, const double* data, long long ndata)
{
    const long long n = (ndata - 2) / (KLARA_D + 1);
    const double lambda = data[0], lpconst = data[1];
    const double* X = data + 2; const double* y = X + n * KLARA_D;
    double dotxy = 0.0, slog = 0.0;
    for (long long r = 0; r < n; ++r) {
        double xp = 0.0;
        for (int e = 0; e < KLARA_D; ++e) xp = kd_fma(X[r * KLARA_D + e], p[e], xp);
        double sp, lg;
        kd_softplus_logistic_rows(xp, &sp, &lg);
        dotxy = dotxy + xp * y[r];
        slog = slog + sp;
    }
    double dotpp = 0.0;
    for (int e = 0; e < KLARA_D; ++e) dotpp = dotpp + p[e] * p[e];
    const double ll = dotxy - slog;
    const double lp = -0.5 * (dotpp / lambda + lpconst);
    return ll + lp;
}
KLARA_USER_FN void klara_user_gradlogtarget(const double* p, int D, const double* data, long long ndata, double* g)
{
    const long long n = (ndata - 2) / (KLARA_D + 1);
    const double lambda = data[0];
    const double* X = data + 2; const double* y = X + n * KLARA_D;
    for (int e = 0; e < KLARA_D; ++e) g[e] = 0.0;
    for (long long r = 0; r < n; ++r) {
        double xp = 0.0;
        for (int e = 0; e < KLARA_D; ++e) xp = kd_fma(X[r * KLARA_D + e], p[e], xp);
        double sp, lg;
        kd_softplus_logistic_rows(xp, &sp, &lg);
        const double res = y[r] - lg;
        for (int e = 0; e < KLARA_D; ++e) g[e] = kd_fma(X[r * KLARA_D + e], res, g[e]);
    }
    for (int e = 0; e < KLARA_D; ++e) g[e] = g[e] - p[e] / lambda;
}
)SRC";

// The dense Gaussian beyond D = 128 (the matrix-core layouts end there): the same closure form — g = -(P d) as a k-ascending fma chain
// per row, lt = c + 1/2 sum_i d_i g_i, d = x - mu (the oracle's ko_dense_grad / ko_dense_lt_from_grad with all elements on one lane);
// data block [c, P (D x D row-major), mu (D)].
static const char* const KLARA_DENSE_WIDE_SRC = R"SRC(
KLARA_USER_FN void klara_user_gradlogtarget(const double* x, int D, const double* data, long long ndata, double* g)
{
    const double* P = data + 1; const double* mu = P + (long long)KLARA_D * KLARA_D;
    _Pragma("nounroll")
    for (int i = 0; i < KLARA_D; ++i) {
        double acc = 0.0;
        _Pragma("unroll 4")
        for (int k = 0; k < KLARA_D; ++k) acc = kd_fma(P[(long long)i * KLARA_D + k], x[k] - mu[k], acc);
        g[i] = -acc;
    }
}
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    const double* P = data + 1; const double* mu = P + (long long)KLARA_D * KLARA_D;
    double s = 0.0;
    _Pragma("nounroll")
    for (int i = 0; i < KLARA_D; ++i) {
        double acc = 0.0;
        _Pragma("unroll 4")
        for (int k = 0; k < KLARA_D; ++k) acc = kd_fma(P[(long long)i * KLARA_D + k], x[k] - mu[k], acc);
        s = s + (x[i] - mu[i]) * (-acc);
    }
    return data[0] + 0.5 * s;
}
)SRC";

// Layout kind 5: the A fragments of both MFMA passes in the order of consumption (klara_logit_mfma.h logitm_eval), zero beyond the n rows / D columns:
// block b = RBT tiles of 16 rows; pass 1, step kk RBT + tt: lane l holds X[16 (b RBT + tt) + (l & 15)][4 kk + (l >> 4)];
// pass 2, step (4 tt + j) MT + t: lane l holds X[16 (b RBT + tt) + 4 j + (l >> 4)][16 t + (l & 15)].  *ypad: the responses, zero-padded to the blocks' rows.
static std::vector<double> pack_logit_stream(const klara_desc& d, int NE, std::vector<double>* ypad, int* nblocks)
{
    const int MT = NE / 4, RBT = klara_logit_mfma_rbt(), S1 = RBT * NE;
    const size_t n = (size_t)d.logit_ndata, D = (size_t)d.ndims;
    const int NT = (int)((n + 15) / 16), nb = (NT + RBT - 1) / RBT;
    std::vector<double> frag((size_t)nb * 2 * S1 * 64, 0.0);
    ypad->assign((size_t)nb * RBT * 16, 0.0);
    for (int b = 0; b < nb; ++b) {
        double* const f1 = frag.data() + (size_t)b * 2 * S1 * 64;
        double* const f2 = f1 + (size_t)S1 * 64;
        for (int sidx = 0; sidx < S1; ++sidx) {
            const int kk = sidx / RBT, tt = sidx % RBT;
            const int tt2 = sidx / (4 * MT), j = (sidx / MT) & 3, t = sidx % MT;
            for (int l = 0; l < 64; ++l) {
                const size_t r1 = 16 * (size_t)(b * RBT + tt) + (l & 15), c1 = 4 * (size_t)kk + (l >> 4);
                if (r1 < n && c1 < D) f1[(size_t)sidx * 64 + l] = d.logit_X[r1 * D + c1];
                const size_t r2 = 16 * (size_t)(b * RBT + tt2) + 4 * (size_t)j + (l >> 4), c2 = 16 * (size_t)t + (l & 15);
                if (r2 < n && c2 < D) f2[(size_t)sidx * 64 + l] = d.logit_X[r2 * D + c2];
            }
        }
    }
    for (size_t r = 0; r < n; ++r) (*ypad)[r] = d.logit_y[r];
    *nblocks = nb;
    return frag;
}

// Layout kinds 1 and 6: the fragment-ordered, zero-padded P for the MFMA A operand (klara_dense.h), followed by the mean where the job has one
// (layout kind 6: ceil(D / 4) k-steps of MT = ceil(D / 16) tiles, k-major, and KLARA_SPLIT_PAD = 8 k-steps of zeros behind them — the ring's last
// prefetch, klara_dense_split.h)
static std::vector<double> pack_dense_fragments(const klara_desc& d, int kind, int E)
{
    const size_t D = (size_t)d.ndims;
    const int NE = kind == 6 ? (D + 3) / 4 : E, MT = kind == 6 ? (D + 15) / 16 : (NE + 3) / 4;
    std::vector<double> frag((size_t)MT * (NE + (kind == 6 ? 8 : 0)) * 64, 0.0);
    // (NE % 4 == 1: the last tile is the 4-row tail for v_mfma_f64_4x4x4_4b, A_b[i][k] on lane 16k + 4b + i)
    const bool tail = kind != 6 && (NE % 4) == 1;
    // tile-major (t, kk) for the LDS-resident layouts; k-major (kk, t) — the order of consumption — for the streamed ones (NE > 32)
    const bool kmajor = NE > 32 || kind == 6;
    for (int t = 0; t < MT; ++t)
        for (int kk = 0; kk < NE; ++kk)
            for (int l = 0; l < 64; ++l) {
                const size_t row = 16 * (size_t)t + ((tail && t == MT - 1) ? (l & 3) : (l & 15)), col = 4 * (size_t)kk + (l >> 4);
                const size_t f = kmajor ? (size_t)kk * MT + t : (size_t)t * NE + kk;
                if (row < D && col < D) frag[f * 64 + l] = d.gauss_prec[row * D + col];
            }
    if (d.gauss_mu) {                                            // the mean, [4 e + q] = mu[4 e + q], zero beyond D
        const size_t at = frag.size();
        frag.resize(at + 4 * (size_t)(kind == 6 ? 4 * MT : NE) + (kind == 6 ? 32 : 0), 0.0);         // (kind 6: 4 MT rows + KLARA_SPLIT_PAD the pass's last prefetch touches)
        for (size_t i = 0; i < D; ++i) frag[at + i] = d.gauss_mu[i];
    }
    return frag;
}

namespace {
struct HandleGuard {            // a handle under construction: freed on every way out of create_impl but the last
    klara_handle* h;
    ~HandleGuard() { if (h) { (void)free_all(h); delete h; } }
};
}

static klara_status create_impl(const klara_desc* desc, const KlaraPlan& plan, klara_handle** out)
{
    const int kind = plan.kind, G = plan.G, E = plan.E;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || desc->device < 0 || desc->device >= ndev)
        return KLARA_ERR_HIP;
    HIPCHK(hipSetDevice(desc->device));

    klara_handle* h = new (std::nothrow) klara_handle();
    if (!h) return KLARA_ERR_NOMEM;
    HandleGuard guard = { h };
    DeviceArrays& mem = h->mem;
    h->d = *desc; h->plan = plan;
    const size_t N = (size_t)desc->nchains, D = (size_t)desc->ndims;
    const bool pooled = desc->tuner_mode == KLARA_TUNE_POOLED;
    const size_t NT = pooled ? 1 : N;

    if (desc->stream) { h->stream = (hipStream_t)desc->stream; h->own_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    HIPCHK(hipEventCreate(&h->ev0)); HIPCHK(hipEventCreate(&h->ev1));
    if (kind == 3) {
        const int np = plan.nparts;
        if (np > 1) HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
        for (int j = 0; j + 1 < np; ++j) {
            HIPCHK(hipStreamCreateWithFlags(&h->side[j], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&h->join_ev[j], hipEventDisableTiming));
        }
        HIPCHK(mem.alloc(&h->clock_probe, 4)); HIPCHK(hipMemset(h->clock_probe, 0, 4 * sizeof(unsigned long long)));
        if (plan.q4_ok && (desc->monitor & KLARA_MON_SUMMARIES)) {
            HIPCHK(mem.alloc(&h->auto_cells, 8)); HIPCHK(mem.alloc(&h->auto_ctr, 4));
            if (hipHostMalloc((void**)&h->auto_mirror, 16 * sizeof(int), hipHostMallocMapped) == hipSuccess) {
                for (int i = 0; i < 16; ++i) h->auto_mirror[i] = (i & 3) == 0 ? 1 : ((i & 3) == 2 ? -1 : 0);
                if (hipHostGetDevicePointer((void**)&h->auto_mirror_dev, h->auto_mirror, 0) != hipSuccess) { hipHostFree(h->auto_mirror); h->auto_mirror = nullptr; h->auto_mirror_dev = nullptr; }
            } else { h->auto_mirror = nullptr; (void)hipGetLastError(); }
        }
    }

    HIPCHK(mem.alloc(&h->X, N * D)); HIPCHK(mem.alloc(&h->GR, N * D)); HIPCHK(mem.alloc(&h->LT, N));
    HIPCHK(mem.alloc(&h->tune_step, NT)); HIPCHK(mem.alloc(&h->tune_acc, NT)); HIPCHK(mem.alloc(&h->tune_prop, NT));
    HIPCHK(mem.alloc(&h->tune_tot, NT));
    if (desc->tuner == KLARA_TUNER_DUAL_AVERAGING) { HIPCHK(mem.alloc(&h->da_epsbar, NT)); HIPCHK(mem.alloc(&h->da_hbar, NT)); } HIPCHK(mem.alloc(&h->pooled_acc, 1)); HIPCHK(mem.alloc(&h->naccept, N));
    // error flag: a mapped word of host memory the kernels store to directly — klara_synchronize then needs no copy command behind the
    // kernels (a 20-transition run of the headline job is ~350 us: a 4-byte device-to-host copy and its completion signal are ~2 % of that)
    if (hipHostMalloc((void**)&h->flag_host, sizeof(int), hipHostMallocMapped) == hipSuccess
        && hipHostGetDevicePointer((void**)&h->err, h->flag_host, 0) == hipSuccess) *h->flag_host = 0;
    else { if (h->flag_host) hipHostFree(h->flag_host); h->flag_host = nullptr; h->err = nullptr; (void)hipGetLastError(); HIPCHK(mem.alloc(&h->err, 1)); HIPCHK(hipMemset(h->err, 0, sizeof(int))); }
    HIPCHK(mem.alloc(&h->pooled_out, 2 * D + 2)); HIPCHK(mem.alloc(&h->pool_partial, (size_t)1024 * (2 * D + 1)));
    if (desc->monitor & KLARA_MON_SUMMARIES) { HIPCHK(mem.alloc(&h->sum, N * D)); HIPCHK(mem.alloc(&h->sumsq, N * D)); HIPCHK(mem.alloc(&h->held, N)); }
    if (desc->bm_batchlen > 0) { HIPCHK(mem.alloc(&h->bm_prev, N * D)); HIPCHK(mem.alloc(&h->bm_mean, N * D)); HIPCHK(mem.alloc(&h->bm_m2, N * D)); }
    if (desc->monitor & KLARA_MON_ACCEPT) {
        h->accept_cap = desc->nsteps;
        HIPCHK(mem.alloc(&h->accept, (size_t)desc->nsteps * N));
    }
    const bool acov = desc->acov_maxlag > 0, cov = plan.cov, marg = desc->marg_nbins > 0, der = desc->derived_nout > 0, keeps = acov || cov || marg || der;      // the consumers of the saved samples keep values
    if ((desc->monitor & (KLARA_MON_HISTORY | KLARA_MON_HIST_LT | KLARA_MON_HIST_GRAD | KLARA_MON_HIST_LLLP)) || keeps) {
        // npoststeps = length((burnin+1):thinning:nsteps)  (BasicMCRange.jl:26)
        h->hist_cols = (desc->nsteps - desc->burnin - 1) / desc->thinning + 1;
        long long ringc = desc->hist_ring_cols;
        if (keeps && !(desc->monitor & KLARA_MON_HISTORY) && ringc == 0) ringc = 32;    // the consumer's own value ring
        if (keeps) { h->d.monitor |= KLARA_MON_HISTORY; h->d.hist_ring_cols = ringc; }   // (the kernels save values; ring_cols(h->d) == ringc)
        if (ringc > 0 && ringc < h->hist_cols) { h->hist_cols = ringc; h->ring = true; }
        if ((desc->monitor & KLARA_MON_HISTORY) || keeps) HIPCHK(mem.alloc(&h->hist, (size_t)h->hist_cols * N * D));
        if (acov) {
            h->acov_W = desc->acov_maxlag + 1;
            const size_t ws = (size_t)h->acov_W * N * D;
            HIPCHK(mem.alloc(&h->acov_S, ws)); HIPCHK(mem.alloc(&h->acov_head, ws)); HIPCHK(mem.alloc(&h->acov_tail, ws)); HIPCHK(mem.alloc(&h->acov_total, N * D));
            if (h->acov_W > 32) HIPCHK(mem.alloc(&h->acov_near, (size_t)32 * N * D));      // (scratch of the far-tail update, launch_acov_update)
        }
        if (cov) {
            if (!klara_cov_plan((long long)N, (int)D, &h->cov)) return KLARA_ERR_UNSUPPORTED;
            HIPCHK(mem.alloc(&h->cov_S, klara_cov_S_elems(h->cov))); HIPCHK(mem.alloc(&h->cov_T, klara_cov_T_elems(h->cov)));
            HIPCHK(mem.alloc(&h->cov_pivot, D)); HIPCHK(mem.alloc(&h->cov_out, D + D * D));
        }
        if (marg) {
            if (!klara_marg_plan((long long)N, (int)D, desc->marg_nbins, &h->marg)) return KLARA_ERR_UNSUPPORTED;
            h->marg_host.assign(desc->marg_lo, desc->marg_lo + D);
            h->marg_host.insert(h->marg_host.end(), desc->marg_hi, desc->marg_hi + D);
            std::vector<double> par(h->marg_host);
            for (size_t i = 0; i < D; ++i) par.push_back(klara_marg_inv_w(desc->marg_nbins, desc->marg_lo[i], desc->marg_hi[i]));
            KCHK(upload(mem, &h->marg_par, par.data(), par.size()));
            HIPCHK(mem.alloc(&h->marg_counts, klara_marg_count_elems(h->marg)));
            HIPCHK(hipMemset(h->marg_counts, 0, klara_marg_count_elems(h->marg) * sizeof(unsigned long long)));
        }
        if (der) {                                               // the closure's kernel, its data block and the chains' sums; the reductions' workspaces
            const int K = (int)desc->derived_nout;
            const size_t NK = N * (size_t)K;
            if (!klara_derived_plan((long long)N, (int)D, K, &h->der)) return KLARA_ERR_UNSUPPORTED;
            KCHK(klara_jit_create_derived(desc->derived_src, (int)D, K, desc->derived_nbins > 0, true, &h->der_jit));
            if (desc->derived_ndata > 0) KCHK(upload(mem, &h->der_data, desc->derived_data, (size_t)desc->derived_ndata));
            h->der_ndata = desc->derived_ndata;
            HIPCHK(mem.alloc(&h->der_sum, NK)); HIPCHK(mem.alloc(&h->der_sumsq, NK)); HIPCHK(mem.alloc(&h->der_zero, N));
            HIPCHK(hipMemset(h->der_sum, 0, NK * sizeof(double))); HIPCHK(hipMemset(h->der_sumsq, 0, NK * sizeof(double)));
            HIPCHK(hipMemset(h->der_zero, 0, N * sizeof(long long)));
            HIPCHK(mem.alloc(&h->der_partial, (size_t)1024 * (2 * (size_t)K + 1))); HIPCHK(mem.alloc(&h->der_out, 2 * (size_t)K + 2));
            if (desc->derived_nbins > 0) {
                if (!klara_marg_plan((long long)N, K, desc->derived_nbins, &h->der_marg)) return KLARA_ERR_UNSUPPORTED;
                h->der_marg_host.assign(desc->derived_lo, desc->derived_lo + K);
                h->der_marg_host.insert(h->der_marg_host.end(), desc->derived_hi, desc->derived_hi + K);
                std::vector<double> par(h->der_marg_host);
                for (int i = 0; i < K; ++i) par.push_back(klara_marg_inv_w(desc->derived_nbins, desc->derived_lo[i], desc->derived_hi[i]));
                KCHK(upload(mem, &h->der_marg_par, par.data(), par.size()));
                HIPCHK(mem.alloc(&h->der_stage, (size_t)KLARA_DERIVED_MAX_COLS * NK));
                HIPCHK(mem.alloc(&h->der_counts, klara_marg_count_elems(h->der_marg)));
                HIPCHK(hipMemset(h->der_counts, 0, klara_marg_count_elems(h->der_marg) * sizeof(unsigned long long)));
            }
        }
        if (desc->monitor & KLARA_MON_HIST_LT) HIPCHK(mem.alloc(&h->hist_lt, (size_t)h->hist_cols * N));
        if (desc->monitor & KLARA_MON_HIST_LLLP) { HIPCHK(mem.alloc(&h->hist_ll, (size_t)h->hist_cols * N)); HIPCHK(mem.alloc(&h->hist_lp, (size_t)h->hist_cols * N)); }
        if (desc->monitor & KLARA_MON_HIST_GRAD) HIPCHK(mem.alloc(&h->hist_g, (size_t)h->hist_cols * N * D));
    }
    if (desc->sampler == KLARA_SAMPLER_MH) KCHK(upload(mem, &h->vecparam, desc->mh_sigma, D));
    if (desc->sampler == KLARA_SAMPLER_SLICE) KCHK(upload(mem, &h->vecparam, desc->slice_widths, D));
    if (desc->sampler == KLARA_SAMPLER_RAM) {                    // the packed lower triangle of S0, in the planes' order (ktri(j, i, D))
        std::vector<double> tri(D * (D + 1) / 2);
        for (size_t i = 0; i < D; ++i) for (size_t j = 0; j <= i; ++j) tri[(size_t)ktri((int)j, (int)i, (int)D)] = desc->ram_S0[i * D + j];
        KCHK(upload(mem, &h->ram_S0, tri.data(), tri.size()));
        HIPCHK(mem.alloc(&h->ram_S, tri.size() * N)); HIPCHK(mem.alloc(&h->ram_skipped, 1));
    }
    if (desc->sampler == KLARA_SAMPLER_AM) {                     // the packed upper triangle of C0 (C_ij, i <= j, at ktri(i, j, D)); the means' 2 D planes
        std::vector<double> tri(D * (D + 1) / 2);
        for (size_t i = 0; i < D; ++i) for (size_t j = i; j < D; ++j) tri[(size_t)ktri((int)i, (int)j, (int)D)] = desc->am_C0[i * D + j];
        KCHK(upload(mem, &h->am_C0, tri.data(), tri.size()));
        HIPCHK(mem.alloc(&h->am_C, tri.size() * N)); HIPCHK(mem.alloc(&h->am_mean, 2 * D * N)); HIPCHK(mem.alloc(&h->am_fallbacks, 1));
    }
    if (desc->sampler == KLARA_SAMPLER_AMWG) {                   // D planes of scales, window counts and accepted proposals; the coordinate masks beside the accept mask
        KCHK(upload(mem, &h->amwg_logsig0, desc->amwg_logsigma0, D));
        HIPCHK(mem.alloc(&h->amwg_logsig, D * N)); HIPCHK(mem.alloc(&h->amwg_acc, D * N)); HIPCHK(mem.alloc(&h->amwg_nacc, D * N));
        if (desc->monitor & KLARA_MON_ACCEPT) HIPCHK(mem.alloc(&h->amwg_mask, (size_t)desc->nsteps * N));
    }
    if (desc->sampler == KLARA_SAMPLER_MH_COV) {                 // one triangle for the job (validated above)
        (void)pack_mh_factor(desc->mh_factor, (int)D, h->mh_factor0);
        KCHK(upload(mem, &h->mh_factor, h->mh_factor0.data(), h->mh_factor0.size()));
    }
    if (desc->target == KLARA_TARGET_GAUSS_DIAG) {
        if (desc->gauss_w) KCHK(upload(mem, &h->gw, desc->gauss_w, D));
        if (desc->gauss_mu) KCHK(upload(mem, &h->gmu, desc->gauss_mu, D));
    } else if (desc->target == KLARA_TARGET_HIER_NORMAL) {
        KCHK(upload(mem, &h->hY, desc->hier_Y, (size_t)desc->hier_nunits * (size_t)desc->hier_ntimes));
        KCHK(upload(mem, &h->hxc, desc->hier_xc, (size_t)desc->hier_ntimes));
    } else if (desc->target == KLARA_TARGET_CUSTOM) {
        if (desc->custom_ndata > 0) KCHK(upload(mem, &h->cdata, desc->custom_data, (size_t)desc->custom_ndata));
        if (plan.jit_pair) {
            // k_diagt instantiations for this job: fused launches always; one transition per launch where that kernel exists
            const bool mon_ = (h->d.monitor & ~(uint32_t)KLARA_MON_ACCEPT) != 0, da_ = desc->tuner == KLARA_TUNER_DUAL_AVERAGING;
            const bool tune_ = !plan.plain || da_;
            const int modes[2] = { 0, 1 };
            KCHK(klara_jit_create_pair(desc->custom_src, desc->sampler, desc->ndims, E / 2, G, mon_, tune_, da_, modes, (!mon_ && !tune_ && desc->sampler != KLARA_SAMPLER_SLICE) ? 2 : 1, true, &h->jit));
        } else {
            KCHK(klara_jit_create(desc->custom_src, desc->sampler, desc->ndims, E, G, plan.modes, plan.nmodes, true, &h->jit, desc->smmala_softabs > 0.0));
        }
    } else if (desc->target == KLARA_TARGET_LOGISTIC && kind == 5) {
        std::vector<double> ypad;
        const std::vector<double> frag = pack_logit_stream(*desc, E, &ypad, &h->logit_nblocks);
        KCHK(upload(mem, &h->Pfrag, frag.data(), frag.size()));
        KCHK(upload(mem, &h->ly, ypad.data(), ypad.size()));
        h->lpconst = (double)desc->ndims * kd_log(2.0 * 3.141592653589793 * desc->logit_lambda);
    } else if (desc->target == KLARA_TARGET_LOGISTIC) {
        KCHK(upload(mem, &h->lX, desc->logit_X, (size_t)desc->logit_ndata * D));
        KCHK(upload(mem, &h->ly, desc->logit_y, (size_t)desc->logit_ndata));
        // length(p)*log(2*pi*v[1])  (doc/examples/swiss/MALA/analytical.jl:16)
        h->lpconst = (double)desc->ndims * kd_log(2.0 * 3.141592653589793 * desc->logit_lambda);
    } else {
        const std::vector<double> frag = pack_dense_fragments(*desc, kind, E);
        h->dense_mu = desc->gauss_mu != nullptr;
        KCHK(upload(mem, &h->Pfrag, frag.data(), frag.size()));
    }
    // the descriptor's host pointers are not retained
    h->d.mh_sigma = nullptr; h->d.slice_widths = nullptr; h->d.gauss_w = nullptr; h->d.gauss_mu = nullptr;
    h->d.gauss_prec = nullptr; h->d.logit_X = nullptr; h->d.logit_y = nullptr; h->d.hier_Y = nullptr; h->d.hier_xc = nullptr; h->d.stream = nullptr;
    h->d.custom_src = nullptr; h->d.custom_data = nullptr; h->d.ram_S0 = nullptr; h->d.am_C0 = nullptr; h->d.amwg_logsigma0 = nullptr; h->d.mh_factor = nullptr; h->d.marg_lo = nullptr; h->d.marg_hi = nullptr;
    h->d.derived_src = nullptr; h->d.derived_data = nullptr; h->d.derived_lo = nullptr; h->d.derived_hi = nullptr;
    {   // static kernel parameters live in device memory (read with scalar loads at the point of use)
        const KParams hp = make_params(h);
        HIPCHK(mem.alloc(&h->d_params, 1));
        HIPCHK(hipMemcpy(h->d_params, &hp, sizeof(KParams), hipMemcpyHostToDevice));
    }
    guard.h = nullptr;
    *out = h;
    return KLARA_OK;
}

extern "C" klara_status klara_create(const klara_desc* desc, klara_handle** out)
{
    if (!out) return KLARA_ERR_INVALID_ARG;
    *out = nullptr;
    klara_status st = validate_fields(desc);
    if (st != KLARA_OK) return st;
    KlaraPlan plan;
    st = klara_plan_job(*desc, klara_read_overrides(), &plan);      // (a job the planner refuses is KLARA_ERR_UNSUPPORTED whatever it monitors)
    if (st != KLARA_OK) return st;
    // a closure form: the job as a user-defined target, with the data block its closure reads
    klara_desc dd = *desc;
    std::vector<double> blk;
    std::string src;
    if (plan.rewrite == KLARA_REWRITE_LOGIT_WIDE) {            // [lambda, D log(2 pi lambda), X, y]
        const size_t n = (size_t)desc->logit_ndata, D = (size_t)desc->ndims;
        blk.resize(2 + n * (D + 1));
        blk[0] = desc->logit_lambda;
        blk[1] = (double)desc->ndims * kd_log(2.0 * 3.141592653589793 * desc->logit_lambda);
        memcpy(blk.data() + 2, desc->logit_X, n * D * sizeof(double));
        memcpy(blk.data() + 2 + n * D, desc->logit_y, n * sizeof(double));
        dd.custom_src = KLARA_LOGIT_WIDE_SRC; dd.logit_X = nullptr; dd.logit_y = nullptr; dd.logit_ndata = 0;
    } else if (plan.rewrite == KLARA_REWRITE_DENSE_WIDE) {     // [c, P, mu]
        const size_t D = (size_t)desc->ndims;
        blk.assign(1 + D * D + D, 0.0);
        blk[0] = desc->gauss_const;
        memcpy(blk.data() + 1, desc->gauss_prec, D * D * sizeof(double));
        if (desc->gauss_mu) memcpy(blk.data() + 1 + D * D, desc->gauss_mu, D * sizeof(double));
        dd.custom_src = KLARA_DENSE_WIDE_SRC; dd.gauss_prec = nullptr; dd.gauss_mu = nullptr;
    } else if (plan.rewrite == KLARA_REWRITE_PAIR_AS_WHOLE) {
        src = pair_as_whole_source(desc->custom_src);
        dd.custom_src = src.c_str();
    }
    if (plan.rewrite == KLARA_REWRITE_LOGIT_WIDE || plan.rewrite == KLARA_REWRITE_DENSE_WIDE) { dd.target = KLARA_TARGET_CUSTOM; dd.custom_data = blk.data(); dd.custom_ndata = (int64_t)blk.size(); }
    dd.monitor &= ~(uint32_t)KLARA_MON_COVARIANCE;      // (plan.cov carries it: a consumer's flag, not a monitor of the kernels)
    st = validate_monitors(dd);                  // (the job as it runs: a pair closure in its whole-vector form is not a pair closure any more)
    if (st != KLARA_OK) return st;
    return create_impl(&dd, plan, out);
}

extern "C" klara_status klara_destroy(klara_handle* h)
{
    if (!h) return KLARA_ERR_INVALID_ARG;
    hipSetDevice(h->d.device);
    hipStreamSynchronize(h->stream);
    for (int j = 0; j < 3; ++j) if (h->side[j]) hipStreamSynchronize(h->side[j]);
    const bool intact = free_all(h);
    delete h;
    return intact ? KLARA_OK : KLARA_ERR_STATE;        // (KLARA_DEBUG_CANARY=1: a kernel of this job wrote outside one of its arrays)
}

KParams make_params(klara_handle* h)
{
    KParams p;
    memset(&p, 0, sizeof(p));
    const klara_desc& d = h->d;
    p.X = (decltype(p.X))h->X; p.GR = (decltype(p.GR))h->GR; p.LT = (decltype(p.LT))h->LT;
    p.tune_step = (decltype(p.tune_step))h->tune_step; p.tune_accepted = (decltype(p.tune_accepted))h->tune_acc; p.tune_proposed = (decltype(p.tune_proposed))h->tune_prop;
    p.tune_totproposed = (decltype(p.tune_totproposed))h->tune_tot; p.pooled_accepted = (decltype(p.pooled_accepted))h->pooled_acc;
    p.accept = (decltype(p.accept))h->accept; p.naccept = (decltype(p.naccept))h->naccept; p.sum = (decltype(p.sum))h->sum; p.sumsq = (decltype(p.sumsq))h->sumsq; p.held = (decltype(p.held))h->held;
    p.hist = (decltype(p.hist))h->hist; p.hist_cols = h->hist_cols; p.error_flag = (decltype(p.error_flag))h->err;
    p.hist_lt = (decltype(p.hist_lt))h->hist_lt; p.hist_g = (decltype(p.hist_g))h->hist_g;
    p.hist_ll = (decltype(p.hist_ll))h->hist_ll; p.hist_lp = (decltype(p.hist_lp))h->hist_lp;
    p.nchains = d.nchains; p.chain_offset = d.chain_offset; p.D = d.ndims; p.G = h->plan.G; p.rs = h->plan.RS;
    p.pooled = d.tuner_mode == KLARA_TUNE_POOLED;
    p.seed = d.seed + h->epoch * KLARA_EPOCH_KEY_STRIDE;      // (mod 2^64)
    p.vecparam = (decltype(p.vecparam))h->vecparam; p.nleaps = d.nleaps; p.stepout = d.slice_stepout;
    p.tuner = d.tuner; p.cnt = cnt_predicate(d); p.targetrate = d.targetrate;
    p.tuner_score = d.tuner_score; p.score_k = d.score_k; p.period = d.period; p.is_mh = d.sampler == KLARA_SAMPLER_MH;
    p.da_epsbar = (decltype(p.da_epsbar))h->da_epsbar; p.da_hbar = (decltype(p.da_hbar))h->da_hbar; p.da_nadapt = d.da_nadapt; p.da_gamma = d.da_gamma;
    p.da_kappa = d.da_kappa; p.da_t0 = d.da_t0;
    // sampler_state(..., tuner::DualAveragingMCTuner): lambda = nleaps*leapstep, mu = log(10*step) (HMC.jl:124-133,192-213)
    p.da_lambda = (double)d.nleaps * d.leapstep; p.da_mu = kd_log(10.0 * d.leapstep);
    p.step0 = sampler_step0(d);
    p.sqrt_step0 = std::sqrt(p.step0); p.inv_step0 = 1.0 / p.step0;
    p.burnin = d.burnin; p.thinning = d.thinning; p.nsteps_total = d.nsteps;
    p.gw = (decltype(p.gw))h->gw; p.gmu = (decltype(p.gmu))h->gmu; p.gconst = d.gauss_const;
    p.lX = (decltype(p.lX))h->lX; p.ly = (decltype(p.ly))h->ly; p.ndata = d.logit_ndata; p.lambda = d.logit_lambda; p.lpconst = h->lpconst;
    p.hY = (decltype(p.hY))h->hY; p.hxc = (decltype(p.hxc))h->hxc; p.hR = d.hier_nunits; p.hT = d.hier_ntimes; p.hp0 = d.hier_prior_prec;
    p.ha0 = d.hier_gamma_a; p.hb0 = d.hier_gamma_b;
    p.cdata = (decltype(p.cdata))h->cdata; p.cndata = d.custom_ndata;
    p.clock_probe = (decltype(p.clock_probe))h->clock_probe;
    p.smmala_softabs = d.smmala_softabs;
    p.ram_S = (decltype(p.ram_S))h->ram_S; p.ram_skipped = (decltype(p.ram_skipped))h->ram_skipped; p.ram_targetrate = d.ram_targetrate; p.ram_gamma = d.ram_gamma;
    p.am_C = (decltype(p.am_C))h->am_C; p.am_mean = (decltype(p.am_mean))h->am_mean; p.am_fallbacks = (decltype(p.am_fallbacks))h->am_fallbacks;
    p.am_corescale = d.am_corescale; p.am_sqrtminor = std::sqrt(d.am_minorscale); p.am_w1 = 1.0 - d.am_c; p.am_t0 = d.am_t0;     // AM.jl:235-236: sqrtminorscale, w = [1 - c, c]
    p.amwg_logsig = (decltype(p.amwg_logsig))h->amwg_logsig; p.amwg_acc = (decltype(p.amwg_acc))h->amwg_acc; p.amwg_nacc = (decltype(p.amwg_nacc))h->amwg_nacc;
    p.amwg_mask = (decltype(p.amwg_mask))h->amwg_mask;
    p.mh_factor = (decltype(p.mh_factor))h->mh_factor;
    return p;
}

extern "C" const char* klara_strerror(klara_status s)
{
    switch (s) {
    case KLARA_OK: return "ok";
    case KLARA_ERR_INVALID_ARG: return "invalid argument";
    case KLARA_ERR_NONFINITE_INIT: return "log-target (or its gradient) not finite at the initial values";
    case KLARA_ERR_HIP: return "HIP runtime error or no device";
    case KLARA_ERR_NOMEM: return "out of device memory";
    case KLARA_ERR_UNSUPPORTED: return "option not supported by this build";
    case KLARA_ERR_STATE: return "call order / missing state";
    case KLARA_ERR_SLICE_STUCK: return "slice sampler shrunk to current position and still not acceptable";
    case KLARA_ERR_COMPILE: return "user-defined target did not compile (see klara_compile_log)";
    default: return "unknown status";
    }
}

extern "C" int32_t klara_abi_version(void) { return KLARA_ABI_VERSION; }
