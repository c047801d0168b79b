/* klara_oracle.c — CPU restatement of Klara.jl's sampler transition path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library; the
 * product (libklara_hip.so and the klara_jl_amd host package) never links, imports or calls it.
 *
 * PARITY STATUS: "parity unpinned" for sampler trajectories — the reference holds no golden sampler
 * outputs (test/runtests.jl:1-17 runs no sampler/job test) and never seeds its RNG
 * (iterate/MH.jl:79,97; MALA.jl:84,94; HMC.jl:135,165; SliceSampler.jl:66,71,93), and Julia is not
 * installed here, so the reference cannot be run.  Pinned pieces: the tuner score functions
 * (test/common.jl:6, test/AcceptanceRateMCTuner.jl:8-14), the Gaussian target closures
 * (test/BasicContMuvParameter.jl:39-56,62-80,...), the NState column layout
 * (test/ParameterNStates.jl:139-146), Philox4x32-10 (Random123 known-answer vectors) — see
 * tests/test_oracle_kats.py.  Beyond that the oracle is checked against analytic posterior moments and, transition by transition,
 * against an independent Python restatement of the same Julia sources (tests/numpy_mirror.py, tests/test_numpy_mirror.py).
 *
 * Third-party pieces of the reference's arithmetic that are NOT in /root/reference (REQUIRE lists version floors only,
 * there is no lockfile): Julia Base `randn`/`rand` (dSFMT + ziggurat, unseeded — replaced by the build-defined stream
 * below), Base `sum`/`dot` (order unspecified — fixed to the kernels' order below) and Distributions.jl (>= 0.4.7)
 * `rand(::MvNormal)`, `logpdf`/`gradlogpdf(::MvNormal)` at the call sites iterate/MH.jl:79,86,91 and
 * BasicContMuvParameter.jl:163,195: their published definitions are restated (x = mu + sigma .* randn(D) for a diagonal
 * covariance; logpdf = -1/2 (|x-mu|^2/sigma^2 + D log 2 pi) - sum log sigma; gradlogpdf = -(x-mu)/sigma^2) and pinned by
 * the reference's own test values (tests/test_oracle_kats.py::test_mvnormal_target_closures).
 *
 * Each function cites the reference lines it restates.  Arithmetic follows the Julia expressions
 * literally (no fma contraction, same association); the only liberty is the summation order of
 * `sum`/`dot` (unspecified in Julia: BLAS ddot / pairwise SIMD sum), which is fixed to the order the
 * gfx950 kernels use (lane partials, then a pairwise tree over lanes — see ko_layout).
 *
 * Random stream (build-defined; the reference's is unseeded MT19937): Philox4x32-10, key = seed,
 * counter = (transition << 24 | slot, global chain id) — detmath.h kd_stream_block.
 *   normals of a transition: element pair p = i >> 1 <- 64 bits: half (p >> 3) & 1 of block slot (p & 7) + 8 (p >> 4) (one block
 *     serves pairs p and p + 8), Box-Muller on a 44-bit radius uniform and a 20-bit angle, cos branch for even i, sin branch for odd i;
 *   accept uniform (MH, MALA, HMC): slot ceil(D/2), words (x,y), 44 bits;
 *   slice sampler, coordinate i: slot (i << 14): words (x,y) -> log-uniform, (z,w) -> runiform;
 *     shrink attempt a >= 1: slot (i << 14) | ((a + 1) >> 1), words (x,y) for odd a, (z,w) for even a (two attempts per block).
 *   initial state x0 ~ N(0,I): transition index 2^40 - 1 ("-1"), same element -> slot mapping.
 *   SMMALA, RAM, AM: the D normals and the accept uniform of MH / MALA; AM's component selector: words (z,w) of the accept block.
 *
 * SMMALA (with or without the softabs transform of its metric, klara_softabs.h), RAM and AM restate the kernels of klara_kernels.h
 * (step_smmala, step_ram / ram_update, step_am / am_covariance / am_factor) loop for loop — DESIGN.md section 2, deviations S1-S5, T1-T5,
 * R1-R4, A1-A5 — for E <= 8 padded elements per chain and a logistic or user-defined target.  They run in ko_run's two loops like every
 * other sampler; what a chain carries beyond x, g and lt (RAM's factor, AM's covariance and means) comes in through ko_sampler_state.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#include "../include/klara_hip.h"
#include "../klara.jl_amd/csrc/detmath.h"
#include "../klara.jl_amd/csrc/klara_softabs.h"      /* the very header the device compiles (ko_smmala) */

#define KO_MAXD 1024
#define KO_MAXE 8                                    /* SMMALA, RAM, AM: elements per lane the kernels hold a chain's matrix in */
#define KO_MAXNT (KO_MAXE * (KO_MAXE + 1) / 2)

/* LITERAL MODE (VERDICT r3 item 5 / ADVICE r3): ko_set_literal(1) — or KO_LITERAL=1 in the environment when the library is loaded —
 * takes back the deliberate deviations from the literal Julia arithmetic that the shipped oracle shares with the kernels (DESIGN.md
 * section 2 (2), (6), (7)): the leapfrog runs as samplers.jl:130-133 writes it (four unmerged, unfused updates per step), MALA's
 * correction terms are 0.5*(abs2(.)/step) (MALA.jl:90,92), and the logistic rows take log(1+exp(Xp)) and 1/(1+exp(-Xp)) from two
 * exponentials (swiss/MALA/analytical.jl:13,17).  Used by tests/test_literal_arithmetic.py alone, to MEASURE how far the shipped
 * arithmetic is from the literal one; the kernels are compared with the shipped mode. */
static int ko_literal = -1;
static int ko_is_literal(void)
{
    if (ko_literal < 0) { const char* e = getenv("KO_LITERAL"); ko_literal = (e && e[0] == '1') ? 1 : 0; }
    return ko_literal;
}
void ko_set_literal(int on) { ko_literal = on ? 1 : 0; }
int ko_get_literal(void) { return ko_is_literal(); }
/* the data row's pair (log(1+exp(xp)), 1/(1+exp(-xp))): shipped = one exponential (detmath.h), literal = the example's two */
static void ko_row_softplus_logistic(double xp, double* sp, double* lg)
{
    if (ko_is_literal()) {
        *sp = kd_log(1.0 + kd_exp(xp));                                  /* analytical.jl:13 log.(1+exp.(Xp)) */
        *lg = 1.0 / (1.0 + kd_exp(-xp));                                 /* analytical.jl:17 1./(1+exp.(-Xp)) */
    } else {
        kd_softplus_logistic_rows(xp, sp, lg);
    }
}
#define KO_SLICE_ATT_BITS 14
#define KO_SLICE_MAX_ATT ((1 << KO_SLICE_ATT_BITS) - 1)
#define KO_INIT_TRANSITION ((((uint64_t)1) << 40) - 1)

/* lane layout of the device kernels — determines summation order only */
typedef struct ko_layout {
    int32_t kind; /* 0: element i on lane i / E (E contiguous elements per lane), G lanes per chain
                     1: element i on lane-quarter i % 4 (MFMA-transposed), 4 lanes per chain
                     2: logistic row split: every lane holds all elements (sums over elements are sequential),
                        the data rows are dealt round-robin to G lanes and combined by the xor tree
                     3: pair-transposed (klara_diagt.h): element pair i/2 on lane (i/2) % G, lane partials in
                        ascending element order, xor tree over the G lanes
                     4: hierarchical target, few lanes per chain (klara_hiert.h): unit r on lane r / (E/2), the
                        hyper block on lane 0 (after its units); per-unit sums skip the other parameter's slot
                     5: logistic regression on the matrix cores (klara_logit_mfma.h): elements as in kind 1 (element i on
                        lane-quarter i % 4), data row r on lane-quarter r % 4 — row sums are lane partials over ascending
                        rows, then the tree (q0 + q1) + (q2 + q3); X p and X' (y - 1/(1+exp(-Xp))) are the fma chains of
                        v_mfma_f64_16x16x4 (k ascending from zero), i.e. the sequential chains of the closure form
                     6: dense Gaussian on a workgroup of G wavefronts per tile of 16 chains (klara_dense_split.h): element i on
                        lane-quarter i % 4 of the wavefront that owns row tile i / 16 (an even deal of consecutive tiles); lane
                        partials in ascending element order, the tree (q0 + q1) + (q2 + q3) inside each wavefront, then the
                        wavefronts' values in ascending order                                                                */
    int32_t G;
    int32_t E;
} ko_layout;

static double ko_reduce(const ko_layout* L, const double* terms, int D)
{
    double part[64], nw[64];
    if (L->kind == 6) {
        /* the ceil(D / 16) row tiles dealt evenly to the G wavefronts (the first MT % G one more), consecutive tiles each: klara_dense_split.h make_sctx */
        const int MT = (D + 15) / 16, base = MT / L->G, rem = MT - base * L->G;
        double tot = 0.0;
        for (int w = 0; w < L->G; ++w) {
            const int T = base + (w < rem ? 1 : 0), t0 = w * base + (w < rem ? w : rem);
            double pq[4] = { 0.0, 0.0, 0.0, 0.0 };
            for (int i = 16 * t0; i < D && i < 16 * (t0 + T); ++i) pq[i & 3] = pq[i & 3] + terms[i];
            const double v = (pq[0] + pq[1]) + (pq[2] + pq[3]);
            tot = w == 0 ? v : tot + v;
        }
        return tot;
    }
    const int G = (L->kind == 1 || L->kind == 5) ? 4 : (L->kind == 2 ? 1 : L->G);
    for (int l = 0; l < G; ++l) part[l] = 0.0;
    for (int i = 0; i < D; ++i) {
        /* kind 3 (pair-transposed, klara_diagt.h): element pair P = i>>1 belongs to lane P % G */
        /* kind 4 (klara_hiert.h, D = 2R + 5): unit i/2 on lane (i/2) / (E/2); the five hyper elements on lane 0 */
        const int lane = (L->kind == 1 || L->kind == 5) ? (i & 3) : (L->kind == 2 ? 0 : (L->kind == 3 ? ((i >> 1) % L->G) :
                         (L->kind == 4 ? (i < D - 5 ? (i >> 1) / (L->E / 2) : 0) : i / L->E)));
        part[lane] = part[lane] + terms[i];
    }
    for (int m = 1; m < G; m <<= 1) {
        for (int l = 0; l < G; ++l) nw[l] = part[l] + part[l ^ m];
        memcpy(part, nw, sizeof(double) * (size_t)G);
    }
    return part[0];
}

/* the same reduction of the products a[i] * b[i], every lane partial accumulated as fma(a, b, partial) */
static double ko_reduce_prod(const ko_layout* L, const double* a, const double* b, int D)
{
    double part[64], nw[64];
    const int G = L->G;
    for (int l = 0; l < G; ++l) part[l] = 0.0;
    for (int i = 0; i < D; ++i) { const int lane = i / L->E; part[lane] = kd_fma(a[i], b[i], part[lane]); }     /* (contiguous rule only) */
    for (int m = 1; m < G; m <<= 1) {
        for (int l = 0; l < G; ++l) nw[l] = part[l] + part[l ^ m];
        memcpy(part, nw, sizeof(double) * (size_t)G);
    }
    return part[0];
}

/* ------------------------------------------------------------------ tuner scores */
/* src/stats/logistic.jl:11  logistic(x, l, k, x0, y0) = l/(1+exp(-k*(x-x0)))+y0 */
double ko_logistic(double x, double l, double k, double x0, double y0)
{
    return l / (1.0 + kd_exp(-k * (x - x0))) + y0;
}
/* src/tuners/AcceptanceRateMCTuner.jl:9  logistic_rate_score(x, k=7.) = logistic(x, 2., k, 0., 0.) */
double ko_logistic_rate_score(double x, double k) { return ko_logistic(x, 2.0, k, 0.0, 0.0); }
/* src/tuners/AcceptanceRateMCTuner.jl:17 erf_rate_score(x, k=3.) = erf(k*x)+1  (detmath kd_erf: msun s_erf.c operation for operation; the
 * reference vectors test/AcceptanceRateMCTuner.jl:13-14 bit for bit) */
double ko_erf_rate_score(double x, double k) { return kd_erf(k * x) + 1.0; }

/* ------------------------------------------------------------------ targets */
typedef struct ko_target_ctx {
    const klara_desc* d;
    const ko_layout* L;
    double logit_lpconst; /* D*log(2*pi*lambda) */
} ko_target_ctx;

/* README.md:23 `-dot(z,z)`, :155 `-2*z`; MvNormal forms of test/BasicContMuvParameter.jl:39-56 */
static double ko_diag_lt(const ko_target_ctx* c, const double* x, double* scratch)
{
    const klara_desc* d = c->d;
    for (int i = 0; i < d->ndims; ++i) {
        const double mu = d->gauss_mu ? d->gauss_mu[i] : 0.0;
        const double w = d->gauss_w ? d->gauss_w[i] : 1.0;
        const double dd = x[i] - mu;
        scratch[i] = w * (dd * dd);
    }
    return d->gauss_const - ko_reduce(c->L, scratch, d->ndims);
}
static void ko_diag_grad(const ko_target_ctx* c, const double* x, double* g)
{
    const klara_desc* d = c->d;
    for (int i = 0; i < d->ndims; ++i) {
        const double mu = d->gauss_mu ? d->gauss_mu[i] : 0.0;
        const double w = d->gauss_w ? d->gauss_w[i] : 1.0;
        g[i] = (-2.0 * w) * (x[i] - mu);
    }
}

/* dense Gaussian: builder-defined target (SURVEY F8/§8(d) cfg 3). g = -(P d) as a k-ascending fma
 * chain per row (the order of v_mfma_f64_16x16x4_f64 accumulation); lt = c + 1/2 sum_i d_i g_i. */
static void ko_dense_grad(const ko_target_ctx* c, const double* x, double* g)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double dd[KO_MAXD];
    for (int i = 0; i < D; ++i) dd[i] = x[i] - (d->gauss_mu ? d->gauss_mu[i] : 0.0);
    for (int i = 0; i < D; ++i) {
        double acc = 0.0;
        const double* row = d->gauss_prec + (size_t)i * D;
        for (int k = 0; k < D; ++k) acc = kd_fma(row[k], dd[k], acc);
        g[i] = -acc;
    }
}
static double ko_dense_lt_from_grad(const ko_target_ctx* c, const double* x, const double* g, double* scratch)
{
    const klara_desc* d = c->d;
    for (int i = 0; i < d->ndims; ++i) {
        const double dd = x[i] - (d->gauss_mu ? d->gauss_mu[i] : 0.0);
        scratch[i] = dd * g[i];
    }
    return d->gauss_const + 0.5 * ko_reduce(c->L, scratch, d->ndims);
}

/* doc/examples/swiss/MALA/analytical.jl:11-18 (ploglikelihood, plogprior, pgradlogtarget);
 * lt = loglikelihood + logprior (BasicContMuvParameter.jl:184-189).  Row sums are sequential over
 * the data index (the device evaluates one chain per lane). */
static void ko_logit_eval(const ko_target_ctx* c, const double* p, double* lt, double* g)
{
    const klara_desc* d = c->d;
    const int D = d->ndims, n = d->logit_ndata;
    /* row split: row r belongs to lane r % RS; lane partials are then combined pairwise (xor tree) */
    const int RS = (c->L->kind == 2) ? c->L->G : 1;
    double pdot[64], plog[64], pg[64][16];
    if (c->L->kind == 5) {                       /* on the matrix cores (klara_logit_mfma.h): the chains of the closure form, row sums over 4 lane-quarters */
        double pd[4] = { 0.0, 0.0, 0.0, 0.0 }, pl[4] = { 0.0, 0.0, 0.0, 0.0 }, g1[KO_MAXD];
        for (int k = 0; k < D; ++k) g1[k] = 0.0;
        for (int r = 0; r < n; ++r) {
            const double* row = d->logit_X + (size_t)r * D;
            double xp = 0.0;
            for (int k = 0; k < D; ++k) xp = kd_fma(row[k], p[k], xp);          /* pass 1: B = the lanes' parameters, k ascending */
            double sp, lg;
            ko_row_softplus_logistic(xp, &sp, &lg);
            if (lt) { pd[r & 3] = pd[r & 3] + xp * d->logit_y[r]; pl[r & 3] = pl[r & 3] + sp; }
            if (g) { const double res = d->logit_y[r] - lg; for (int k = 0; k < D; ++k) g1[k] = kd_fma(row[k], res, g1[k]); }   /* pass 2: k = data rows ascending */
        }
        if (lt) {
            const double dotxy = (pd[0] + pd[1]) + (pd[2] + pd[3]), slog = (pl[0] + pl[1]) + (pl[2] + pl[3]);
            double pp[KO_MAXD];
            for (int k = 0; k < D; ++k) pp[k] = p[k] * p[k];
            const double dotpp = ko_reduce(c->L, pp, D);
            *lt = (dotxy - slog) + -0.5 * (dotpp / d->logit_lambda + c->logit_lpconst);
        }
        if (g) for (int k = 0; k < D; ++k) g[k] = g1[k] - p[k] / d->logit_lambda;
        return;
    }
    if (RS == 1 && D > 16) {                     /* beyond 16 parameters: all rows on one lane, no tree (the closure form of the library) */
        double dotxy1 = 0.0, slog1 = 0.0, g1[KO_MAXD];
        for (int k = 0; k < D; ++k) g1[k] = 0.0;
        for (int r = 0; r < n; ++r) {
            const double* row = d->logit_X + (size_t)r * D;
            double xp = 0.0;
            for (int k = 0; k < D; ++k) xp = kd_fma(row[k], p[k], xp);
            double sp, lg;
            ko_row_softplus_logistic(xp, &sp, &lg);
            if (lt) { dotxy1 = dotxy1 + xp * d->logit_y[r]; slog1 = slog1 + sp; }
            if (g) { const double res = d->logit_y[r] - lg; for (int k = 0; k < D; ++k) g1[k] = kd_fma(row[k], res, g1[k]); }
        }
        if (lt) {
            double dotpp = 0.0;
            for (int k = 0; k < D; ++k) dotpp = dotpp + p[k] * p[k];
            *lt = (dotxy1 - slog1) + -0.5 * (dotpp / d->logit_lambda + c->logit_lpconst);
        }
        if (g) for (int k = 0; k < D; ++k) g[k] = g1[k] - p[k] / d->logit_lambda;
        return;
    }
    if (D > 16 || RS > 64) { if (lt) *lt = NAN; return; }
    for (int q = 0; q < RS; ++q) { pdot[q] = 0.0; plog[q] = 0.0; for (int k = 0; k < D; ++k) pg[q][k] = 0.0; }
    for (int r = 0; r < n; ++r) {
        const int q = r % RS;
        const double* row = d->logit_X + (size_t)r * D;
        double xp = 0.0;
        for (int k = 0; k < D; ++k) xp = kd_fma(row[k], p[k], xp);            /* Xp = v[2]*p        */
        double sp, lg;                                                          /* log(1+exp(Xp)), 1/(1+exp(-Xp)) from one */
        ko_row_softplus_logistic(xp, &sp, &lg);                                     /* exponential (detmath.h): same value, no overflow */
        if (lt) {
            pdot[q] = pdot[q] + xp * d->logit_y[r];                             /* dot(Xp, v[3])      */
            plog[q] = plog[q] + sp;                                             /* sum(log(1+exp(Xp)))*/
        }
        if (g) {
            const double res = d->logit_y[r] - lg;                              /* v[3]-1./(1+exp(-Xp)) */
            for (int k = 0; k < D; ++k) pg[q][k] = kd_fma(row[k], res, pg[q][k]); /* v[2]'*(...)      */
        }
    }
    for (int m = 1; m < RS; m <<= 1) {
        double nd[64], nl[64], ng[64][16];
        for (int q = 0; q < RS; ++q) {
            nd[q] = pdot[q] + pdot[q ^ m]; nl[q] = plog[q] + plog[q ^ m];
            for (int k = 0; k < D; ++k) ng[q][k] = pg[q][k] + pg[q ^ m][k];
        }
        memcpy(pdot, nd, sizeof(double) * (size_t)RS); memcpy(plog, nl, sizeof(double) * (size_t)RS);
        memcpy(pg, ng, sizeof(double) * 16 * (size_t)RS);
    }
    const double dotxy = pdot[0], slog = plog[0];
    double gacc[KO_MAXD];
    for (int k = 0; k < D; ++k) gacc[k] = pg[0][k];
    if (lt) {
        double pp[KO_MAXD];
        for (int k = 0; k < D; ++k) pp[k] = p[k] * p[k];
        const double dotpp = ko_reduce(c->L, pp, D);
        const double ll = dotxy - slog;
        const double lp = -0.5 * (dotpp / d->logit_lambda + c->logit_lpconst);  /* plogprior          */
        *lt = ll + lp;
    }
    if (g) for (int k = 0; k < D; ++k) g[k] = gacc[k] - p[k] / d->logit_lambda; /* -p/v[1]            */
}

/* KLARA_TARGET_HIER_NORMAL — builder-defined (the reference ships data/rats/*.csv but no model:
 * doc/examples/rats/Gibbs.jl:1-7 is a stub).  BUGS "Rats" in theta = (a_1, b_1, ..., a_R, b_R,
 * a_c, b_c, s_c, s_a, s_b), s = log sigma; w_k = exp(-2 s_k) = 1/sigma_k^2:
 *   lt = -R T s_c - 1/2 w_c sum_ij r_ij^2 - R s_a - 1/2 w_a sum_i (a_i-a_c)^2 - R s_b - 1/2 w_b sum_i (b_i-b_c)^2
 *        - 1/2 p0 (a_c^2 + b_c^2) + sum_k (-2 a0 s_k - b0 w_k),        r_ij = (Y_ij - a_i) - b_i xc_j
 * (Gamma(a0, b0) prior on each precision, Jacobian of s = log sigma included, additive constants dropped).
 * The five sums over rats are reduced in the device's lane order with the rat-i terms at element 2i (a-slots)
 * or 2i+1 (b-slots); per-rat sums over j are sequential. */
static double ko_hier_eval(const ko_target_ctx* c, const double* th, double* g, double* scratch)
{
    const klara_desc* d = c->d;
    const int R = d->hier_nunits, T = d->hier_ntimes, D = d->ndims;
    const double p0 = d->hier_prior_prec, a0 = d->hier_gamma_a, b0 = d->hier_gamma_b;
    const double ac = th[2 * R], bc = th[2 * R + 1], sc = th[2 * R + 2], sa = th[2 * R + 3], sb = th[2 * R + 4];
    const double wc = kd_exp(-2.0 * sc), wa = kd_exp(-2.0 * sa), wb = kd_exp(-2.0 * sb);
    double tA1[KO_MAXD], tB1[KO_MAXD], tA2[KO_MAXD], tB2[KO_MAXD], tC2[KO_MAXD];
    (void)scratch;
    for (int i = 0; i < D; ++i) tA1[i] = tB1[i] = tA2[i] = tB2[i] = tC2[i] = 0.0;
    /* The residuals r_ij = Y_ij - a_i - b_i xc_j enter only through three sums per unit, which are formed from the
     * unit's sufficient statistics (ascending j):  sum r = Sy - T a - b X1,  sum r x = Sxy - a X1 - b X2,
     * sum r^2 = Syy + a (T a - 2 Sy) + b (b X2 + 2 a X1 - 2 Sxy),  with X1 = sum x, X2 = sum x^2. */
    double X1 = 0.0, X2 = 0.0;
    const double Td = (double)T;
    for (int j = 0; j < T; ++j) { X1 = X1 + d->hier_xc[j]; X2 = kd_fma(d->hier_xc[j], d->hier_xc[j], X2); }
    for (int i = 0; i < R; ++i) {
        const double ai = th[2 * i], bi = th[2 * i + 1];
        const double da = ai - ac, db = bi - bc;
        double Sy = 0.0, Sxy = 0.0, Syy = 0.0;
        for (int j = 0; j < T; ++j) {
            const double y = d->hier_Y[i * T + j];
            Sy = Sy + y; Sxy = kd_fma(y, d->hier_xc[j], Sxy); Syy = kd_fma(y, y, Syy);
        }
        const double S1 = kd_fma(-bi, X1, kd_fma(-Td, ai, Sy));
        const double Sx = kd_fma(-bi, X2, kd_fma(-ai, X1, Sxy));
        const double u = kd_fma(Td, ai, -2.0 * Sy);
        const double v = kd_fma(bi, X2, kd_fma(2.0 * ai, X1, -2.0 * Sxy));
        const double S2 = kd_fma(bi, v, kd_fma(ai, u, Syy));
        if (g) { g[2 * i] = kd_fma(wc, S1, -(wa * da)); g[2 * i + 1] = kd_fma(wc, Sx, -(wb * db)); }
        tA1[2 * i] = da; tA2[2 * i] = da * da; tC2[2 * i] = S2;
        tB1[2 * i + 1] = db; tB2[2 * i + 1] = db * db;
    }
    double A1, B1, A2, B2, C2;
    if (c->L->kind == 4) {
        /* lane partial over the lane's units, ascending, one term per unit (no zero slots), then the xor tree */
        double uA1[KO_MAXD], uB1[KO_MAXD], uA2[KO_MAXD], uB2[KO_MAXD], uC2[KO_MAXD];
        for (int i = 0; i < R; ++i) { uA1[i] = tA1[2 * i]; uA2[i] = tA2[2 * i]; uC2[i] = tC2[2 * i]; uB1[i] = tB1[2 * i + 1]; uB2[i] = tB2[2 * i + 1]; }
        const ko_layout U = { 0, c->L->G, c->L->E / 2 };      /* unit r on lane r / (E/2): the contiguous rule */
        A1 = ko_reduce(&U, uA1, R); B1 = ko_reduce(&U, uB1, R);
        /* the sums of squares accumulate the products themselves: partial = fma(d, d, partial) (klara_hiert.h hier_eval) */
        A2 = ko_reduce_prod(&U, uA1, uA1, R); B2 = ko_reduce_prod(&U, uB1, uB1, R); C2 = ko_reduce(&U, uC2, R);
        (void)uA2; (void)uB2;
    } else {
        A1 = ko_reduce(c->L, tA1, D); B1 = ko_reduce(c->L, tB1, D);
        A2 = ko_reduce(c->L, tA2, D); B2 = ko_reduce(c->L, tB2, D); C2 = ko_reduce(c->L, tC2, D);
    }
    const double RT = (double)R * (double)T, Rd = (double)R;
    if (g) {
        g[2 * R] = kd_fma(wa, A1, -(p0 * ac));
        g[2 * R + 1] = kd_fma(wb, B1, -(p0 * bc));
        g[2 * R + 2] = kd_fma(2.0 * b0, wc, kd_fma(wc, C2, -RT) - 2.0 * a0);
        g[2 * R + 3] = kd_fma(2.0 * b0, wa, kd_fma(wa, A2, -Rd) - 2.0 * a0);
        g[2 * R + 4] = kd_fma(2.0 * b0, wb, kd_fma(wb, B2, -Rd) - 2.0 * a0);
    }
    const double l_c = (-RT * sc - 0.5 * (wc * C2)) + (-2.0 * a0 * sc - b0 * wc);
    const double l_a = (-Rd * sa - 0.5 * (wa * A2)) + (-2.0 * a0 * sa - b0 * wa);
    const double l_b = (-Rd * sb - 0.5 * (wb * B2)) + (-2.0 * a0 * sb - b0 * wb);
    return ((l_c + l_a) + l_b) - (0.5 * p0) * (ac * ac + bc * bc);
}

/* KLARA_TARGET_CUSTOM: the user's closures (BasicContMuvParameter(:p, logtarget=f, gradlogtarget=g),
 * BasicContMuvParameter.jl:174-201,264-279).  The test harness compiles the same C text the device path compiles
 * (tests/oracle_ffi.py, gcc -ffp-contract=off with detmath.h) and registers the two functions here. */
typedef double (*ko_user_lt_fn)(const double* x, int D, const double* data, long long ndata);
typedef void (*ko_user_grad_fn)(const double* x, int D, const double* data, long long ndata, double* g);
static ko_user_lt_fn ko_user_lt = NULL;
static ko_user_grad_fn ko_user_grad = NULL;
void ko_set_custom_target(ko_user_lt_fn lt, ko_user_grad_fn grad) { ko_user_lt = lt; ko_user_grad = grad; }
/* SMMALA: the user's klara_user_tensorlogtarget (the metric G(x), D x D row-major, upper triangle read) */
typedef void (*ko_user_tensor_fn)(const double* x, int D, const double* data, long long ndata, double* G);
static ko_user_tensor_fn ko_user_tensor = NULL;
void ko_set_custom_tensor(ko_user_tensor_fn tensor) { ko_user_tensor = tensor; }

/* The same closures given one element pair at a time (`#define KLARA_USER_PAIR_TARGET 1`, include/klara_hip.h):
 *     lt(x) = sum over pairs P of klara_user_pair(x[2P], x[2P+1], P, ...),   which also returns the pair's two partial derivatives.
 * The device evaluates it on the pair-transposed layout (klara_diagt.h USERPAIR): pair P on lane P % G, a lane adds ITS pairs' terms in
 * ascending order, then the xor butterfly — ko_reduce_pairs; the sums run over -term and lt = 0 - sum, the same bits as the sum of
 * the terms.  The missing half of an odd D's last pair is passed as 0 and its derivative is dropped. */
typedef double (*ko_user_pair_fn)(double x0, double x1, int pair, int D, const double* data, long long ndata, double* g0, double* g1);
static ko_user_pair_fn ko_user_pair = NULL;
void ko_set_custom_pair_target(ko_user_pair_fn f) { ko_user_pair = f; }
static double ko_reduce_pairs(const ko_layout* L, const double* pt, int npairs)
{
    double part[64], nw[64];
    const int G = L->G;
    for (int l = 0; l < G; ++l) part[l] = 0.0;
    for (int P = 0; P < npairs; ++P) part[P % G] = part[P % G] + pt[P];
    for (int m = 1; m < G; m <<= 1) {
        for (int l = 0; l < G; ++l) nw[l] = part[l] + part[l ^ m];
        memcpy(part, nw, sizeof(double) * (size_t)G);
    }
    return part[0];
}
static double ko_pair_eval(const ko_target_ctx* c, const double* x, double* g)
{
    const klara_desc* d = c->d;
    const int D = d->ndims, np = (D + 1) / 2;
    double nt[KO_MAXD];
    for (int P = 0; P < np; ++P) {
        const int full = 2 * P + 1 < D;
        double g0 = 0.0, g1 = 0.0;
        const double u = ko_user_pair(x[2 * P], full ? x[2 * P + 1] : 0.0, P, D, d->custom_data, (long long)d->custom_ndata, &g0, &g1);
        nt[P] = -u;
        if (g) { g[2 * P] = g0; if (full) g[2 * P + 1] = g1; }
    }
    return 0.0 - ko_reduce_pairs(c->L, nt, np);
}

/* logtarget!(state) — BasicContMuvParameter.jl:174-201 */
static double ko_logtarget(const ko_target_ctx* c, const double* x, double* scratch)
{
    switch (c->d->target) {
    case KLARA_TARGET_GAUSS_DIAG: return ko_diag_lt(c, x, scratch);
    case KLARA_TARGET_GAUSS_DENSE: {
        double g[KO_MAXD];
        ko_dense_grad(c, x, g);
        return ko_dense_lt_from_grad(c, x, g, scratch);
    }
    case KLARA_TARGET_HIER_NORMAL: return ko_hier_eval(c, x, NULL, scratch);
    case KLARA_TARGET_CUSTOM:
        if (ko_user_pair) return ko_pair_eval(c, x, NULL);
        return ko_user_lt(x, c->d->ndims, c->d->custom_data, (long long)c->d->custom_ndata);
    default: { double lt; ko_logit_eval(c, x, &lt, NULL); return lt; }
    }
}
/* gradlogtarget!(state) — BasicContMuvParameter.jl:192-201 */
static void ko_gradlogtarget(const ko_target_ctx* c, const double* x, double* g)
{
    switch (c->d->target) {
    case KLARA_TARGET_GAUSS_DIAG: ko_diag_grad(c, x, g); break;
    case KLARA_TARGET_GAUSS_DENSE: ko_dense_grad(c, x, g); break;
    case KLARA_TARGET_HIER_NORMAL: { double sc[1]; (void)ko_hier_eval(c, x, g, sc); break; }
    case KLARA_TARGET_CUSTOM:      /* (MH / slice jobs need no gradient closure; their init evaluates none) */
        if (ko_user_pair) { (void)ko_pair_eval(c, x, g); break; }
        if (ko_user_grad) ko_user_grad(x, c->d->ndims, c->d->custom_data, (long long)c->d->custom_ndata, g);
        else for (int i = 0; i < c->d->ndims; ++i) g[i] = 0.0;
        break;
    default: ko_logit_eval(c, x, NULL, g); break;
    }
}
/* uptogradlogtarget!(state) = logtarget! then gradlogtarget! — BasicContMuvParameter.jl:270-274 */
static double ko_uptograd(const ko_target_ctx* c, const double* x, double* g, double* scratch)
{
    switch (c->d->target) {
    case KLARA_TARGET_GAUSS_DIAG: ko_diag_grad(c, x, g); return ko_diag_lt(c, x, scratch);
    case KLARA_TARGET_GAUSS_DENSE: ko_dense_grad(c, x, g); return ko_dense_lt_from_grad(c, x, g, scratch);
    case KLARA_TARGET_HIER_NORMAL: return ko_hier_eval(c, x, g, scratch);
    case KLARA_TARGET_CUSTOM: { const double lt = ko_logtarget(c, x, scratch); ko_gradlogtarget(c, x, g); return lt; }
    default: { double lt; ko_logit_eval(c, x, &lt, g); return lt; }
    }
}

/* ------------------------------------------------------------------ random draws */
static void ko_normals(uint64_t seed, uint64_t chain, uint64_t t, int D, double* z)
{
    /* element pair j <- half (j >> 3) & 1 of block slot (j & 7) + 8 (j >> 4): detmath.h kd_normal_pair_at */
    for (int j = 0; 2 * j < D; ++j) {
        double z0, z1, u1, lg1;
        kd_normal_pair_at(seed, chain, t, (uint32_t)j, (uint32_t)((D + 1) / 2), &z0, &z1, &u1, &lg1);
        z[2 * j] = z0;
        if (2 * j + 1 < D) z[2 * j + 1] = z1;
    }
}
static double ko_accept_uniform(uint64_t seed, uint64_t chain, uint64_t t, int D)
{
    return kd_accept_uniform(kd_stream_block(seed, chain, t, (uint32_t)((D + 1) / 2)));
}

/* ------------------------------------------------------------------ per-chain state bundle */
typedef struct ko_tune { double step; int64_t accepted, proposed, totproposed; double rate; } ko_tune;

static int ko_isfinite(double v) { return v == v && v - v == 0.0; }

/* rate!(tune), reset_burnin!(tune) — src/tuners/tuners.jl:27-32; tune!(tune, tuner) —
 * src/tuners/AcceptanceRateMCTuner.jl:46.  pool = number of chains sharing the tune (1 per-chain). */
static void ko_tuning_block(const klara_desc* d, ko_tune* tn, int cnt, int64_t pool)
{
    if (!cnt) return;
    if (tn->totproposed <= d->burnin && (tn->proposed % d->period) == 0) {   /* MALA.jl:131 / HMC.jl:204 */
        tn->rate = (double)tn->accepted / (double)(tn->proposed * pool);      /* rate!                    */
        if (d->tuner == KLARA_TUNER_ACCEPT_RATE && d->sampler != KLARA_SAMPLER_MH)
            tn->step *= d->tuner_score == 1 ? ko_erf_rate_score(tn->rate - d->targetrate, d->score_k)
                                            : ko_logistic_rate_score(tn->rate - d->targetrate, d->score_k); /* tune! */
        tn->totproposed += tn->proposed;                                      /* reset_burnin!            */
        tn->accepted = 0; tn->proposed = 0; tn->rate = NAN;
    }
}

/* CNT predicate ("count proposals/accepts"): MH.jl(iterate):73 `tuner.verbose`;
 * MALA.jl(iterate):79 / HMC.jl(iterate):129-133 `(Vanilla && verbose) || AcceptanceRate`. */
static int ko_cnt(const klara_desc* d)
{
    if (d->sampler == KLARA_SAMPLER_MH || d->sampler == KLARA_SAMPLER_SLICE || d->sampler == KLARA_SAMPLER_RAM || d->sampler == KLARA_SAMPLER_AM)
        return d->verbose != 0;                                          /* iterate/RAM.jl:68, iterate/AM.jl:80: tuner.verbose */
    return (d->tuner == KLARA_TUNER_VANILLA && d->verbose) || d->tuner == KLARA_TUNER_ACCEPT_RATE ||
           (d->tuner == KLARA_TUNER_DUAL_AVERAGING && d->verbose);      /* HMC.jl(iterate):129-133 */
}

/* ------------------------------------------------------------------ transitions */
/* iterate!(job, MH, Multivariate) — src/samplers/iterate/MH.jl:72-124, symmetric normalised branch */
static int ko_mh(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double z[KO_MAXD], xp[KO_MAXD], scratch[KO_MAXD];
    ko_normals(d->seed, chain, t, D, z);
    for (int i = 0; i < D; ++i) xp[i] = x[i] + d->mh_sigma[i] * z[i];  /* :79 rand(MvNormal(x, sigma)) */
    const double ltp = ko_logtarget(c, xp, scratch);                    /* :81 */
    const double ratio = ltp - *lt;                                     /* :83 */
    int acc = ratio > 0.0;                                              /* :97 */
    if (!acc) acc = ratio > kd_log_u01(ko_accept_uniform(d->seed, chain, t, D));
    if (acc) { memcpy(x, xp, sizeof(double) * (size_t)D); *lt = ltp; }  /* :98-100 */
    return acc;
}

/* iterate!(job, MALA, Multivariate) — src/samplers/iterate/MALA.jl:78-128 */
static int ko_mala(const ko_target_ctx* c, uint64_t chain, uint64_t t, double h,
                   double* x, double* g, double* lt)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double z[KO_MAXD], mu[KO_MAXD], xp[KO_MAXD], gp[KO_MAXD], s1[KO_MAXD], s2[KO_MAXD], scratch[KO_MAXD];
    ko_normals(d->seed, chain, t, D, z);
    const double halfh = 0.5 * h, sq = sqrt(h);
    /* DEVIATION from the literal `abs2.(...)/step` of MALA.jl:90,92: the quotient is formed as abs2(.)*(1/step)
     * (<= 1 ulp per element from the literal expression) because the gfx950 kernels do so to save two f64
     * divisions per element; the reference's own summation order is unspecified anyway (header). */
    const double inv_h = 1.0 / h, half_inv_h = 0.5 * inv_h;   /* 0.5*(abs2(.)/h) as abs2(.)*(0.5/h): the halving is exact */
    for (int i = 0; i < D; ++i) mu[i] = x[i] + halfh * g[i];            /* :83 */
    for (int i = 0; i < D; ++i) xp[i] = mu[i] + sq * z[i];              /* :84 */
    const double ltp = ko_uptograd(c, xp, gp, scratch);                  /* :86 */
    double ratio = ltp - *lt;                                            /* :88 */
    const int literal = ko_is_literal();
    for (int i = 0; i < D; ++i) { const double q = mu[i] - xp[i]; s1[i] = literal ? 0.5 * ((q * q) / h) : (q * q) * half_inv_h; }
    ratio += ko_reduce(c->L, s1, D);                                     /* :90 */
    for (int i = 0; i < D; ++i) {
        const double mup = xp[i] + halfh * gp[i];                        /* :91 */
        const double q = mup - x[i];
        s2[i] = literal ? 0.5 * ((q * q) / h) : (q * q) * half_inv_h;
    }
    ratio -= ko_reduce(c->L, s2, D);                                     /* :92 */
    int acc = ratio > 0.0;                                               /* :94 */
    if (!acc) acc = ratio > kd_log_u01(ko_accept_uniform(d->seed, chain, t, D));
    if (acc) {                                                           /* :95-105 */
        memcpy(x, xp, sizeof(double) * (size_t)D);
        memcpy(g, gp, sizeof(double) * (size_t)D);
        *lt = ltp;
    }
    return acc;
}

/* iterate!(job, HMC, Multivariate) — src/samplers/iterate/HMC.jl:124-201;
 * leapfrog! — src/samplers/samplers.jl:122-134; hamiltonian — samplers.jl:103 */
static int ko_hmc(const ko_target_ctx* c, uint64_t chain, uint64_t t, double eps, int64_t nleaps,
                  double* x, double* g, double* lt, double* a_out)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double p[KO_MAXD], xp[KO_MAXD], gp[KO_MAXD], sc[KO_MAXD], scratch[KO_MAXD];
    ko_normals(d->seed, chain, t, D, p);                                 /* :135 */
    for (int i = 0; i < D; ++i) sc[i] = p[i] * p[i];
    const double H0 = *lt - 0.5 * ko_reduce(c->L, sc, D);                /* :137 */
    memcpy(xp, x, sizeof(double) * (size_t)D);                           /* :139 */
    memcpy(gp, g, sizeof(double) * (size_t)D);                           /* :140 */
    const double halfe = 0.5 * eps;
    /* DELIBERATE DEVIATION, as every HMC kernel of the library runs it: leapfrog! L times
     * (samplers.jl:122-134: p = p + eps/2 g; x = x + eps p; g = grad(x); p = p + eps/2 g, each an unfused a + b*c) in its merged
     * form — the closing half-kick of step l and the opening half-kick of step l + 1 use the same gradient and are ONE update
     * p += eps g, and every update is one fma.  The same trajectory in exact arithmetic; <= 1 ulp per update from the literal form. */
    if (ko_is_literal()) {
        for (int64_t l = 0; l < nleaps; ++l) {                           /* :146-155, leapfrog! as written */
            for (int i = 0; i < D; ++i) p[i] = p[i] + halfe * gp[i];     /* samplers.jl:130 */
            for (int i = 0; i < D; ++i) xp[i] = xp[i] + eps * p[i];      /* samplers.jl:131 */
            ko_gradlogtarget(c, xp, gp);                                 /* samplers.jl:132 */
            for (int i = 0; i < D; ++i) p[i] = p[i] + halfe * gp[i];     /* samplers.jl:133 */
        }
    } else {
    for (int i = 0; i < D; ++i) p[i] = kd_fma(halfe, gp[i], p[i]);       /* samplers.jl:130 of the first step */
    for (int64_t l = 0; l < nleaps; ++l) {                               /* :146-155 */
        for (int i = 0; i < D; ++i) xp[i] = kd_fma(eps, p[i], xp[i]);    /* samplers.jl:131 */
        ko_gradlogtarget(c, xp, gp);                                     /* samplers.jl:132 */
        const double kf = l + 1 < nleaps ? eps : halfe;                  /* :133 of this step (+ :130 of the next) */
        for (int i = 0; i < D; ++i) p[i] = kd_fma(kf, gp[i], p[i]);
    }
    }
    double ltp;                                                          /* :157 logtarget!(x') */
    if (d->target == KLARA_TARGET_GAUSS_DENSE) ltp = ko_dense_lt_from_grad(c, xp, gp, scratch);
    else ltp = ko_logtarget(c, xp, scratch);
    for (int i = 0; i < D; ++i) sc[i] = p[i] * p[i];
    const double H1 = ltp - 0.5 * ko_reduce(c->L, sc, D);                /* :159 */
    const double ratio = H1 - H0;                                        /* :161 */
    const double e = kd_exp(ratio);
    const double a = 1.0 < e ? 1.0 : e;                                  /* :163 min(1., exp(ratio)) */
    const double u = ko_accept_uniform(d->seed, chain, t, D);            /* :165 rand() always drawn */
    const int acc = u < a;
    if (a_out) *a_out = a;
    if (acc) {
        memcpy(x, xp, sizeof(double) * (size_t)D);
        memcpy(g, gp, sizeof(double) * (size_t)D);
        *lt = ltp;
    }
    return acc;
}

/* iterate!(job, SliceSampler, Multivariate) — src/samplers/iterate/SliceSampler.jl:60-109 */
static int ko_slice(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt, int* stuck)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double tmp[KO_MAXD], scratch[KO_MAXD];
    for (int i = 0; i < D; ++i) {                                        /* :65 */
        const uint32_t base = (uint32_t)i << KO_SLICE_ATT_BITS;
        const kd_u32x4 b0 = kd_stream_block(d->seed, chain, t, base);
        const double logu = kd_log_u01(kd_uniform_xy(b0)) + *lt;             /* :66 */
        const double ru = kd_uniform_zw(b0);                             /* :71 */
        const double w = d->slice_widths[i], xi = x[i];
        double Li = xi - ru * w;                                         /* :72 */
        double Ri = xi + (1.0 - ru) * w;                                 /* :73 */
        memcpy(tmp, x, sizeof(double) * (size_t)D);
        if (d->slice_stepout) {                                          /* :75-89 */
            int guard = 0;
            tmp[i] = Li;
            double l = ko_logtarget(c, tmp, scratch);
            while (l > logu) {
                Li -= w; tmp[i] = Li; l = ko_logtarget(c, tmp, scratch);
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
            guard = 0;
            tmp[i] = Ri;
            l = ko_logtarget(c, tmp, scratch);
            while (l > logu) {
                Ri += w; tmp[i] = Ri; l = ko_logtarget(c, tmp, scratch);
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
        }
        double xprime = xi;
        for (uint32_t a = 1;; ++a) {                                     /* :91-106 */
            if (a > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            const double u = kd_slice_attempt_uniform(d->seed, chain, t, base, a);
            xprime = u * (Ri - Li) + Li;                                 /* :92-93 */
            tmp[i] = xprime;
            *lt = ko_logtarget(c, tmp, scratch);                         /* :94 */
            if (*lt > logu) break;                                       /* :95 */
            if (xprime > xi) Ri = xprime;                                /* :98 */
            else if (xprime < xi) Li = xprime;                           /* :100 */
            else { *stuck = 1; return 0; }                               /* :102 */
        }
        x[i] = xprime;                                                   /* :108 */
    }
    return 1;
}

/* The same update on the diagonal Gaussian in the pair-transposed layout (kind 3), where the kernels compare in DIFFERENCE form (deliberate
 * deviation (8)): the target is a sum of per-coordinate terms t_i = w_i (x_i - mu_i)^2, so
 *     lt(candidate) > log(rand()) + lt   <=>   t_i(current) - t_i(candidate) > log(rand())
 * and the coordinates of a transition do not depend on each other (every lane of the kernel updates its own).  The new state's log-target is one full
 * evaluation in the layout's order at the end.  ko_set_literal(1) takes this back (ko_slice above: a full evaluation per probe). */
static int ko_slice_diag_delta(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt, int* stuck)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double scratch[KO_MAXD];
    for (int i = 0; i < D; ++i) {                                        /* :65 */
        const uint32_t base = (uint32_t)i << KO_SLICE_ATT_BITS;
        const kd_u32x4 b0 = kd_stream_block(d->seed, chain, t, base);
        const double lgu = kd_log_u01(kd_uniform_xy(b0));                /* :66 log(rand()) */
        const double ru = kd_uniform_zw(b0);                             /* :71 */
        const double w = d->slice_widths[i], xi = x[i];
        const double mu = d->gauss_mu ? d->gauss_mu[i] : 0.0, wt = d->gauss_w ? d->gauss_w[i] : 1.0;
#define KO_TERM(v) (wt * (((v) - mu) * ((v) - mu)))
        const double tcur = KO_TERM(xi);
        double Li = xi - ru * w;                                         /* :72 */
        double Ri = xi + (1.0 - ru) * w;                                 /* :73 */
        if (d->slice_stepout) {                                          /* :75-89 */
            int guard = 0;
            while (tcur - KO_TERM(Li) > lgu) {
                Li -= w;
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
            guard = 0;
            while (tcur - KO_TERM(Ri) > lgu) {
                Ri += w;
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
        }
        double xprime = xi;
        for (uint32_t a = 1;; ++a) {                                     /* :91-106 */
            if (a > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            const double u = kd_slice_attempt_uniform(d->seed, chain, t, base, a);
            xprime = u * (Ri - Li) + Li;                                 /* :92-93 */
            if (tcur - KO_TERM(xprime) > lgu) break;                     /* :94-95 */
            if (xprime > xi) Ri = xprime;                                /* :98 */
            else if (xprime < xi) Li = xprime;                           /* :100 */
            else { *stuck = 1; return 0; }                               /* :102 */
        }
#undef KO_TERM
        x[i] = xprime;                                                   /* :108 */
    }
    *lt = ko_logtarget(c, x, scratch);
    return 1;
}

/* The same update for a PAIR CLOSURE in the pair-transposed layout (round 6: k_diagt<SLICE, .., USERPAIR>): lt = sum over pairs P of f_P(x_2P, x_2P+1), so a probe of
 * coordinate i = 2P (+ 1) changes the term of pair P only and every comparison of the update, lt(candidate) > log(rand()) + lt, is made on that term:
 *     n_P(current) - n_P(candidate) > log(rand())          with n_P = -f_P (the "negative term" the kernels sum)
 * — the deviation (8) of the diagonal target, for the same reason (the other pairs cancel; a lane updates its own pairs).  Coordinate 2P + 1 sees the new
 * x_2P (ascending coordinates, :65, :108).  The new state's log-target is one full evaluation in the layout's order.  ko_set_literal(1) takes this back. */
static int ko_slice_pair_delta(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt, int* stuck)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double scratch[KO_MAXD];
    for (int i = 0; i < D; ++i) {                                        /* :65 */
        const uint32_t base = (uint32_t)i << KO_SLICE_ATT_BITS;
        const kd_u32x4 b0 = kd_stream_block(d->seed, chain, t, base);
        const double lgu = kd_log_u01(kd_uniform_xy(b0));                /* :66 log(rand()) */
        const double ru = kd_uniform_zw(b0);                             /* :71 */
        const double w = d->slice_widths[i], xi = x[i];
        const int P = i >> 1, full = 2 * P + 1 < D, second = i & 1;
        const double other = second ? x[2 * P] : (full ? x[2 * P + 1] : 0.0);
        double g0_, g1_;
#define KO_TERM(v) (-ko_user_pair(second ? other : (v), second ? (v) : other, P, D, d->custom_data, (long long)d->custom_ndata, &g0_, &g1_))
        const double tcur = KO_TERM(xi);
        double Li = xi - ru * w;                                         /* :72 */
        double Ri = xi + (1.0 - ru) * w;                                 /* :73 */
        if (d->slice_stepout) {                                          /* :75-89 */
            int guard = 0;
            while (tcur - KO_TERM(Li) > lgu) {
                Li -= w;
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
            guard = 0;
            while (tcur - KO_TERM(Ri) > lgu) {
                Ri += w;
                if (++guard > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            }
        }
        double xprime = xi;
        for (uint32_t a = 1;; ++a) {                                     /* :91-106 */
            if (a > KO_SLICE_MAX_ATT) { *stuck = 1; return 0; }
            const double u = kd_slice_attempt_uniform(d->seed, chain, t, base, a);
            xprime = u * (Ri - Li) + Li;                                 /* :92-93 */
            if (tcur - KO_TERM(xprime) > lgu) break;                     /* :94-95 */
            if (xprime > xi) Ri = xprime;                                /* :98 */
            else if (xprime < xi) Li = xprime;                           /* :100 */
            else { *stuck = 1; return 0; }                               /* :102 */
        }
#undef KO_TERM
        x[i] = xprime;                                                   /* :108 */
    }
    *lt = ko_logtarget(c, x, scratch);
    return 1;
}

/* ------------------------------------------------------------------ SMMALA, RAM, AM: the samplers that carry a matrix per chain */
/* What such a chain carries beyond x, g and lt, as the caller of ko_init / ko_run holds it (NULL for the other samplers; SMMALA's factor
 * state is not here: it is formed from x and its gradient at the start of every ko_run call, as the kernels do at a launch start). */
typedef struct ko_sampler_state {
    double* ram_S;            /* RAM: nchains packed E x E lower factors, S_ij (i >= j) at ko_tri(j, i, E), the identity in the padding */
    int64_t* ram_skipped;     /* RAM: += the factor updates skipped (z . z or a pivot not a finite positive number), over all chains */
    double* am_C;             /* AM: nchains packed D x D upper triangles, C_ij (i <= j) at ko_tri(i, j, D) */
    double* am_mean;          /* AM: nchains x D, lastmean */
    double* am_mean2;         /* AM: nchains x D, secondlastmean */
    int64_t* am_fallbacks;    /* AM: += the transitions whose covariance did not factor (A2), over all chains */
    int64_t* softabs_sweeps;  /* SMMALA with the transform, may be NULL: [0] += metrics transformed, [1] += their sweeps, [2] = max(., most sweeps) */
} ko_sampler_state;

static int ko_matrix_sampler(int s) { return s == KLARA_SAMPLER_SMMALA || s == KLARA_SAMPLER_RAM || s == KLARA_SAMPLER_AM; }
static int ko_tri(int a, int b, int E) { return a * E - (a * (a - 1)) / 2 + (b - a); }

/* smmala_factor's loop nest (klara_kernels.h tri_factor), which ram_update and am_factor share (R4, A2): the packed n x n matrix A (upper
 * triangle, A_ji (j <= i) at ko_tri(j, i, n)) becomes its lower Cholesky factor in place, column by column.  1 when every pivot is a finite
 * positive number; a pivot that is not counts as 1. */
static int ko_tri_factor(int n, double* A)
{
    int ok = 1;
    for (int j = 0; j < n; ++j) {
        double sj = A[ko_tri(j, j, n)];
        for (int k = 0; k < j; ++k) sj = sj - A[ko_tri(k, j, n)] * A[ko_tri(k, j, n)];
        const int okj = sj > 0.0 && ko_isfinite(sj);
        ok = ok && okj;
        const double ljj = sqrt(okj ? sj : 1.0);
        const double rj = 1.0 / ljj;
        A[ko_tri(j, j, n)] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double a = A[ko_tri(j, i, n)];
            for (int k = 0; k < j; ++k) a = a - A[ko_tri(k, i, n)] * A[ko_tri(k, j, n)];
            A[ko_tri(j, i, n)] = a * rj;
        }
    }
    return ok;
}

/* a chain of one of the three samplers during a ko_run call */
typedef struct ko_smmala_state { double L[KO_MAXNT], r[KO_MAXE], f[KO_MAXE], ld; } ko_smmala_state;
typedef struct ko_chain {
    ko_smmala_state sm;       /* SMMALA: factor of the metric at x, its reciprocal diagonal, the drift G^-1 g, log det L */
    double* S;                /* RAM: this chain's factor */
    double *C, *m, *m2;       /* AM: this chain's covariance and means */
    int64_t cn[4];            /* counted during the call: RAM updates skipped, AM fallbacks, metrics transformed, their sweeps ... */
    int64_t maxsweeps;        /* ... and the most sweeps of one metric */
} ko_chain;

/* ---- SMMALA (klara_kernels.h step_smmala; iterate/SMMALA.jl) */
/* the butterflied upper triangle of X' diag(r (1 - r)) X over E padded columns (LogisticTarget::eval, NTRI > 0), or the upper triangle of a
 * user's tensor (CustomTarget::eval); no other target runs the softabs transform: NaNs */
void ko_smmala_metric(const klara_desc* d, const ko_layout* L, const double* x, double* gm)
{
    const int E = L->E, D = d->ndims, NT = E * (E + 1) / 2, n = d->logit_ndata;
    if (d->target == KLARA_TARGET_CUSTOM) {
        double gt[KO_MAXE * KO_MAXE];
        ko_user_tensor(x, D, d->custom_data, (long long)d->custom_ndata, gt);
        for (int a = 0; a < E; ++a) for (int b = a; b < E; ++b) gm[ko_tri(a, b, E)] = b < D ? gt[a * D + b] : 0.0;
        return;
    }
    if (d->smmala_softabs > 0.0) {
        for (int k = 0; k < NT; ++k) gm[k] = kd_u2d(0x7ff8000000000000ull);          /* (no other target runs the transform) */
        return;
    }
    const int RS = L->kind == 2 ? L->G : 1;
    double part[16][KO_MAXNT], nw[16][KO_MAXNT];
    for (int l = 0; l < RS; ++l) for (int k = 0; k < NT; ++k) part[l][k] = 0.0;
    for (int r = 0; r < n; ++r) {
        double row[KO_MAXE], xp = 0.0, sp, lg;
        for (int e = 0; e < E; ++e) row[e] = e < D ? d->logit_X[(size_t)r * D + e] : 0.0;
        for (int e = 0; e < E; ++e) xp = kd_fma(row[e], e < D ? x[e] : 0.0, xp);
        kd_softplus_logistic_rows(xp, &sp, &lg);
        const double wr = lg * (1.0 - lg);
        double* pl = part[r % RS];
        for (int a = 0; a < E; ++a) {
            const double ta = row[a] * wr;
            for (int b = a; b < E; ++b) pl[ko_tri(a, b, E)] = kd_fma(ta, row[b], pl[ko_tri(a, b, E)]);
        }
    }
    for (int m = 1; m < RS; m <<= 1) {
        for (int l = 0; l < RS; ++l) for (int k = 0; k < NT; ++k) nw[l][k] = part[l][k] + part[l ^ m][k];
        memcpy(part, nw, sizeof(part));
    }
    for (int k = 0; k < NT; ++k) gm[k] = part[0][k];
}

/* the metric's diagonal term beyond gm (T::metric_diag): I / lambda of the logistic target, nothing for a user's tensor */
static double ko_smmala_diag(const klara_desc* d) { return d->target == KLARA_TARGET_LOGISTIC ? 1.0 / d->logit_lambda : 0.0; }

/* klara_desc.smmala_softabs > 0: the metric with T::metric_diag added, transformed (klara_kernels.h smmala_softabs_metric); the
 * factorisation then adds nothing.  Returns the diagonal term that is left for the factorisation to add. */
static double ko_smmala_transform(const klara_desc* d, int E, double* gm, ko_chain* ch)
{
    const int D = d->ndims;
    const double diag = ko_smmala_diag(d);
    if (!(d->smmala_softabs > 0.0)) return diag;
    for (int j = 0; j < D; ++j) gm[ko_tri(j, j, E)] = gm[ko_tri(j, j, E)] + diag;
    double Q[KO_MAXE * KO_MAXE];
    const int sweeps = ksa_softabs_tri(gm, D, E, d->smmala_softabs, Q, 1);
    if (sweeps > ch->maxsweeps) ch->maxsweeps = sweeps;
    if (sweeps >= 0) { ch->cn[3] += sweeps; ch->cn[2] += 1; }
    return 0.0;
}

/* smmala_factor: G = L L' column by column; 1 when every pivot is a finite positive number */
static int ko_smmala_factor(const double* gm, int D, int E, double inv_lambda, ko_smmala_state* s)
{
    for (int j = 0; j < E; ++j) {
        s->L[ko_tri(j, j, E)] = j < D ? gm[ko_tri(j, j, E)] + inv_lambda : 1.0;
        for (int i = j + 1; i < E; ++i) s->L[ko_tri(j, i, E)] = (i < D && j < D) ? gm[ko_tri(j, i, E)] : 0.0;
    }
    const int pd = ko_tri_factor(E, s->L);
    double ld = 0.0;
    for (int j = 0; j < E; ++j) {
        const double ljj = s->L[ko_tri(j, j, E)];
        s->r[j] = 1.0 / ljj;
        ld = ld + kd_log(ljj);
    }
    s->ld = ld;
    return pd;
}
static void ko_smmala_solve_lt(const ko_smmala_state* s, int E, const double* z, double* v)
{
    for (int i = E - 1; i >= 0; --i) {
        double t = z[i];
        for (int k = i + 1; k < E; ++k) t = t - s->L[ko_tri(i, k, E)] * v[k];
        v[i] = t * s->r[i];
    }
}
static void ko_smmala_drift(ko_smmala_state* s, int E, const double* g)
{
    double y[KO_MAXE];
    for (int i = 0; i < E; ++i) {
        double t = g[i];
        for (int k = 0; k < i; ++k) t = t - s->L[ko_tri(k, i, E)] * y[k];
        y[i] = t * s->r[i];
    }
    ko_smmala_solve_lt(s, E, y, s->f);
}
static double ko_smmala_quad(const ko_smmala_state* s, int E, const double* d)
{
    double q = 0.0;
    for (int i = 0; i < E; ++i) {
        double w = s->L[ko_tri(i, i, E)] * d[i];
        for (int k = i + 1; k < E; ++k) w = w + s->L[ko_tri(i, k, E)] * d[k];
        q = q + w * w;
    }
    return q;
}

/* the factor state at x (padded to E) with gradient g: what the kernels form at a launch start and check at a start state (S5) */
static int ko_smmala_state_at(const ko_target_ctx* c, const double* x, const double* g, ko_chain* ch)
{
    const klara_desc* d = c->d;
    const int E = c->L->E, D = d->ndims;
    double gm[KO_MAXNT], gp[KO_MAXE];
    ko_smmala_metric(d, c->L, x, gm);
    for (int e = 0; e < E; ++e) gp[e] = e < D ? g[e] : 0.0;
    const double diag = ko_smmala_transform(d, E, gm, ch);
    const int pd = ko_smmala_factor(gm, D, E, diag, &ch->sm);
    ko_smmala_drift(&ch->sm, E, gp);
    return pd;
}

/* step_smmala for one chain: x, g (D), lt and the factor state are updated on acceptance */
static int ko_smmala(const ko_target_ctx* c, uint64_t chain, uint64_t t, double h, double* x, double* g, double* lt, ko_chain* ch)
{
    const klara_desc* d = c->d;
    const int E = c->L->E, D = d->ndims;
    ko_smmala_state* s = &ch->sm;
    double z[KO_MAXE], xe[KO_MAXE], mu[KO_MAXE], v[KO_MAXE], xp[KO_MAXE], dd[KO_MAXE], gp[KO_MAXE], gm[KO_MAXNT], scratch[KO_MAXD];
    for (int e = 0; e < KO_MAXE; ++e) { z[e] = 0.0; gp[e] = 0.0; }
    ko_normals(d->seed, chain, t, D, z);
    for (int e = 0; e < E; ++e) xe[e] = e < D ? x[e] : 0.0;
    const double halfh = 0.5 * h, sq = sqrt(h), inv_h = 1.0 / h, dlogh = (double)D * kd_log(h);
    for (int e = 0; e < E; ++e) mu[e] = xe[e] + halfh * s->f[e];
    ko_smmala_solve_lt(s, E, z, v);
    for (int e = 0; e < E; ++e) xp[e] = mu[e] + sq * v[e];
    for (int e = 0; e < E; ++e) dd[e] = xp[e] - mu[e];
    const double fwd = 0.5 * ((dlogh - 2.0 * s->ld) + ko_smmala_quad(s, E, dd) * inv_h);
    const double ltp = ko_uptograd(c, xp, gp, scratch);
    ko_smmala_metric(d, c->L, xp, gm);
    ko_smmala_state sn;
    const double diag = ko_smmala_transform(d, E, gm, ch);
    const int pd = ko_smmala_factor(gm, D, E, diag, &sn);
    ko_smmala_drift(&sn, E, gp);
    for (int e = 0; e < E; ++e) dd[e] = xe[e] - (xp[e] + halfh * sn.f[e]);
    const double rev = 0.5 * ((dlogh - 2.0 * sn.ld) + ko_smmala_quad(&sn, E, dd) * inv_h);
    double ratio = ltp - *lt;
    ratio += fwd;
    ratio -= rev;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(ko_accept_uniform(d->seed, chain, t, D));
    acc = acc && pd;
    if (acc) {
        memcpy(x, xp, sizeof(double) * (size_t)D);
        memcpy(g, gp, sizeof(double) * (size_t)D);
        *lt = ltp;
        *s = sn;
    }
    return acc;
}

/* ---- RAM (klara_kernels.h step_ram / ram_update; iterate/RAM.jl) */
/* iterate/RAM.jl:123-127: c = eta (min(1, exp(ratio)) - targetrate) / (z . z), eta = min(1, D count^-gamma), count = t + 1 (R3) */
double ko_ram_coef(int D, uint64_t t, double gamma, double targetrate, double ratio, double zz)
{
    double eta = (double)D * kd_exp(-gamma * kd_log((double)(t + 1ull)));
    eta = eta < 1.0 ? eta : 1.0;
    const double ap = ratio >= 0.0 ? 1.0 : (ko_isfinite(ratio) ? kd_exp(ratio) : 0.0);
    return eta * (ap - targetrate) / zz;
}

/* ram_update from c on: A = S S' + c w w' (R2), factored in place (R4).  S: the packed E x E lower factor, S_ij (i >= j) at ko_tri(j, i, E).
 * Returns 1 and the new factor, or 0 — S as it was — where z . z or a pivot is not a finite positive number. */
int ko_ram_update_c(int E, double c, double zz, const double* w, double* S)
{
    const int NT = E * (E + 1) / 2;
    double A[KO_MAXNT];
    for (int j = 0; j < E; ++j)
        for (int i = j; i < E; ++i) {
            double a = S[ko_tri(0, i, E)] * S[ko_tri(0, j, E)];
            for (int k = 1; k <= j; ++k) a = a + S[ko_tri(k, i, E)] * S[ko_tri(k, j, E)];
            A[ko_tri(j, i, E)] = a + (c * w[i]) * w[j];
        }
    const int ok = ko_tri_factor(E, A) && zz > 0.0 && ko_isfinite(zz);
    if (ok) memcpy(S, A, sizeof(double) * (size_t)NT);
    return ok;
}

/* step_ram for one chain: x (D) and lt are updated on acceptance, the factor S (packed, E padded) after every transition; z_out (E) and
 * c_out, where given, take what the transition drew and formed */
static int ko_ram(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt, ko_chain* ch, double* z_out, double* c_out)
{
    const klara_desc* d = c->d;
    const int E = c->L->E, D = d->ndims;
    double* S = ch->S;
    double z[KO_MAXE], w[KO_MAXE], xp[KO_MAXE], zz = 0.0, scratch[KO_MAXD];
    for (int e = 0; e < KO_MAXE; ++e) z[e] = 0.0;
    ko_normals(d->seed, chain, t, D, z);
    for (int e = 0; e < E; ++e) zz = zz + z[e] * z[e];
    for (int i = 0; i < E; ++i) {                                   /* R1 */
        double a = S[ko_tri(0, i, E)] * z[0];
        for (int k = 1; k <= i; ++k) a = a + S[ko_tri(k, i, E)] * z[k];
        w[i] = a;
    }
    for (int e = 0; e < E; ++e) xp[e] = (e < D ? x[e] : 0.0) + w[e];
    const double ltp = ko_logtarget(c, xp, scratch);
    const double ratio = ltp - *lt;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(ko_accept_uniform(d->seed, chain, t, D));
    if (acc) { memcpy(x, xp, sizeof(double) * (size_t)D); *lt = ltp; }
    const double cf = ko_ram_coef(D, t, d->ram_gamma, d->ram_targetrate, ratio, zz);
    if (z_out) { memcpy(z_out, z, sizeof(double) * (size_t)E); *c_out = cf; }
    if (!ko_ram_update_c(E, cf, zz, w, S)) ch->cn[0] += 1;
    return acc;
}

/* ---- AM (klara_kernels.h step_am / am_covariance / am_factor; iterate/AM.jl): plain loops over the D elements — the kernel's padding to
 * E elements may change no bit (A5) */
/* the component selector of transition t: words (z, w) of the accept block, slot ceil(D / 2) */
double ko_am_selector(uint64_t seed, uint64_t chain, uint64_t t, int D)
{
    return kd_uniform_zw(kd_stream_block(seed, chain, t, (uint32_t)((D + 1) >> 1)));
}

/* covariance!(C, C, k, x, lastmean, secondlastmean), stats/covariance.jl:6-19, on the packed upper triangle (C_ij, i <= j, at ko_tri(i, j, D)) */
void ko_am_covariance(int D, int64_t k, const double* x, const double* m, const double* m2, double* C)
{
    const double kf = (double)k, km1 = (double)(k - 1), nk1 = (double)(-(k + 1));
    for (int i = 0; i < D; ++i) {
        const double a = nk1 * m[i], b = kf * m2[i];
        for (int j = i; j < D; ++j) {
            double c = km1 * C[ko_tri(i, j, D)];
            c = c + x[i] * x[j];
            c = c + a * m[j];
            c = c + b * m2[j];
            C[ko_tri(i, j, D)] = c / kf;
        }
    }
}

/* L = chol(corescale C), lower, L_ji (j >= i) at ko_tri(i, j, D); 1, or 0 where a pivot is not a finite positive number (A2) */
int ko_am_factor(int D, double corescale, const double* C, double* A)
{
    for (int k = 0; k < D * (D + 1) / 2; ++k) A[k] = corescale * C[k];
    return ko_tri_factor(D, A);
}

/* step_am for one chain: x (D) and lt are updated on acceptance; C (packed), m, m2 as the kernel keeps them */
static int ko_am(const ko_target_ctx* c, uint64_t chain, uint64_t t, double* x, double* lt, ko_chain* ch)
{
    const klara_desc* d = c->d;
    const int D = d->ndims;
    double *C = ch->C, *m = ch->m, *m2 = ch->m2;
    const int64_t count = (int64_t)t + 1;
    const double sqrtminor = sqrt(d->am_minorscale), w1 = 1.0 - d->am_c;
    double z[KO_MAXE], xp[KO_MAXE], scratch[KO_MAXD];
    for (int e = 0; e < KO_MAXE; ++e) { z[e] = 0.0; xp[e] = 0.0; }
    ko_normals(d->seed, chain, t, D, z);
    if (count > d->am_t0) {
        double Lf[KO_MAXNT];
        ko_am_covariance(D, count - 2, x, m, m2, C);
        const int ok = ko_am_factor(D, d->am_corescale, C, Lf);
        if (!ok) ch->cn[1] += 1;
        const int core = ok && ko_am_selector(d->seed, chain, t, D) < w1;
        for (int i = 0; i < D; ++i) {
            double a = Lf[ko_tri(0, i, D)] * z[0];
            for (int k = 1; k <= i; ++k) a = a + Lf[ko_tri(k, i, D)] * z[k];
            xp[i] = x[i] + (core ? a : sqrtminor * z[i]);
        }
    } else {
        for (int e = 0; e < D; ++e) xp[e] = x[e] + sqrtminor * z[e];
    }
    const double ltp = ko_logtarget(c, xp, scratch);
    const double ratio = ltp - *lt;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(ko_accept_uniform(d->seed, chain, t, D));
    if (acc) { memcpy(x, xp, sizeof(double) * (size_t)D); *lt = ltp; }
    const double cm1 = (double)(count - 1), cf = (double)count;
    for (int e = 0; e < D; ++e) { m2[e] = m[e]; m[e] = (cm1 * m[e] + x[e]) / cf; }
    return acc;
}

/* ---- the three samplers inside ko_init / ko_run */
/* what the kernels serve (klara_plan.h smmala_eligible / ram_eligible / am_eligible): E <= 8 padded elements, and the state that RAM and AM need */
static int ko_matrix_check(const klara_desc* d, const ko_layout* L, const ko_sampler_state* ss)
{
    if (L->E > KO_MAXE || d->ndims > L->E || d->ndims < 1) return KLARA_ERR_UNSUPPORTED;
    if (d->sampler == KLARA_SAMPLER_RAM && !(ss && ss->ram_S)) return KLARA_ERR_INVALID_ARG;
    if (d->sampler == KLARA_SAMPLER_AM && !(ss && ss->am_C && ss->am_mean && ss->am_mean2)) return KLARA_ERR_INVALID_ARG;
    if (d->sampler == KLARA_SAMPLER_SMMALA && d->target == KLARA_TARGET_CUSTOM && !ko_user_tensor) return KLARA_ERR_INVALID_ARG;
    return KLARA_OK;
}
/* chain n at the start of a ko_run call */
static void ko_chain_begin(const ko_target_ctx* c, const ko_sampler_state* ss, int64_t n, const double* x, const double* g, ko_chain* ch)
{
    const int D = c->d->ndims, E = c->L->E;
    memset(ch->cn, 0, sizeof ch->cn); ch->maxsweeps = 0;
    if (c->d->sampler == KLARA_SAMPLER_SMMALA) (void)ko_smmala_state_at(c, x, g, ch);
    else if (c->d->sampler == KLARA_SAMPLER_RAM) ch->S = ss->ram_S + n * (E * (E + 1) / 2);
    else { ch->C = ss->am_C + n * (D * (D + 1) / 2); ch->m = ss->am_mean + n * D; ch->m2 = ss->am_mean2 + n * D; }
}
/* the counts of a call, summed over its chains, go out once */
static void ko_counts_out(const ko_sampler_state* ss, const int64_t cn[4], int64_t maxsweeps)
{
    if (!ss) return;
    if (ss->ram_skipped) *ss->ram_skipped += cn[0];
    if (ss->am_fallbacks) *ss->am_fallbacks += cn[1];
    if (ss->softabs_sweeps) {
        ss->softabs_sweeps[0] += cn[2]; ss->softabs_sweeps[1] += cn[3];
        if (maxsweeps > ss->softabs_sweeps[2]) ss->softabs_sweeps[2] = maxsweeps;
    }
}

/* Streaming batch means (klara_desc.bm_batchlen): mcvar(v, Val{:bm}) of src/stats/variance/mcvar.jl:35-41 takes
 * var(batch means); the history-free form closes a batch from the running sums at its two boundaries and updates the mean
 * and the sum of squared deviations of the batch means in place (Welford).  n = nchains * D series, count = batches closed
 * before this call. */
void ko_bm_close(const double* sum, double* prev, double* mean, double* m2, int64_t n, int64_t count, int64_t batchlen)
{
    for (int64_t i = 0; i < n; ++i) {
        const double s = sum[i];
        const double b = (s - prev[i]) / (double)batchlen;
        prev[i] = s;
        const double delta = b - mean[i];
        const double mn = mean[i] + delta / (double)(count + 1);
        mean[i] = mn;
        m2[i] = m2[i] + delta * (b - mn);
    }
}

/* ------------------------------------------------------------------ public entry points */
static void ko_ctx_init(ko_target_ctx* c, const klara_desc* d, const ko_layout* L)
{
    c->d = d; c->L = L;
    c->logit_lpconst = 0.0;
    if (d->target == KLARA_TARGET_LOGISTIC)
        c->logit_lpconst = (double)d->ndims * kd_log(2.0 * 3.141592653589793 * d->logit_lambda);
}

/* initialize!(pstate, parameter, sampler) — MH.jl:72-85, MALA.jl:76-90, HMC.jl:106-120,
 * SliceSampler.jl:40-48; tuner_state — samplers.jl:29-45 (totproposed starts at tuner.period).  SMMALA, RAM, AM: klara_plan.h
 * sampler_needs_gradient / sampler_step0; the caller sets RAM's factor and AM's covariance and means (ss) to their start values; SMMALA's
 * metric must be positive definite at every start state (S5). */
int ko_init(const klara_desc* d, const ko_layout* L, const double* X, double* G, double* LT,
            double* step, int64_t* accepted, int64_t* proposed, int64_t* totproposed,
            double* da_epsbar, double* da_hbar, const ko_sampler_state* ss)
{
    ko_target_ctx c; ko_ctx_init(&c, d, L);
    const int D = d->ndims;
    if (D > KO_MAXD) return KLARA_ERR_UNSUPPORTED;
    if (ko_matrix_sampler(d->sampler)) { const int st = ko_matrix_check(d, L, ss); if (st != KLARA_OK) return st; }
    const int needgrad = d->sampler == KLARA_SAMPLER_MALA || d->sampler == KLARA_SAMPLER_HMC || d->sampler == KLARA_SAMPLER_SMMALA;
    int bad = 0;
    for (int64_t n = 0; n < d->nchains; ++n) {
        double scratch[KO_MAXD];
        const double* x = X + n * D;
        if (needgrad) {
            LT[n] = ko_uptograd(&c, x, G + n * D, scratch);
            for (int i = 0; i < D; ++i) if (!ko_isfinite(G[n * D + i])) bad = 1;
        } else {
            LT[n] = ko_logtarget(&c, x, scratch);
        }
        if (!ko_isfinite(LT[n])) bad = 1;
        const int pooled = d->tuner_mode == KLARA_TUNE_POOLED;
        if (!pooled || n == 0) {
            const int64_t k = pooled ? 0 : n;
            step[k] = (d->sampler == KLARA_SAMPLER_MH || d->sampler == KLARA_SAMPLER_RAM || d->sampler == KLARA_SAMPLER_AM) ? 1.0
                    : (d->sampler == KLARA_SAMPLER_MALA || d->sampler == KLARA_SAMPLER_SMMALA) ? d->driftstep
                    : d->sampler == KLARA_SAMPLER_HMC ? d->leapstep : NAN;
            accepted[k] = 0; proposed[k] = 0; totproposed[k] = d->period;
            /* tuner_state(parameter, sampler::HMC, tuner::DualAveragingMCTuner) — HMC.jl:124-133 */
            if (d->tuner == KLARA_TUNER_DUAL_AVERAGING && da_epsbar) { da_epsbar[k] = d->da_eps0bar; da_hbar[k] = d->da_h0bar; }
        }
    }
    if (!bad && d->sampler == KLARA_SAMPLER_SMMALA) {
        ko_chain ch = { .cn = { 0, 0, 0, 0 }, .maxsweeps = 0 };
        for (int64_t n = 0; n < d->nchains; ++n) if (!ko_smmala_state_at(&c, X + n * D, G + n * D, &ch)) bad = 1;
        ko_counts_out(ss, ch.cn, ch.maxsweeps);
    }
    return bad ? KLARA_ERR_NONFINITE_INIT : KLARA_OK;
}

/* x0 ~ N(0, I) from the init stream */
void ko_init_state_normal(const klara_desc* d, double* X)
{
    for (int64_t n = 0; n < d->nchains; ++n)
        ko_normals(d->seed, (uint64_t)(d->chain_offset + n), KO_INIT_TRANSITION, d->ndims, X + n * d->ndims);
}

/* the chain leaves the state xold after *held saved steps: fold them into the running sums (see ko_run) */
static void ko_fold(double* sum, double* sumsq, const double* xold, int D, int64_t* held)
{
    const double h = (double)*held;
    for (int i = 0; i < D; ++i) {
        sum[i] = sum[i] + h * xold[i];
        sumsq[i] = sumsq[i] + h * (xold[i] * xold[i]);
    }
    *held = 0;
}

/* the save rule of run(), BasicMCJob.jl:226-231: the 1-based step i = t + 1 is saved as column (i - burnin - 1) / thinning (see ko_run) */
static void ko_save(const klara_desc* d, int64_t n, int64_t t, const double* x, const double* g, double lt, int64_t* held,
                    double* hist, int64_t hist_cols, double* hist_lt, double* hist_g)
{
    const int D = d->ndims;
    const int64_t i1 = t + 1;                       /* 1-based step index i of run() */
    if (i1 > d->burnin && (i1 - d->burnin - 1) % d->thinning == 0 && i1 <= d->nsteps) {
        const int64_t col = (i1 - d->burnin - 1) / d->thinning;
        if (held) held[n] += 1;
        if (hist && col < hist_cols)
            memcpy(hist + ((size_t)col * (size_t)d->nchains + (size_t)n) * (size_t)D, x, sizeof(double) * (size_t)D);
        if (hist_lt && col < hist_cols) hist_lt[(size_t)col * (size_t)d->nchains + (size_t)n] = lt;
        if (hist_g && col < hist_cols)
            memcpy(hist_g + ((size_t)col * (size_t)d->nchains + (size_t)n) * (size_t)D, g, sizeof(double) * (size_t)D);
    }
}

/* one transition of one chain; returns accept flag (ch: the chain's state of SMMALA, RAM and AM, unused by the others) */
static int ko_transition(const ko_target_ctx* c, uint64_t gchain, uint64_t t, double step, int64_t nleaps,
                         double* x, double* g, double* lt, int* stuck, double* a_out, ko_chain* ch)
{
    const klara_desc* d = c->d;
    switch (d->sampler) {
    case KLARA_SAMPLER_MH: return ko_mh(c, gchain, t, x, lt);
    case KLARA_SAMPLER_MALA: return ko_mala(c, gchain, t, step, x, g, lt);
    case KLARA_SAMPLER_HMC: return ko_hmc(c, gchain, t, step, nleaps, x, g, lt, a_out);
    case KLARA_SAMPLER_SMMALA: return ko_smmala(c, gchain, t, step, x, g, lt, ch);
    case KLARA_SAMPLER_RAM: return ko_ram(c, gchain, t, x, lt, ch, NULL, NULL);
    case KLARA_SAMPLER_AM: return ko_am(c, gchain, t, x, lt, ch);
    default:
        if (c->L->kind == 3 && d->target == KLARA_TARGET_GAUSS_DIAG && !ko_is_literal()) return ko_slice_diag_delta(c, gchain, t, x, lt, stuck);
        if (c->L->kind == 3 && d->target == KLARA_TARGET_CUSTOM && ko_user_pair && !ko_is_literal()) return ko_slice_pair_delta(c, gchain, t, x, lt, stuck);
        return ko_slice(c, gchain, t, x, lt, stuck);
    }
}

/* run(job) — src/jobs/BasicMCJob.jl:212-244 for every chain.  t0 = number of transitions already
 * done (the global 0-based index of the first transition of this call).  Outputs may be NULL:
 *   accept_out[s * nchains + n]      diagnosticvalues[:accept] of transition t0+s
 *   sum/sumsq[n * D + i], held[n]    running sums over postrange steps (BasicMCRange.jl:17-36) in sojourn form: a saved step
 *                                    only counts (held[n] += 1); when the chain leaves a state x after `held` saved steps,
 *                                    sum += held * x and sumsq += held * (x * x) (one product, one sum each) and held = 0.
 *                                    The sums over the saved steps are sum + held * x (ko users form this view); a chain that
 *                                    moves at every saved step adds 1 * x each time — the plain running sum.  (Julia's
 *                                    mean(chain) sums the stored values in its own pairwise order, stats/mean.jl:7-11; the order
 *                                    here is build-defined like every other reduction, and it is what lets the device skip the
 *                                    running-sum traffic of chains that did not move.)
 *   naccept[n]                       accepted transitions
 *   hist[(col * nchains + n) * D + i] value saved as column `col` (save rule BasicMCJob.jl:226-231)
 * Tuner arrays have nchains entries (per-chain mode) or 1 entry (pooled mode).
 * ss: what the chains of SMMALA, RAM and AM carry beyond that (ko_sampler_state), NULL for the other samplers; `matrix` below is the one
 * test, uniform over the call, behind which all of its handling sits. */
int ko_run(const klara_desc* d, const ko_layout* L, double* X, double* G, double* LT,
           double* step, int64_t* accepted, int64_t* proposed, int64_t* totproposed,
           int64_t t0, int64_t nsteps, uint8_t* accept_out, double* sum, double* sumsq,
           uint64_t* naccept, double* hist, int64_t hist_cols, double* hist_lt, double* hist_g,
           double* da_epsbar, double* da_hbar, int64_t* held, const ko_sampler_state* ss)
{
    ko_target_ctx c; ko_ctx_init(&c, d, L);
    const int D = d->ndims;
    if (D > KO_MAXD) return KLARA_ERR_UNSUPPORTED;
    const int matrix = ko_matrix_sampler(d->sampler);
    if (matrix) { const int st = ko_matrix_check(d, L, ss); if (st != KLARA_OK) return st; }
    int64_t cn[4] = { 0, 0, 0, 0 }, maxsweeps = 0;      /* (matrix) counted over the chains of this call: ko_chain.cn */
    const int cnt = ko_cnt(d);
    const int pooled = d->tuner_mode == KLARA_TUNE_POOLED;
    const int da = d->tuner == KLARA_TUNER_DUAL_AVERAGING && d->sampler == KLARA_SAMPLER_HMC;
    /* sampler_state(...::DualAveragingMCTuner), HMC.jl:192-213: lambda = nleaps*leapstep, mu = log(10*step).
     * initialize_step! (samplers.jl:170-202) returns step0 in the reference as shipped: the proposal state's
     * logtarget is never evaluated (NaN), every comparison is false and the loop body (which would crash on the
     * undefined `moment`, samplers.jl:195) is never entered.  That effective behaviour is what is restated. */
    const double da_lambda = (double)d->nleaps * d->leapstep, da_mu = kd_log(10.0 * d->leapstep);
    int stuck_any = 0;

    if (!pooled) {
#pragma omp parallel for schedule(static) reduction(| : stuck_any) reduction(+ : cn[:4]) reduction(max : maxsweeps)
        for (int64_t n = 0; n < d->nchains; ++n) {
            double* x = X + n * D; double* g = G + n * D;
            ko_tune tn = { step[n], accepted[n], proposed[n], totproposed[n], NAN };
            int stuck = 0;
            ko_chain ch;
            if (matrix) ko_chain_begin(&c, ss, n, x, g, &ch);
            for (int64_t s = 0; s < nsteps && !stuck; ++s) {
                const int64_t t = t0 + s;
                if (cnt) tn.proposed += 1;
                int64_t nl = d->nleaps;
                double a_prob = 0.0;
                if (da) {                                       /* iterate/HMC.jl:142-144 */
                    const double q = da_lambda / tn.step;
                    nl = (q == q && q < 65536.0) ? (int64_t)nearbyint(q) : 65536;   /* Int(round(.)), ties to even; capped */
                    if (nl < 1) nl = 1;
                }
                double xold[KO_MAXD];
                const int want_fold = sum && held[n] > 0;
                if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
                const int acc = ko_transition(&c, (uint64_t)(d->chain_offset + n), (uint64_t)t,
                                              tn.step, nl, x, g, &LT[n], &stuck, &a_prob, &ch);
                if (stuck) break;
                if (want_fold && acc) ko_fold(sum + n * D, sumsq + n * D, xold, D, &held[n]);
                if (da) {                                       /* iterate/HMC.jl:225-249 */
                    const int64_t count = t + 1;                /* job.sstate.count, incremented at :125-127 */
                    if (count <= d->da_nadapt) {                /* tune!(tune, tuner, count, a) DualAveragingMCTuner.jl:95-101 */
                        const double hweight = 1.0 / (double)(count + d->da_t0);
                        /* DEVIATION: a NaN a (a proposal that is not finite; the transition rejected it) counts as 0 here.  The
                         * reference, DualAveragingMCTuner.jl:95-101, would carry it into h_bar and leave the chain with a NaN step for good. */
                        const double a_tune = a_prob == a_prob ? a_prob : 0.0;
                        da_hbar[n] = (1.0 - hweight) * da_hbar[n] + hweight * (d->targetrate - a_tune);
                        tn.step = kd_exp(da_mu - sqrt((double)count) * da_hbar[n] / d->da_gamma);
                        const double eweight = kd_exp(-d->da_kappa * kd_log((double)count));   /* count^(-kappa) */
                        da_epsbar[n] = kd_exp((1.0 - eweight) * kd_log(da_epsbar[n]) + eweight * kd_log(tn.step));
                    } else {
                        tn.step = da_epsbar[n];                 /* :247 */
                    }
                }
                if (acc && cnt && d->sampler != KLARA_SAMPLER_SLICE) tn.accepted += 1;
                if (accept_out) accept_out[s * d->nchains + n] = (uint8_t)acc;
                if (naccept) naccept[n] += (uint64_t)acc;
                if (!da) ko_tuning_block(d, &tn, cnt, 1);
                else if (cnt && (tn.proposed % d->period) == 0 && t + 1 <= d->da_nadapt) {   /* verbose report block :229-243 */
                    tn.totproposed += tn.proposed; tn.accepted = 0; tn.proposed = 0;
                }
                ko_save(d, n, t, x, g, LT[n], sum ? held : NULL, hist, hist_cols, hist_lt, hist_g);
            }
            step[n] = tn.step; accepted[n] = tn.accepted; proposed[n] = tn.proposed;
            totproposed[n] = tn.totproposed;
            stuck_any |= stuck;
            if (matrix) {
                for (int k = 0; k < 4; ++k) cn[k] += ch.cn[k];
                if (ch.maxsweeps > maxsweeps) maxsweeps = ch.maxsweeps;
            }
        }
    } else {
        ko_tune tn = { step[0], accepted[0], proposed[0], totproposed[0], NAN };
        ko_chain* chs = NULL;                                   /* (matrix) every chain's state, for the length of this call */
        if (matrix) {
            chs = (ko_chain*)malloc(sizeof(ko_chain) * (size_t)d->nchains);
            if (!chs) return KLARA_ERR_NOMEM;
            for (int64_t n = 0; n < d->nchains; ++n) ko_chain_begin(&c, ss, n, X + n * D, G + n * D, &chs[n]);
        }
        for (int64_t s = 0; s < nsteps && !stuck_any; ++s) {
            const int64_t t = t0 + s;
            if (cnt) tn.proposed += 1;
            int64_t nacc = 0;
#pragma omp parallel for schedule(static) reduction(+ : nacc) reduction(| : stuck_any)
            for (int64_t n = 0; n < d->nchains; ++n) {
                int stuck = 0;
                double* x = X + n * D; double* g = G + n * D;
                double xold[KO_MAXD];
                const int want_fold = sum && held[n] > 0;
                if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
                const int acc = ko_transition(&c, (uint64_t)(d->chain_offset + n), (uint64_t)t,
                                              tn.step, d->nleaps, x, g, &LT[n], &stuck, NULL, matrix ? &chs[n] : NULL);
                stuck_any |= stuck;
                if (want_fold && acc && !stuck) ko_fold(sum + n * D, sumsq + n * D, xold, D, &held[n]);
                nacc += acc;
                if (accept_out) accept_out[s * d->nchains + n] = (uint8_t)acc;
                if (naccept) naccept[n] += (uint64_t)acc;
                ko_save(d, n, t, x, g, LT[n], sum ? held : NULL, hist, hist_cols, hist_lt, hist_g);
            }
            if (cnt) tn.accepted += nacc;
            ko_tuning_block(d, &tn, cnt, d->nchains);
        }
        step[0] = tn.step; accepted[0] = tn.accepted; proposed[0] = tn.proposed;
        totproposed[0] = tn.totproposed;
        if (matrix) {
            for (int64_t n = 0; n < d->nchains; ++n) {
                for (int k = 0; k < 4; ++k) cn[k] += chs[n].cn[k];
                if (chs[n].maxsweeps > maxsweeps) maxsweeps = chs[n].maxsweeps;
            }
            free(chs);
        }
    }
    if (matrix) ko_counts_out(ss, cn, maxsweeps);
    return stuck_any ? KLARA_ERR_SLICE_STUCK : KLARA_OK;
}

/* thread control for the cpu_baseline leg of bench.py (OpenMP over chains) */
#ifdef _OPENMP
#include <omp.h>
void ko_set_num_threads(int n) { if (n > 0) omp_set_num_threads(n); }
int ko_get_max_threads(void) { return omp_get_max_threads(); }
#else
void ko_set_num_threads(int n) { (void)n; }
int ko_get_max_threads(void) { return 1; }
#endif

/* ------------------------------------------------------------------ small exports for KATs */
void ko_philox_block(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    const kd_u32x4 r = kd_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
void ko_stream_block(uint64_t seed, uint64_t chain, uint64_t t, uint32_t slot, uint32_t out[4])
{
    const kd_u32x4 r = kd_stream_block(seed, chain, t, slot);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
void ko_math(int op, int64_t n, const double* in, const double* in2, double* out)
{
    for (int64_t i = 0; i < n; ++i) {
        double s, c;
        switch (op) {
        case 0: out[i] = kd_log(in[i]); break;
        case 1: out[i] = kd_exp(in[i]); break;
        case 2: kd_sincos2pi(in[i], &s, &c); out[i] = s; break;
        case 3: kd_sincos2pi(in[i], &s, &c); out[i] = c; break;
        case 4: out[i] = sqrt(in[i]); break;
        case 6: out[i] = kd_erf(in[i]); break;
    case 7: out[i] = kd_log_u01(in[i]); break;
        case 9: out[i] = kd_exp_neg(in[i]); break;
        case 10: kd_softplus_logistic(in[i], &s, &c); out[i] = s; break;
        case 11: kd_softplus_logistic(in[i], &s, &c); out[i] = c; break;
    case 8: out[i] = kd_sqrt_radicand(in[i]); break;
        case 12: out[i] = kd_log12(in[i]); break;
        default: out[i] = in[i] / in2[i]; break;
        }
    }
}
double ko_u52(uint32_t hi, uint32_t lo) { return kd_u52(hi, lo); }
double ko_u44(uint32_t wa, uint32_t wb) { return kd_u44(wa, wb); }
/* the slice sampler's draws of coordinate i in transition t: out[0] = log-uniform's uniform, out[1] = runiform, out[2 ..] = the uniforms of shrink attempts 1 .. nattempts */
void ko_slice_draws(uint64_t seed, uint64_t chain, uint64_t t, uint32_t i, int32_t nattempts, double* out)
{
    const uint32_t base = i << KO_SLICE_ATT_BITS;
    const kd_u32x4 b0 = kd_stream_block(seed, chain, t, base);
    out[0] = kd_uniform_xy(b0); out[1] = kd_uniform_zw(b0);
    for (int32_t a = 1; a <= nattempts; ++a) out[1 + a] = kd_slice_attempt_uniform(seed, chain, t, base, (uint32_t)a);
}
/* the samplers' form: n word pairs (wa, wb) -> 2n normals */
void ko_normal_pairs_w(int64_t n, const uint32_t* w, double* out)
{
    for (int64_t i = 0; i < n; ++i) {
        double u1, lg;
        kd_normal_pair_w(w[2 * i], w[2 * i + 1], &out[2 * i], &out[2 * i + 1], &u1, &lg);
    }
}
/* proposal normals of one transition of one chain as the samplers draw them (D values) and its accept uniform */
void ko_transition_normals(uint64_t seed, uint64_t chain, uint64_t t, int32_t D, double* z, double* accept_u)
{
    ko_normals(seed, chain, t, D, z);
    *accept_u = ko_accept_uniform(seed, chain, t, D);
}
/* the CPU mirror of klara_selftest_normal_tail (same blocks, same counts) */
void ko_normal_tail(uint64_t seed, uint64_t first_chain, int64_t nchains, int64_t ntransitions, int32_t nthr, const double* thr,
                    uint64_t* counts, double* moments)
{
    uint64_t c[8] = { 0 };
    double s1 = 0.0, s2 = 0.0, s4 = 0.0, mx = 0.0;
#pragma omp parallel for schedule(static) reduction(+ : c[:8], s1, s2, s4) reduction(max : mx)
    for (int64_t i = 0; i < nchains; ++i)
        for (int64_t t = 0; t < ntransitions; ++t) {
            double z[4], u1, lg;
            const kd_u32x4 b = kd_stream_block(seed, first_chain + (uint64_t)i, (uint64_t)t, 0u);
            kd_normal_pair_w(b.x, b.y, &z[0], &z[1], &u1, &lg);
            kd_normal_pair_w(b.z, b.w, &z[2], &z[3], &u1, &lg);
            for (int h = 0; h < 4; ++h) {
                const double a = fabs(z[h]);
                for (int k = 0; k < nthr && k < 8; ++k) c[k] += a > thr[k];
                s1 += z[h]; s2 += z[h] * z[h]; s4 += (z[h] * z[h]) * (z[h] * z[h]);
                if (a > mx) mx = a;
            }
        }
    for (int k = 0; k < nthr && k < 8; ++k) counts[k] = c[k];
    if (moments) { moments[0] = s1; moments[1] = s2; moments[2] = s4; moments[3] = mx; }
}

/* target closures for KATs: evaluates lt and gradient of one point */
int ko_eval_target(const klara_desc* d, const ko_layout* L, const double* x, double* lt, double* g)
{
    ko_target_ctx c; ko_ctx_init(&c, d, L);
    double scratch[KO_MAXD];
    if (d->ndims > KO_MAXD) return KLARA_ERR_UNSUPPORTED;
    *lt = ko_uptograd(&c, x, g, scratch);
    return KLARA_OK;
}

/* ---- pieces of SMMALA, RAM and AM for the host tests (ko_smmala_metric, ko_ram_coef, ko_ram_update_c, ko_am_selector, ko_am_covariance
 * and ko_am_factor above are exported as they stand) */
/* one RAM transition of one chain (x, lt, its packed factor S), which also returns what it drew and formed: z (E) and c */
int ko_ram_step(const klara_desc* d, const ko_layout* L, uint64_t chain, uint64_t t, double* x, double* lt, double* S, double* z, double* c_out)
{
    ko_target_ctx c; ko_ctx_init(&c, d, L);
    if (L->E > KO_MAXE || d->ndims > L->E || d->ndims < 1) return -1;
    ko_chain ch = { .S = S };
    return ko_ram(&c, chain, t, x, lt, &ch, z, c_out);
}
/* C = L^-T of a D x D row-major SPD matrix G (tests: C C' = inv(G)); returns 0 when G does not factor */
int ko_smmala_inv_chol_t(const double* G, int D, double* Cout)
{
    const int E = D;
    double gm[KO_MAXNT];
    ko_smmala_state s;
    if (D > KO_MAXE) return 0;
    for (int a = 0; a < D; ++a) for (int b = a; b < D; ++b) gm[ko_tri(a, b, E)] = G[a * D + b];
    /* ko_smmala_factor adds inv_lambda on the diagonal: 0 here */
    const int pd = ko_smmala_factor(gm, D, E, 0.0, &s);
    for (int j = 0; j < D; ++j) {
        double e[KO_MAXE], col[KO_MAXE];
        for (int i = 0; i < D; ++i) e[i] = i == j ? 1.0 : 0.0;
        ko_smmala_solve_lt(&s, E, e, col);
        for (int i = 0; i < D; ++i) Cout[i * D + j] = col[i];
    }
    return pd;
}
/* klara_softabs.h's pieces */
double ko_softabs_f(double lam, double a) { return ksa_f(lam, a); }
/* softabs of a D x D row-major symmetric matrix H (upper triangle read), padded to E as the kernels hold it; T out (D x D, mirrored); returns the sweeps (-1: not transformed) */
int ko_softabs(const double* H, int D, int E, double a, double* T)
{
    double gm[KO_MAXNT];
    if (D > E || E > KO_MAXE) return -2;
    for (int i = 0; i < E; ++i) for (int j = i; j < E; ++j) gm[ko_tri(i, j, E)] = (j < D) ? H[i * D + j] : 0.0;
    double Q[KO_MAXE * KO_MAXE];
    const int sw = ksa_softabs_tri(gm, D, E, a, Q, 1);
    for (int i = 0; i < D; ++i) for (int j = i; j < D; ++j) { T[i * D + j] = gm[ko_tri(i, j, E)]; T[j * D + i] = gm[ko_tri(i, j, E)]; }
    return sw;
}
void ko_softabs_limits(double* out) { out[0] = (double)KSA_MAX_SWEEPS; out[1] = KSA_TOL2; out[2] = KSA_SMALL; out[3] = KSA_BIG; }
