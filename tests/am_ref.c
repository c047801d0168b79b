/* am_ref.c — CPU reference of the AM transition kernels (klara_kernels.h step_am / am_covariance / am_factor) — TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/klara_oracle.c) does not know the AM sampler.  This file adds it on top of the oracle's exported pieces, bound at
 * run time (ar_bind): ko_transition_normals for the draws (the same D normals and accept uniform as MH) and ko_eval_target, handed the
 * job's descriptor relabelled as MH and the job's ko_layout, for the log-target in the kernel's row deal (a user-defined target: the
 * host build of its source, bound by the oracle).  The selector uniform is words (z, w) of the accept block, from detmath.h.  The
 * covariance update, the factorisation and the proposal are the kernel's operations as plain loops over the D elements — the kernel's
 * padding to E elements may change no bit.  The driver restates the oracle's ko_run for this sampler: the
 * counting of a verbose VanillaMCTuner, the save rule, running sums in sojourn form, the value / log-target histories.  Compiled by
 * tests/am_ref.py with gcc -ffp-contract=off against detmath.h; with AM_REF_MAIN it is a stand-alone program (its own target, draws from
 * detmath.h) for a run under the host sanitizers. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "detmath.h"
#include "klara_hip.h"

#define AR_MAXD 8
#define AR_MAXNT (AR_MAXD * (AR_MAXD + 1) / 2)

typedef struct ar_layout { int32_t kind, G, E; } ar_layout;      /* = the oracle's ko_layout */
typedef void (*ar_normals_fn)(uint64_t seed, uint64_t chain, uint64_t t, int32_t D, double* z, double* accept_u);
typedef int (*ar_eval_fn)(const klara_desc* d, const ar_layout* L, const double* x, double* lt, double* g);

static ar_normals_fn ar_normals;
static ar_eval_fn ar_eval;

void ar_bind(void* normals, void* eval) { ar_normals = (ar_normals_fn)normals; ar_eval = (ar_eval_fn)eval; }

static int ktri(int a, int b, int D) { return a * D - (a * (a - 1)) / 2 + (b - a); }
static int ar_isfinite(double v) { return v == v && v - v == 0.0; }

/* the component selector of transition t: words (z, w) of the accept block, slot ceil(D / 2) */
double ar_selector(uint64_t seed, uint64_t chain, uint64_t t, int D)
{
    return kd_uniform_zw(kd_stream_block(seed, chain, t, (uint32_t)((D + 1) >> 1)));
}

/* covariance!(C, C, k, x, lastmean, secondlastmean), stats/covariance.jl:6-19, on the packed upper triangle (C_ij, i <= j, at ktri(i, j, D)) */
void ar_covariance(int D, int64_t k, const double* x, const double* m, const double* m2, double* C)
{
    const double kf = (double)k, km1 = (double)(k - 1), nk1 = (double)(-(k + 1));
    for (int i = 0; i < D; ++i) {
        const double a = nk1 * m[i], b = kf * m2[i];
        for (int j = i; j < D; ++j) {
            double c = km1 * C[ktri(i, j, D)];
            c = c + x[i] * x[j];
            c = c + a * m[j];
            c = c + b * m2[j];
            C[ktri(i, j, D)] = c / kf;
        }
    }
}

/* L = chol(corescale C), lower, L_ji (j >= i) at ktri(i, j, D); 1, or 0 where a pivot is not a finite positive number (A2) */
int ar_factor(int D, double corescale, const double* C, double* A)
{
    int ok = 1;
    for (int k = 0; k < D * (D + 1) / 2; ++k) A[k] = corescale * C[k];
    for (int j = 0; j < D; ++j) {
        double sj = A[ktri(j, j, D)];
        for (int k = 0; k < j; ++k) sj = sj - A[ktri(k, j, D)] * A[ktri(k, j, D)];
        const int okj = sj > 0.0 && ar_isfinite(sj);
        ok = ok && okj;
        const double ljj = sqrt(okj ? sj : 1.0);
        const double rj = 1.0 / ljj;
        A[ktri(j, j, D)] = ljj;
        for (int i = j + 1; i < D; ++i) {
            double a = A[ktri(j, i, D)];
            for (int k = 0; k < j; ++k) a = a - A[ktri(k, i, D)] * A[ktri(k, j, D)];
            A[ktri(j, i, D)] = a * rj;
        }
    }
    return ok;
}

/* step_am for one chain: x (D) and lt are updated on acceptance; C (packed), m, m2 as the kernel keeps them */
int ar_step(const klara_desc* d, const ar_layout* L, uint64_t chain, uint64_t t, double* x, double* lt, double* C, double* m, double* m2,
            int64_t* fallbacks)
{
    const int D = d->ndims;
    const int64_t count = (int64_t)t + 1;
    const double sqrtminor = sqrt(d->am_minorscale), w1 = 1.0 - d->am_c;
    double z[AR_MAXD], u, xp[AR_MAXD], gp[AR_MAXD], ltp;
    for (int e = 0; e < AR_MAXD; ++e) { z[e] = 0.0; gp[e] = 0.0; xp[e] = 0.0; }
    ar_normals(d->seed, chain, t, D, z, &u);
    if (count > d->am_t0) {
        double Lf[AR_MAXNT];
        ar_covariance(D, count - 2, x, m, m2, C);
        const int ok = ar_factor(D, d->am_corescale, C, Lf);
        if (!ok) *fallbacks += 1;
        const int core = ok && ar_selector(d->seed, chain, t, D) < w1;
        for (int i = 0; i < D; ++i) {
            double a = Lf[ktri(0, i, D)] * z[0];
            for (int k = 1; k <= i; ++k) a = a + Lf[ktri(k, i, D)] * z[k];
            xp[i] = x[i] + (core ? a : sqrtminor * z[i]);
        }
    } else {
        for (int e = 0; e < D; ++e) xp[e] = x[e] + sqrtminor * z[e];
    }
    ar_eval(d, L, xp, &ltp, gp);
    const double ratio = ltp - *lt;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(u);
    if (acc) { memcpy(x, xp, sizeof(double) * (size_t)D); *lt = ltp; }
    const double cm1 = (double)(count - 1), cf = (double)count;
    for (int e = 0; e < D; ++e) { m2[e] = m[e]; m[e] = (cm1 * m[e] + x[e]) / cf; }
    return acc;
}

static void ar_save(const klara_desc* d, int64_t n, int64_t t, const double* x, double lt, int64_t* held,
                    double* hist, int64_t hist_cols, double* hist_lt, int sums)
{
    const int D = d->ndims;
    const int64_t i1 = t + 1;
    if (i1 > d->burnin && (i1 - d->burnin - 1) % d->thinning == 0 && i1 <= d->nsteps) {
        const int64_t col = (i1 - d->burnin - 1) / d->thinning;
        if (sums) held[n] += 1;
        if (hist && col < hist_cols) memcpy(hist + ((size_t)col * (size_t)d->nchains + (size_t)n) * (size_t)D, x, sizeof(double) * (size_t)D);
        if (hist_lt && col < hist_cols) hist_lt[(size_t)col * (size_t)d->nchains + (size_t)n] = lt;
    }
}

/* ko_run's contract for the AM sampler (d: the job's descriptor relabelled as MH, with the job's am_corescale / am_minorscale / am_c / am_t0; C: nchains
 * packed D x D upper triangles; M, M2: nchains x D running means; the tuner is a VanillaMCTuner that counts when verbose, iterate/AM.jl:80-82, 123-125,
 * 137-151) */
int ar_run(const klara_desc* d, const ar_layout* L, double* X, double* LT, double* C, double* M, double* M2, int64_t* fallbacks,
           int64_t* accepted, int64_t* proposed, int64_t* totproposed,
           int64_t t0, int64_t nsteps, uint8_t* accept_out, double* sum, double* sumsq,
           uint64_t* naccept, double* hist, int64_t hist_cols, double* hist_lt, int64_t* held)
{
    const int D = d->ndims, NT = D * (D + 1) / 2;
    if (D > AR_MAXD || D < 1) return KLARA_ERR_UNSUPPORTED;
    const int cnt = d->verbose != 0;
    for (int64_t n = 0; n < d->nchains; ++n) {
        double* x = X + n * D;
        for (int64_t k = 0; k < nsteps; ++k) {
            const int64_t t = t0 + k;
            if (cnt) proposed[n] += 1;
            double xold[AR_MAXD];
            const int want_fold = sum && held[n] > 0;
            if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
            const int acc = ar_step(d, L, (uint64_t)(d->chain_offset + n), (uint64_t)t, x, &LT[n], C + n * NT, M + n * D, M2 + n * D, fallbacks);
            if (want_fold && acc) {
                const double hf = (double)held[n];
                for (int i = 0; i < D; ++i) { sum[n * D + i] = sum[n * D + i] + hf * xold[i]; sumsq[n * D + i] = sumsq[n * D + i] + hf * (xold[i] * xold[i]); }
                held[n] = 0;
            }
            if (acc && cnt) accepted[n] += 1;
            if (accept_out) accept_out[k * d->nchains + n] = (uint8_t)acc;
            if (naccept) naccept[n] += (uint64_t)acc;
            if (cnt && totproposed[n] <= d->burnin && (proposed[n] % d->period) == 0) {      /* :137-151: rate!, reset_burnin! */
                totproposed[n] += proposed[n]; accepted[n] = 0; proposed[n] = 0;
            }
            ar_save(d, n, t, x, LT[n], held, hist, hist_cols, hist_lt, sum != NULL);
        }
    }
    return KLARA_OK;
}

#ifdef AM_REF_MAIN
/* Stand-alone run for the host sanitizers: 5 chains of a D = 3 job with t0 = 2 (so that the fallback path runs) on a Gaussian target of its own,
 * drawing through detmath.h as the oracle does (kd_normal_pair_at, kd_accept_uniform).  Prints a checksum; exit status 0 when the state is finite. */
#include <stdio.h>
static void main_normals(uint64_t seed, uint64_t chain, uint64_t t, int32_t D, double* z, double* accept_u)
{
    const uint32_t np = (uint32_t)((D + 1) / 2);
    for (uint32_t p = 0; p < np; ++p) {
        double z0, z1, u1, lg;
        kd_normal_pair_at(seed, chain, t, p, np, &z0, &z1, &u1, &lg);
        z[2 * p] = z0;
        if ((int32_t)(2 * p + 1) < D) z[2 * p + 1] = z1;
    }
    *accept_u = kd_accept_uniform(kd_stream_block(seed, chain, t, np));
}
static int main_eval(const klara_desc* d, const ar_layout* L, const double* x, double* lt, double* g)
{
    (void)L; (void)g;
    double s = 0.0;
    for (int i = 0; i < d->ndims; ++i) s = s + (double)(i + 1) * x[i] * x[i];
    *lt = -0.5 * s;
    return 0;
}
int main(void)
{
    enum { N = 5, D = 3, STEPS = 60 };
    klara_desc d;
    memset(&d, 0, sizeof d);
    d.ndims = D; d.nchains = N; d.nsteps = STEPS; d.thinning = 1; d.period = 7; d.verbose = 1; d.seed = 20260927u;
    d.am_corescale = 1.9; d.am_minorscale = 0.25; d.am_c = 0.1; d.am_t0 = 2;
    ar_layout L = { 0, 1, 4 };
    ar_bind((void*)main_normals, (void*)main_eval);
    double* X = malloc(sizeof(double) * N * D); double* LT = malloc(sizeof(double) * N);
    double* C = malloc(sizeof(double) * N * D * (D + 1) / 2); double* M = malloc(sizeof(double) * N * D); double* M2 = malloc(sizeof(double) * N * D);
    int64_t* acc = calloc(N, sizeof(int64_t)); int64_t* prop = calloc(N, sizeof(int64_t)); int64_t* tot = calloc(N, sizeof(int64_t));
    int64_t* held = calloc(N, sizeof(int64_t)); uint64_t* nacc = calloc(N, sizeof(uint64_t));
    uint8_t* mask = malloc((size_t)STEPS * N);
    double* sum = calloc(N * D, sizeof(double)); double* sumsq = calloc(N * D, sizeof(double));
    double* hist = malloc(sizeof(double) * STEPS * N * D); double* hist_lt = malloc(sizeof(double) * STEPS * N);
    int64_t fallbacks = 0;
    for (int n = 0; n < N; ++n) {
        for (int i = 0; i < D; ++i) { X[n * D + i] = 0.1 * (n + 1) - 0.2 * i; M[n * D + i] = M2[n * D + i] = X[n * D + i]; }
        for (int i = 0; i < D; ++i) for (int j = i; j < D; ++j) C[n * (D * (D + 1) / 2) + ktri(i, j, D)] = i == j ? 1.0 : 0.0;
        main_eval(&d, &L, X + n * D, &LT[n], NULL);
        tot[n] = d.period;
    }
    int st = ar_run(&d, &L, X, LT, C, M, M2, &fallbacks, acc, prop, tot, 0, 25, mask, sum, sumsq, nacc, hist, STEPS, hist_lt, held);
    if (st == 0) st = ar_run(&d, &L, X, LT, C, M, M2, &fallbacks, acc, prop, tot, 25, STEPS - 25, mask + 25 * N, sum, sumsq, nacc, hist, STEPS, hist_lt, held);
    double cs = 0.0; int finite = 1; uint64_t na = 0;
    for (int k = 0; k < N * D; ++k) { cs += X[k] + M[k] + M2[k]; finite = finite && ar_isfinite(X[k]) && ar_isfinite(M[k]); }
    for (int k = 0; k < N * D * (D + 1) / 2; ++k) { cs += C[k]; finite = finite && ar_isfinite(C[k]); }
    for (int n = 0; n < N; ++n) na += nacc[n];
    printf("am_ref main: status %d, checksum %.17g, accepted %llu of %d, fallbacks %lld, finite %d\n", st, cs, (unsigned long long)na, N * STEPS,
           (long long)fallbacks, finite);
    free(X); free(LT); free(C); free(M); free(M2); free(acc); free(prop); free(tot); free(held); free(nacc); free(mask); free(sum); free(sumsq);
    free(hist); free(hist_lt);
    return st == 0 && finite && fallbacks > 0 ? 0 : 1;
}
#endif
