/* softabs_ref.c — CPU reference of the SMMALA transition kernels with the softabs transform of the metric (klara_softabs.h) — TEST INFRASTRUCTURE ONLY.
 *
 * tests/smmala_ref.c has no hook between the metric and its factorisation, so this file restates its transition loop for user-defined targets
 * (the only ones the transform runs on) in the same operation order as the kernel (klara_kernels.h step_smmala, SMMALA deviations S1-S5):
 * every metric — at a launch start, at a start state, at a proposal — goes through ksa_softabs_tri(gm, D, E, desc.smmala_softabs), the very
 * header the device compiles, between CustomTarget::eval's triangle and the factorisation.  Bound to the oracle's exported pieces like
 * smmala_ref.c (same entry-point names, so tests/smmala_ref.py's job class drives either library).  sa_f / sa_softabs / sa_limits expose the
 * header's pieces to tests/test_softabs_host.py.  Compiled by tests/softabs_ref.py with gcc -ffp-contract=off against detmath.h. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "detmath.h"
#include "klara_hip.h"
#include "klara_softabs.h"

#define SR_MAXE 8
#define SR_MAXNT (SR_MAXE * (SR_MAXE + 1) / 2)

typedef struct sr_layout { int32_t kind, G, E; } sr_layout;      /* = the oracle's ko_layout */
typedef void (*sr_normals_fn)(uint64_t seed, uint64_t chain, uint64_t t, int32_t D, double* z, double* accept_u);
typedef int (*sr_eval_fn)(const klara_desc* d, const sr_layout* L, const double* x, double* lt, double* g);
typedef double (*sr_score_fn)(double x, double k);

static sr_normals_fn sr_normals;
static sr_eval_fn sr_eval;
static sr_score_fn sr_logistic_score, sr_erf_score;
/* a user-defined target's klara_user_tensorlogtarget (the host build of the job's source, tests/oracle_ffi.py compile_user_target) */
typedef void (*sr_tensor_fn)(const double* x, int D, const double* data, long long ndata, double* G);
static sr_tensor_fn sr_tensor;
void sr_bind_tensor(void* tensor) { sr_tensor = (sr_tensor_fn)tensor; }

void sr_bind(void* normals, void* eval, void* logistic_score, void* erf_score)
{
    sr_normals = (sr_normals_fn)normals; sr_eval = (sr_eval_fn)eval;
    sr_logistic_score = (sr_score_fn)logistic_score; sr_erf_score = (sr_score_fn)erf_score;
}

static int ktri(int a, int b, int E) { return a * E - (a * (a - 1)) / 2 + (b - a); }
static int sr_isfinite(double v) { return v == v && v - v == 0.0; }

typedef struct sr_state { double L[SR_MAXNT], r[SR_MAXE], f[SR_MAXE], ld; } sr_state;

/* the upper triangle of a user's tensor (CustomTarget::eval, NTRI > 0) */
void sr_metric(const klara_desc* d, const sr_layout* L, const double* x, double* gm)
{
    const int E = L->E, D = d->ndims, NT = E * (E + 1) / 2, n = d->logit_ndata;
    if (d->target == KLARA_TARGET_CUSTOM) {
        double gt[SR_MAXE * SR_MAXE];
        sr_tensor(x, D, d->custom_data, (long long)d->custom_ndata, gt);
        for (int a = 0; a < E; ++a) for (int b = a; b < E; ++b) gm[ktri(a, b, E)] = b < D ? gt[a * D + b] : 0.0;
        return;
    }
    (void)NT; (void)n;
    for (int k = 0; k < NT; ++k) gm[k] = kd_u2d(0x7ff8000000000000ull);          /* (no other target runs the transform) */
}

/* the metric's diagonal term beyond gm (T::metric_diag): I / lambda of the logistic target, nothing for a user's tensor */
static double sr_diag(const klara_desc* d) { return d->target == KLARA_TARGET_LOGISTIC ? 1.0 / d->logit_lambda : 0.0; }

/* the metric with T::metric_diag added, transformed (klara_kernels.h smmala_softabs_metric); the factorisation then adds nothing */
static int sr_last_sweeps, sr_max_sweeps;
static long long sr_sum_sweeps, sr_nfactor;
static void sr_transform(const klara_desc* d, int E, double* gm)
{
    const int D = d->ndims;
    const double diag = sr_diag(d);
    for (int j = 0; j < D; ++j) gm[ktri(j, j, E)] = gm[ktri(j, j, E)] + diag;
    double Q[SR_MAXE * SR_MAXE];
    sr_last_sweeps = ksa_softabs_tri(gm, D, E, d->smmala_softabs, Q, 1);
    if (sr_last_sweeps > sr_max_sweeps) sr_max_sweeps = sr_last_sweeps;
    if (sr_last_sweeps >= 0) { sr_sum_sweeps += sr_last_sweeps; sr_nfactor += 1; }
}
/* sweeps per transformed metric since the last call: out[0] = how many, out[1] = their sum, out[2] = the maximum; the counters start again */
void sa_sweep_stats(long long* out) { out[0] = sr_nfactor; out[1] = sr_sum_sweeps; out[2] = sr_max_sweeps; sr_nfactor = 0; sr_sum_sweeps = 0; sr_max_sweeps = 0; }

/* smmala_factor: G = L L' column by column; 1 when every pivot is a finite positive number */
static int sr_factor(const double* gm, int D, int E, double inv_lambda, sr_state* s)
{
    int pd = 1;
    double ld = 0.0;
    for (int j = 0; j < E; ++j) {
        double sj = j < D ? gm[ktri(j, j, E)] + inv_lambda : 1.0;
        for (int k = 0; k < j; ++k) sj = sj - s->L[ktri(k, j, E)] * s->L[ktri(k, j, E)];
        const int ok = sj > 0.0 && sr_isfinite(sj);
        pd = pd && ok;
        const double ljj = sqrt(ok ? sj : 1.0);
        const double rj = 1.0 / ljj;
        s->L[ktri(j, j, E)] = ljj; s->r[j] = rj;
        ld = ld + kd_log(ljj);
        for (int i = j + 1; i < E; ++i) {
            double t = (i < D && j < D) ? gm[ktri(j, i, E)] : 0.0;
            for (int k = 0; k < j; ++k) t = t - s->L[ktri(k, i, E)] * s->L[ktri(k, j, E)];
            s->L[ktri(j, i, E)] = t * rj;
        }
    }
    s->ld = ld;
    return pd;
}
static void sr_solve_lt(const sr_state* s, int E, const double* z, double* v)
{
    for (int i = E - 1; i >= 0; --i) {
        double t = z[i];
        for (int k = i + 1; k < E; ++k) t = t - s->L[ktri(i, k, E)] * v[k];
        v[i] = t * s->r[i];
    }
}
static void sr_drift(sr_state* s, int E, const double* g)
{
    double y[SR_MAXE];
    for (int i = 0; i < E; ++i) {
        double t = g[i];
        for (int k = 0; k < i; ++k) t = t - s->L[ktri(k, i, E)] * y[k];
        y[i] = t * s->r[i];
    }
    sr_solve_lt(s, E, y, s->f);
}
static double sr_quad(const sr_state* s, int E, const double* d)
{
    double q = 0.0;
    for (int i = 0; i < E; ++i) {
        double w = s->L[ktri(i, i, E)] * d[i];
        for (int k = i + 1; k < E; ++k) w = w + s->L[ktri(i, k, E)] * d[k];
        q = q + w * w;
    }
    return q;
}

/* the factor state at x (padded to E) with gradient g: what the kernels form at a launch start and check at a start state */
static int sr_state_at(const klara_desc* d, const sr_layout* L, const double* x, const double* g, sr_state* s)
{
    const int E = L->E, D = d->ndims;
    double gm[SR_MAXNT], gp[SR_MAXE];
    sr_metric(d, L, x, gm);
    for (int e = 0; e < E; ++e) gp[e] = e < D ? g[e] : 0.0;
    sr_transform(d, E, gm);
    const int pd = sr_factor(gm, D, E, 0.0, s);
    sr_drift(s, E, gp);
    return pd;
}

/* 1 when the metric at every start state x[n] (gradient g[n]) is positive definite; bad[n] flags the others */
int sr_check_init(const klara_desc* d, const sr_layout* L, const double* X, const double* G, uint8_t* bad)
{
    const int D = d->ndims;
    int all = 1;
    for (int64_t n = 0; n < d->nchains; ++n) {
        sr_state s;
        const int pd = sr_state_at(d, L, X + n * D, G + n * D, &s);
        if (bad) bad[n] = (uint8_t)!pd;
        all = all && pd;
    }
    return all;
}

/* step_smmala for one chain: x, g (D), lt and the factor state s are updated on acceptance */
int sr_step(const klara_desc* d, const sr_layout* L, uint64_t chain, uint64_t t, double h, double* x, double* g, double* lt, sr_state* s)
{
    const int E = L->E, D = d->ndims, NT = E * (E + 1) / 2;
    double z[SR_MAXE], u, xe[SR_MAXE], mu[SR_MAXE], v[SR_MAXE], xp[SR_MAXE], dd[SR_MAXE], gp[SR_MAXE], gm[SR_MAXNT];
    for (int e = 0; e < SR_MAXE; ++e) { z[e] = 0.0; gp[e] = 0.0; }
    sr_normals(d->seed, chain, t, D, z, &u);
    for (int e = 0; e < E; ++e) xe[e] = e < D ? x[e] : 0.0;
    const double halfh = 0.5 * h, sq = sqrt(h), inv_h = 1.0 / h, dlogh = (double)D * kd_log(h);
    for (int e = 0; e < E; ++e) mu[e] = xe[e] + halfh * s->f[e];
    sr_solve_lt(s, E, z, v);
    for (int e = 0; e < E; ++e) xp[e] = mu[e] + sq * v[e];
    for (int e = 0; e < E; ++e) dd[e] = xp[e] - mu[e];
    const double fwd = 0.5 * ((dlogh - 2.0 * s->ld) + sr_quad(s, E, dd) * inv_h);
    double ltp;
    sr_eval(d, L, xp, &ltp, gp);
    sr_metric(d, L, xp, gm);
    sr_state sn;
    sr_transform(d, E, gm);
    const int pd = sr_factor(gm, D, E, 0.0, &sn);
    sr_drift(&sn, E, gp);
    for (int e = 0; e < E; ++e) dd[e] = xe[e] - (xp[e] + halfh * sn.f[e]);
    const double rev = 0.5 * ((dlogh - 2.0 * sn.ld) + sr_quad(&sn, E, dd) * inv_h);
    double ratio = ltp - *lt;
    ratio += fwd;
    ratio -= rev;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(u);
    acc = acc && pd;
    (void)NT;
    if (acc) {
        memcpy(x, xp, sizeof(double) * (size_t)D);
        memcpy(g, gp, sizeof(double) * (size_t)D);
        *lt = ltp;
        *s = sn;
    }
    return acc;
}

static void sr_tuning_block(const klara_desc* d, double* step, int64_t* accepted, int64_t* proposed, int64_t* totproposed, int cnt, int64_t pool)
{
    if (!cnt) return;
    if (*totproposed <= d->burnin && (*proposed % d->period) == 0) {
        const double rate = (double)*accepted / (double)(*proposed * pool);
        if (d->tuner == KLARA_TUNER_ACCEPT_RATE)
            *step *= d->tuner_score == 1 ? sr_erf_score(rate - d->targetrate, d->score_k) : sr_logistic_score(rate - d->targetrate, d->score_k);
        *totproposed += *proposed;
        *accepted = 0; *proposed = 0;
    }
}

static void sr_save(const klara_desc* d, int64_t n, int64_t t, const double* x, const double* g, double lt, int64_t* held,
                    double* hist, int64_t hist_cols, double* hist_lt, double* hist_g, int sums)
{
    const int D = d->ndims;
    const int64_t i1 = t + 1;
    if (i1 > d->burnin && (i1 - d->burnin - 1) % d->thinning == 0 && i1 <= d->nsteps) {
        const int64_t col = (i1 - d->burnin - 1) / d->thinning;
        if (sums) held[n] += 1;
        if (hist && col < hist_cols) memcpy(hist + ((size_t)col * (size_t)d->nchains + (size_t)n) * (size_t)D, x, sizeof(double) * (size_t)D);
        if (hist_lt && col < hist_cols) hist_lt[(size_t)col * (size_t)d->nchains + (size_t)n] = lt;
        if (hist_g && col < hist_cols) memcpy(hist_g + ((size_t)col * (size_t)d->nchains + (size_t)n) * (size_t)D, g, sizeof(double) * (size_t)D);
    }
}
static void sr_fold(double* sum, double* sumsq, const double* xold, int D, int64_t* held)
{
    const double hf = (double)*held;
    for (int i = 0; i < D; ++i) { sum[i] = sum[i] + hf * xold[i]; sumsq[i] = sumsq[i] + hf * (xold[i] * xold[i]); }
    *held = 0;
}

/* ko_run's contract for the SMMALA sampler (d: the job's descriptor relabelled as MALA; the factor state of every chain is formed from
 * its x and gradient at the start of the call, as the kernels do at a launch start) */
int sr_run(const klara_desc* d, const sr_layout* L, double* X, double* G, double* LT,
           double* step, int64_t* accepted, int64_t* proposed, int64_t* totproposed,
           int64_t t0, int64_t nsteps, uint8_t* accept_out, double* sum, double* sumsq,
           uint64_t* naccept, double* hist, int64_t hist_cols, double* hist_lt, double* hist_g, int64_t* held)
{
    const int D = d->ndims;
    if (L->E > SR_MAXE || D > L->E) return KLARA_ERR_UNSUPPORTED;
    const int cnt = (d->tuner == KLARA_TUNER_VANILLA && d->verbose) || d->tuner == KLARA_TUNER_ACCEPT_RATE;
    const int pooled = d->tuner_mode == KLARA_TUNE_POOLED;
    if (!pooled) {
        for (int64_t n = 0; n < d->nchains; ++n) {
            double* x = X + n * D; double* g = G + n * D;
            sr_state s;
            sr_state_at(d, L, x, g, &s);
            for (int64_t k = 0; k < nsteps; ++k) {
                const int64_t t = t0 + k;
                if (cnt) proposed[n] += 1;
                double xold[SR_MAXE];
                const int want_fold = sum && held[n] > 0;
                if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
                const int acc = sr_step(d, L, (uint64_t)(d->chain_offset + n), (uint64_t)t, step[n], x, g, &LT[n], &s);
                if (want_fold && acc) sr_fold(sum + n * D, sumsq + n * D, xold, D, &held[n]);
                if (acc && cnt) accepted[n] += 1;
                if (accept_out) accept_out[k * d->nchains + n] = (uint8_t)acc;
                if (naccept) naccept[n] += (uint64_t)acc;
                sr_tuning_block(d, &step[n], &accepted[n], &proposed[n], &totproposed[n], cnt, 1);
                sr_save(d, n, t, x, g, LT[n], held, hist, hist_cols, hist_lt, hist_g, sum != NULL);
            }
        }
    } else {
        sr_state* st = (sr_state*)malloc(sizeof(sr_state) * (size_t)d->nchains);
        if (!st) return KLARA_ERR_NOMEM;
        for (int64_t n = 0; n < d->nchains; ++n) sr_state_at(d, L, X + n * D, G + n * D, &st[n]);
        for (int64_t k = 0; k < nsteps; ++k) {
            const int64_t t = t0 + k;
            if (cnt) proposed[0] += 1;
            int64_t nacc = 0;
            for (int64_t n = 0; n < d->nchains; ++n) {
                double* x = X + n * D; double* g = G + n * D;
                double xold[SR_MAXE];
                const int want_fold = sum && held[n] > 0;
                if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
                const int acc = sr_step(d, L, (uint64_t)(d->chain_offset + n), (uint64_t)t, step[0], x, g, &LT[n], &st[n]);
                if (want_fold && acc) sr_fold(sum + n * D, sumsq + n * D, xold, D, &held[n]);
                nacc += acc;
                if (accept_out) accept_out[k * d->nchains + n] = (uint8_t)acc;
                if (naccept) naccept[n] += (uint64_t)acc;
                sr_save(d, n, t, x, g, LT[n], held, hist, hist_cols, hist_lt, hist_g, sum != NULL);
            }
            if (cnt) accepted[0] += nacc;
            sr_tuning_block(d, &step[0], &accepted[0], &proposed[0], &totproposed[0], cnt, d->nchains);
        }
        free(st);
    }
    return KLARA_OK;
}

/* ---- the header's pieces, for tests/test_softabs_host.py ---- */
double sa_f(double lam, double a) { return ksa_f(lam, a); }
/* softabs of a D x D row-major symmetric matrix H (upper triangle read), padded to E as the kernels hold it; T out (D x D, mirrored); returns the sweeps (-1: not transformed) */
int sa_softabs(const double* H, int D, int E, double a, double* T)
{
    double gm[SR_MAXNT];
    if (D > E || E > SR_MAXE) return -2;
    for (int i = 0; i < E; ++i) for (int j = i; j < E; ++j) gm[ktri(i, j, E)] = (j < D) ? H[i * D + j] : 0.0;
    double Q[SR_MAXE * SR_MAXE];
    const int sw = ksa_softabs_tri(gm, D, E, a, Q, 1);
    for (int i = 0; i < D; ++i) for (int j = i; j < D; ++j) { T[i * D + j] = gm[ktri(i, j, E)]; T[j * D + i] = gm[ktri(i, j, E)]; }
    return sw;
}
void sa_limits(double* out) { out[0] = (double)KSA_MAX_SWEEPS; out[1] = KSA_TOL2; out[2] = KSA_SMALL; out[3] = KSA_BIG; }
