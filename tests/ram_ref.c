/* ram_ref.c — CPU reference of the RAM transition kernels (klara_kernels.h step_ram / ram_update) — TEST INFRASTRUCTURE ONLY.
 *
 * The oracle (oracle/klara_oracle.c) does not know the RAM sampler.  This file adds it on top of the oracle's exported pieces, bound at
 * run time (rr_bind): ko_transition_normals for the draws (the same D normals and accept uniform as MH) and ko_eval_target, handed the
 * job's descriptor relabelled as MH and the job's ko_layout, for the log-target in the kernel's row deal (a user-defined target: the
 * host build of its source, bound by the oracle).  The proposal, the rank-one update and the factorisation follow the kernel loop for
 * loop over the E padded elements.  The driver restates the oracle's ko_run for this sampler: the counting
 * of a verbose VanillaMCTuner, the save rule, running sums in sojourn form, the value / log-target histories.  Compiled by
 * tests/ram_ref.py with gcc -ffp-contract=off against detmath.h. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "detmath.h"
#include "klara_hip.h"

#define RR_MAXE 8
#define RR_MAXNT (RR_MAXE * (RR_MAXE + 1) / 2)

typedef struct rr_layout { int32_t kind, G, E; } rr_layout;      /* = the oracle's ko_layout */
typedef void (*rr_normals_fn)(uint64_t seed, uint64_t chain, uint64_t t, int32_t D, double* z, double* accept_u);
typedef int (*rr_eval_fn)(const klara_desc* d, const rr_layout* L, const double* x, double* lt, double* g);

static rr_normals_fn rr_normals;
static rr_eval_fn rr_eval;

void rr_bind(void* normals, void* eval) { rr_normals = (rr_normals_fn)normals; rr_eval = (rr_eval_fn)eval; }

static int ktri(int a, int b, int E) { return a * E - (a * (a - 1)) / 2 + (b - a); }
static int rr_isfinite(double v) { return v == v && v - v == 0.0; }

/* iterate/RAM.jl:123-127: c = eta (min(1, exp(ratio)) - targetrate) / (z . z), eta = min(1, D count^-gamma), count = t + 1 (R3) */
double rr_coef(int D, uint64_t t, double gamma, double targetrate, double ratio, double zz)
{
    double eta = (double)D * kd_exp(-gamma * kd_log((double)(t + 1ull)));
    eta = eta < 1.0 ? eta : 1.0;
    const double ap = ratio >= 0.0 ? 1.0 : (rr_isfinite(ratio) ? kd_exp(ratio) : 0.0);
    return eta * (ap - targetrate) / zz;
}

/* ram_update from c on: A = S S' + c w w' (R2), factored in place by smmala_factor's loop nest (R4).  S: the packed E x E lower factor,
 * S_ij (i >= j) at ktri(j, i, E).  Returns 1 and the new factor, or 0 — S as it was — where z . z or a pivot is not a finite positive number. */
int rr_update_c(int E, double c, double zz, const double* w, double* S)
{
    const int NT = E * (E + 1) / 2;
    int ok = zz > 0.0 && rr_isfinite(zz);
    double A[RR_MAXNT];
    for (int j = 0; j < E; ++j)
        for (int i = j; i < E; ++i) {
            double a = S[ktri(0, i, E)] * S[ktri(0, j, E)];
            for (int k = 1; k <= j; ++k) a = a + S[ktri(k, i, E)] * S[ktri(k, j, E)];
            A[ktri(j, i, E)] = a + (c * w[i]) * w[j];
        }
    for (int j = 0; j < E; ++j) {
        double sj = A[ktri(j, j, E)];
        for (int k = 0; k < j; ++k) sj = sj - A[ktri(k, j, E)] * A[ktri(k, j, E)];
        const int okj = sj > 0.0 && rr_isfinite(sj);
        ok = ok && okj;
        const double ljj = sqrt(okj ? sj : 1.0);
        const double rj = 1.0 / ljj;
        A[ktri(j, j, E)] = ljj;
        for (int i = j + 1; i < E; ++i) {
            double a = A[ktri(j, i, E)];
            for (int k = 0; k < j; ++k) a = a - A[ktri(k, i, E)] * A[ktri(k, j, E)];
            A[ktri(j, i, E)] = a * rj;
        }
    }
    if (ok) memcpy(S, A, sizeof(double) * (size_t)NT);
    return ok;
}

/* what the last rr_step drew and formed, for the algebra checks of tests/test_ram_host.py: z (E), c */
static double rr_last_z[RR_MAXE], rr_last_c;
void rr_last(double* z, double* c) { memcpy(z, rr_last_z, sizeof(rr_last_z)); *c = rr_last_c; }

/* step_ram for one chain: x (D) and lt are updated on acceptance, the factor S (packed, E padded) after every transition */
int rr_step(const klara_desc* d, const rr_layout* L, uint64_t chain, uint64_t t, double* x, double* lt, double* S, int64_t* skipped)
{
    const int E = L->E, D = d->ndims;
    double z[RR_MAXE], u, w[RR_MAXE], xp[RR_MAXE], gp[RR_MAXE], zz = 0.0, ltp;
    for (int e = 0; e < RR_MAXE; ++e) { z[e] = 0.0; gp[e] = 0.0; }
    rr_normals(d->seed, chain, t, D, z, &u);
    for (int e = 0; e < E; ++e) zz = zz + z[e] * z[e];
    for (int i = 0; i < E; ++i) {                                   /* R1 */
        double a = S[ktri(0, i, E)] * z[0];
        for (int k = 1; k <= i; ++k) a = a + S[ktri(k, i, E)] * z[k];
        w[i] = a;
    }
    for (int e = 0; e < E; ++e) xp[e] = (e < D ? x[e] : 0.0) + w[e];
    rr_eval(d, L, xp, &ltp, gp);
    const double ratio = ltp - *lt;
    int acc = ratio > 0.0;
    if (!acc) acc = ratio > kd_log_u01(u);
    if (acc) { memcpy(x, xp, sizeof(double) * (size_t)D); *lt = ltp; }
    const double c = rr_coef(D, t, d->ram_gamma, d->ram_targetrate, ratio, zz);
    memcpy(rr_last_z, z, sizeof(z)); rr_last_c = c;
    if (!rr_update_c(E, c, zz, w, S)) *skipped += 1;
    return acc;
}

static void rr_save(const klara_desc* d, int64_t n, int64_t t, const double* x, double lt, int64_t* held,
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

/* ko_run's contract for the RAM sampler (d: the job's descriptor relabelled as MH, with the job's ram_targetrate / ram_gamma; S: nchains packed
 * E x E factors; the tuner is a VanillaMCTuner that counts when verbose, iterate/RAM.jl:68-69, 96-121) */
int rr_run(const klara_desc* d, const rr_layout* L, double* X, double* LT, double* S, int64_t* skipped,
           int64_t* accepted, int64_t* proposed, int64_t* totproposed,
           int64_t t0, int64_t nsteps, uint8_t* accept_out, double* sum, double* sumsq,
           uint64_t* naccept, double* hist, int64_t hist_cols, double* hist_lt, int64_t* held)
{
    const int D = d->ndims, E = L->E, NT = E * (E + 1) / 2;
    if (E > RR_MAXE || D > E) return KLARA_ERR_UNSUPPORTED;
    const int cnt = d->verbose != 0;
    for (int64_t n = 0; n < d->nchains; ++n) {
        double* x = X + n * D;
        for (int64_t k = 0; k < nsteps; ++k) {
            const int64_t t = t0 + k;
            if (cnt) proposed[n] += 1;
            double xold[RR_MAXE];
            const int want_fold = sum && held[n] > 0;
            if (want_fold) memcpy(xold, x, sizeof(double) * (size_t)D);
            const int acc = rr_step(d, L, (uint64_t)(d->chain_offset + n), (uint64_t)t, x, &LT[n], S + n * NT, skipped);
            if (want_fold && acc) {
                const double hf = (double)held[n];
                for (int i = 0; i < D; ++i) { sum[n * D + i] = sum[n * D + i] + hf * xold[i]; sumsq[n * D + i] = sumsq[n * D + i] + hf * (xold[i] * xold[i]); }
                held[n] = 0;
            }
            if (acc && cnt) accepted[n] += 1;
            if (accept_out) accept_out[k * d->nchains + n] = (uint8_t)acc;
            if (naccept) naccept[n] += (uint64_t)acc;
            if (cnt && totproposed[n] <= d->burnin && (proposed[n] % d->period) == 0) {      /* :107-121: rate!, reset_burnin! */
                totproposed[n] += proposed[n]; accepted[n] = 0; proposed[n] = 0;
            }
            rr_save(d, n, t, x, LT[n], held, hist, hist_cols, hist_lt, sum != NULL);
        }
    }
    return KLARA_OK;
}
