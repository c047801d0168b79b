/* am_sanitizer_main.c — a stand-alone run of the oracle's AM sampler for the host sanitizers — TEST INFRASTRUCTURE ONLY.
 *
 * Compiled together with oracle/klara_oracle.c by tests/am_ref.py (sanitizer_program: -fsanitize=address,undefined) and run as a program of
 * its own by tests/test_am_host.py: 5 chains of a D = 3 job with t0 = 2 (so that the fallback path runs) on a Gaussian target of its own,
 * registered as a user-defined target, through ko_init and two ko_run calls.  Prints a checksum; exit status 0 when the state is finite. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "klara_hip.h"

typedef struct ko_layout { int32_t kind, G, E; } ko_layout;
typedef struct ko_sampler_state { double* ram_S; int64_t* ram_skipped; double *am_C, *am_mean, *am_mean2; int64_t* am_fallbacks; int64_t* softabs_sweeps; } ko_sampler_state;
typedef double (*lt_fn)(const double* x, int D, const double* data, long long ndata);
typedef void (*grad_fn)(const double* x, int D, const double* data, long long ndata, double* g);
void ko_set_custom_target(lt_fn lt, grad_fn grad);
int ko_init(const klara_desc* d, const ko_layout* L, const double* X, double* G, double* LT, double* step, int64_t* accepted, int64_t* proposed,
            int64_t* totproposed, double* da_epsbar, double* da_hbar, const ko_sampler_state* ss);
int ko_run(const klara_desc* d, const ko_layout* L, double* X, double* G, double* LT, double* step, int64_t* accepted, int64_t* proposed,
           int64_t* totproposed, int64_t t0, int64_t nsteps, uint8_t* accept_out, double* sum, double* sumsq, uint64_t* naccept, double* hist,
           int64_t hist_cols, double* hist_lt, double* hist_g, double* da_epsbar, double* da_hbar, int64_t* held, const ko_sampler_state* ss);

static double main_lt(const double* x, int D, const double* data, long long ndata)
{
    (void)data; (void)ndata;
    double s = 0.0;
    for (int i = 0; i < D; ++i) s = s + (double)(i + 1) * x[i] * x[i];
    return -0.5 * s;
}
static int is_finite(double v) { return v == v && v - v == 0.0; }

int main(void)
{
    enum { N = 5, D = 3, NT = D * (D + 1) / 2, STEPS = 60 };
    klara_desc d;
    memset(&d, 0, sizeof d);
    d.sampler = KLARA_SAMPLER_AM; d.target = KLARA_TARGET_CUSTOM;
    d.ndims = D; d.nchains = N; d.nsteps = STEPS; d.thinning = 1; d.period = 7; d.verbose = 1; d.seed = 20260927u;
    d.am_corescale = 1.9; d.am_minorscale = 0.25; d.am_c = 0.1; d.am_t0 = 2;
    ko_layout L = { 0, 1, 4 };
    ko_set_custom_target(main_lt, NULL);
    double* X = malloc(sizeof(double) * N * D); double* G = calloc(N * D, sizeof(double)); double* LT = malloc(sizeof(double) * N);
    double* C = malloc(sizeof(double) * N * NT); double* M = malloc(sizeof(double) * N * D); double* M2 = malloc(sizeof(double) * N * D);
    double* step = malloc(sizeof(double) * N);
    int64_t* acc = calloc(N, sizeof(int64_t)); int64_t* prop = calloc(N, sizeof(int64_t)); int64_t* tot = calloc(N, sizeof(int64_t));
    int64_t* held = calloc(N, sizeof(int64_t)); uint64_t* nacc = calloc(N, sizeof(uint64_t));
    uint8_t* mask = malloc((size_t)STEPS * N);
    double* sum = calloc(N * D, sizeof(double)); double* sumsq = calloc(N * D, sizeof(double));
    double* hist = malloc(sizeof(double) * STEPS * N * D); double* hist_lt = malloc(sizeof(double) * STEPS * N);
    int64_t fallbacks = 0;
    const ko_sampler_state ss = { .am_C = C, .am_mean = M, .am_mean2 = M2, .am_fallbacks = &fallbacks };
    for (int n = 0; n < N; ++n) {
        for (int i = 0; i < D; ++i) { X[n * D + i] = 0.1 * (n + 1) - 0.2 * i; M[n * D + i] = M2[n * D + i] = X[n * D + i]; }
        for (int i = 0, k = 0; i < D; ++i) for (int j = i; j < D; ++j, ++k) C[n * NT + k] = i == j ? 1.0 : 0.0;
    }
    int st = ko_init(&d, &L, X, G, LT, step, acc, prop, tot, NULL, NULL, &ss);
    if (st == 0) st = ko_run(&d, &L, X, G, LT, step, acc, prop, tot, 0, 25, mask, sum, sumsq, nacc, hist, STEPS, hist_lt, NULL, NULL, NULL, held, &ss);
    if (st == 0) st = ko_run(&d, &L, X, G, LT, step, acc, prop, tot, 25, STEPS - 25, mask + 25 * N, sum, sumsq, nacc, hist, STEPS, hist_lt, NULL, NULL, NULL, held, &ss);
    double cs = 0.0; int finite = 1; uint64_t na = 0;
    for (int k = 0; k < N * D; ++k) { cs += X[k] + M[k] + M2[k]; finite = finite && is_finite(X[k]) && is_finite(M[k]); }
    for (int k = 0; k < N * NT; ++k) { cs += C[k]; finite = finite && is_finite(C[k]); }
    for (int n = 0; n < N; ++n) na += nacc[n];
    printf("am_ref main: status %d, checksum %.17g, accepted %llu of %d, fallbacks %lld, finite %d\n", st, cs, (unsigned long long)na, N * STEPS,
           (long long)fallbacks, finite);
    free(X); free(G); free(LT); free(C); free(M); free(M2); free(step); free(acc); free(prop); free(tot); free(held); free(nacc); free(mask);
    free(sum); free(sumsq); free(hist); free(hist_lt);
    return st == 0 && finite && fallbacks > 0 ? 0 : 1;
}
