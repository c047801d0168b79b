/* Host side of tests/test_mala_screen_host.py: the rejection screen of the 4-lane MALA table kernel (klara.jl_amd/csrc/klara_mala_screen.h) as the
 * kernel calls it — TEST INFRASTRUCTURE.  Compiled at test time: gcc -O2 -std=gnu11 -ffp-contract=off, as a shared library for ctypes, and with
 * -DMS_MAIN as a program of its own (the sanitizer run: -fsanitize=address,undefined). */
#include <stdint.h>
#include <string.h>
#include "klara_mala_screen.h"

#define MS_NP 13
#define MS_Q 4
#define MS_E (2 * MS_NP * MS_Q)          /* 104 element slots of a chain: element 2 (p Q + q) + j sits in lane q, pair p, half j */

int ms_consts(double h, double s, double c, double* out5)
{
    const kd_mala_screen_k k = kd_mala_screen_consts(h, s, c);
    out5[0] = k.K0; out5[1] = k.K1; out5[2] = k.K2; out5[3] = k.T0; out5[4] = k.T2;
    return k.on;
}

/* the screen of one chain the way k_diagt runs it: per lane sum x^2, sum x z, sum z^2 as fma chains over the lane's elements, the lane's shares
 * of est and T, the butterfly over the four lanes, the decision */
static int ms_one(const kd_mala_screen_k* k, int D, const double* x, const double* z, double lt, double gconst, double lg, double* est, double* T)
{
    double e[MS_Q], t[MS_Q];
    for (int q = 0; q < MS_Q; ++q) {
        double sxx = 0.0, sxz = 0.0, szz = 0.0;
        for (int p = 0; p < MS_NP; ++p)
            for (int j = 0; j < 2; ++j) {
                const int i = 2 * (p * MS_Q + q) + j;
                const double xv = i < D ? x[i] : 0.0;
                sxx = kd_fma(xv, xv, sxx);
            }
        for (int p = 0; p < MS_NP; ++p) {
            const int i = 2 * (p * MS_Q + q);
            const double x0 = i < D ? x[i] : 0.0, x1 = i + 1 < D ? x[i + 1] : 0.0, z0 = i < D ? z[i] : 0.0, z1 = i + 1 < D ? z[i + 1] : 0.0;
            sxz = kd_fma(x0, z0, sxz); sxz = kd_fma(x1, z1, sxz);
            szz = kd_fma(z0, z0, szz); szz = kd_fma(z1, z1, szz);
        }
        e[q] = kd_mala_screen_e(k->K0, k->K1, k->K2, sxx, sxz, szz);
        t[q] = kd_mala_screen_t(k->T0, k->T2, sxx, szz);
    }
    const double es = (e[0] + e[1]) + (e[2] + e[3]), ts = (t[0] + t[1]) + (t[2] + t[3]);
    return k->on && kd_mala_screen_decide(es, ts, lt, gconst, lg, est, T);
}

/* n chains, x and z row-major n x D; certain[i] = 1: certainly rejected.  Returns the launch's `on`. */
int ms_screen(int64_t n, int D, const double* x, const double* z, const double* lt, double gconst, const double* lg,
              double h, double s, double c, int32_t* certain, double* est, double* T)
{
    const kd_mala_screen_k k = kd_mala_screen_consts(h, s, c);
    for (int64_t i = 0; i < n; ++i) certain[i] = ms_one(&k, D, x + i * D, z + i * D, lt[i], gconst, lg[i], &est[i], &T[i]);
    return k.on;
}

/* MALA.jl:83-92 on lt = gconst - sum x^2 in the operation order of k_diagt<MALA, 13, 4, .., UNITW>: two partial sums per lane (even and odd
 * pairs), the butterfly, the sum of the two partials — a restatement in C for the stand-alone run; the Python tests hold it to their NumPy one */
double ms_literal_ratio(int D, const double* x, const double* z, double lt, double gconst, double h, double s, double c)
{
    double red[3][2][MS_Q];
    const double neg_h = -h;
    for (int q = 0; q < MS_Q; ++q) {
        for (int r = 0; r < 2; ++r) { red[0][r][q] = 0.0; red[1][r][q] = 0.0; red[2][r][q] = 0.0; }
        for (int p = 0; p < MS_NP; ++p)
            for (int j = 0; j < 2; ++j) {
                const int i = 2 * (p * MS_Q + q) + j, r = p & 1;
                const double xv = i < D ? x[i] : 0.0, zv = i < D ? z[i] : 0.0;
                const double m = xv + neg_h * xv;
                const double xe = m + s * zv;
                red[0][r][q] = red[0][r][q] + xe * xe;
                const double q1 = m - xe;
                red[1][r][q] = red[1][r][q] + (q1 * q1) * c;
                const double mup = xe + neg_h * xe;
                const double q2 = mup - xv;
                red[2][r][q] = red[2][r][q] + (q2 * q2) * c;
            }
    }
    double tot[3];
    for (int v = 0; v < 3; ++v) {
        double part[2];
        for (int r = 0; r < 2; ++r) part[r] = (red[v][r][0] + red[v][r][1]) + (red[v][r][2] + red[v][r][3]);
        tot[v] = part[0] + part[1];
    }
    const double ltp = gconst - tot[0];
    double ratio = ltp - lt;
    ratio += tot[1];
    ratio -= tot[2];
    return ratio;
}

void ms_literal(int64_t n, int D, const double* x, const double* z, const double* lt, double gconst, double h, double s, double c, double* ratio)
{
    for (int64_t i = 0; i < n; ++i) ratio[i] = ms_literal_ratio(D, x + i * D, z + i * D, lt[i], gconst, h, s, c);
}

#ifdef MS_MAIN
/* The soundness check on draws of its own: "certain" implies that the literal test rejects, and NaN / infinite inputs are never certain.
 * Exit status 0: no violation. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static uint64_t ms_state = 0x9E3779B97F4A7C15ull;
static uint64_t ms_next(void)
{
    uint64_t v = (ms_state += 0x9E3779B97F4A7C15ull);
    v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull; v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
    return v ^ (v >> 31);
}
static double ms_unif(void) { return ((double)(ms_next() >> 11) + 0.5) * 0x1p-53; }
static double ms_normal(void) { return sqrt(-2.0 * log(ms_unif())) * cos(6.283185307179586 * ms_unif()); }

int main(void)
{
    static const double steps[4] = { 0.9, 0.3, 0.02, 1.5 };
    static const int dims[3] = { 97, 100, 104 };
    const double guard = KD_LOG_UMIN_GUARD;
    long long ncertain = 0, nreject = 0, bad = 0, total = 0;
    for (int n = 0; n < 100000; ++n) {
        const int D = dims[n % 3];
        const double h = n < 70000 ? 0.9 : steps[1 + n % 3], s = sqrt(h), c = 0.5 * (1.0 / h), gconst = (n & 8) ? -3.25 : 0.0;
        const kd_mala_screen_k k = kd_mala_screen_consts(h, s, c);
        double* x = (double*)malloc(sizeof(double) * (size_t)D);       /* exact-size blocks: an index past D is an error the sanitizer sees */
        double* z = (double*)malloc(sizeof(double) * (size_t)D);
        if (!x || !z || !k.on) return 2;
        double sx = 0.0;
        for (int i = 0; i < D; ++i) { x[i] = sqrt(0.5) * ms_normal(); z[i] = ms_normal(); sx += x[i] * x[i]; }
        double lt = gconst - sx;
        const int kind = n % 50;
        if (kind == 7) x[n % D] = 0.0;
        if (kind == 8) x[n % D] = 0x1p-1060;
        if (kind == 9) lt = 5.0 * ms_normal();                           /* lt at odds with x */
        const int poison = kind >= 40 && kind < 46;
        if (kind == 40) x[n % D] = NAN;
        if (kind == 41) x[n % D] = INFINITY;
        if (kind == 42) z[n % D] = NAN;
        if (kind == 43) z[n % D] = -INFINITY;
        if (kind == 44) lt = -INFINITY;
        if (kind == 45) lt = NAN;
        const double u = ms_unif();
        const double lg = D == 104 ? guard : (kind == 10 ? log1p(-0x1p-45) : kind == 11 ? log(0x1p-45) : log(u));
        double est, T;
        const int certain = ms_one(&k, D, x, z, lt, gconst, lg, &est, &T);
        const double ratio = ms_literal_ratio(D, x, z, lt, gconst, h, s, c);
        const int accepts = ratio > 0.0 || ratio > lg;
        ++total; ncertain += certain; nreject += !accepts;
        if (certain && (accepts || poison)) { ++bad; printf("violation at draw %d: D %d h %g ratio %.17g lg %.17g est %.17g T %.17g\n", n, D, h, ratio, lg, est, T); }
        free(x); free(z);
    }
    printf("draws %lld literal rejections %lld certain %lld violations %lld\n", total, nreject, ncertain, bad);
    return bad ? 1 : 0;
}
#endif
