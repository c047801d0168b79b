/* klara_mala_screen.h — "certainly rejected" for a MALA proposal on lt = gconst - sum x_i^2, from two sums of the proposal's normals.
 *
 * Host and device, plain C (KD_FN as in detmath.h).  Used by the 4-lane table kernel of klara_diagt.h (diagt_mala_screen) and, compiled by
 * gcc, by tests/test_mala_screen_host.py.
 *
 * What the kernel computes (k_diagt, MALA branch, unit weights; fl = one IEEE rounding; h the step, s = sqrt_step0, c = 0.5 * inv_step0):
 *     m  = fl(x + fl(-h x))            xe = fl(m + fl(s z))            red0 += fl(xe xe)
 *     q1 = fl(m - xe)                  red1 += fl(fl(q1 q1) c)
 *     mp = fl(xe + fl(-h xe))          q2 = fl(mp - x)                 red2 += fl(fl(q2 q2) c)
 *     ratio = fl(fl(fl(fl(gconst - red0) - lt) + red1) - red2)         rejected  <=>  not (ratio > 0 or ratio > lg),  lg = log u < 0
 * In real arithmetic, with a = 1 - h and b = a^2 - 1:  xe = a x + s z,  q1 = -s z,  q2 = b x + a s z, so with P = sum x^2, S = sum x z,
 * R = sum z^2
 *     ratio = (gconst - lt) + K0 P + K1 S + K2 R,    K0 = -(a^2 + c b^2),  K1 = -2 a s (1 + c b),  K2 = -s^2 (1 + c b)       (= est)
 * and the magnitudes of its terms before any of them cancels, with |S| <= (P + R) / 2, add up to
 *     T = |gconst| + |lt| + |lg| + T0 P + T2 R,      T0 = a^2 + |a| s + c b^2 + c |b| |a| s,
 *                                                    T2 = s^2 + |a| s + c s^2 + c |b| |a| s + c a^2 s^2.
 * The screen answers "certainly rejected" when est + 2^-30 T <= lg.
 *
 * Claim.  For every launch whose constants pass kd_mala_screen_consts (`on`), and T <= 2^1000:  |est_computed - ratio_computed| <= 2^-44 T.
 * Proof (u = 2^-53; X = |x|, Z = |z| of one element; terms of order u^2 are left to the slack at the end).  `on` gives 2^-6 <= h <= 2, hence
 * |a| <= 1 and |b| = h |2 - h| <= 2 h; it checks s^2 = h and c h = 1/2 to 2^-50, hence c |b| <= 1 and c s^2 = 1/2 to that precision.  Let
 * mu = h + |a|,  W = mu X + s Z,  V = |b| X + |a| s Z;  then |a x + s z| <= W and |q2| <= V in the reals.
 *   m:   two roundings, |m - a x| <= u (h X + |a| X) = u mu X.              xe:  |xe - (a x + s z)| <= u mu X + u s Z + u W = 2 u W.
 *   red0 term:  |fl(xe^2) - (a x + s z)^2| <= 2 W (2 u W) + u W^2 = 5 u W^2.
 *   q1:  m - xe = -fl(s z) - (xe's rounding), so |q1 + s z| <= u s Z + u W + u s Z <= 3 u W;  term: c (2 u s^2 Z^2 + 2 s Z 3 u W) <= 8 u c s Z W.
 *   mp:  as m (this is where m = x + (-h) x stands against a x: the error is u mu |xe|, not u |a| |xe|), |mp - a xe| <= u mu W;
 *   q2:  |q2 - (b x + a s z)| <= |a| 2 u W + u mu W + u V <= u (3 mu W + V);  term: c (2 u V^2 + 2 V u (3 mu W + V)) = u c (4 V^2 + 6 mu V W).
 *   Multiplied out with c |b| <= 1 and c s^2 = 1/2 the four bounds add up, per element, to u (e0 X^2 + exz X Z + e2 Z^2) with
 *       e0 = 11 mu^2 + 4 |b|,   exz = s (16 mu + 8 |a| + c mu (8 + 6 mu |a|)),   e2 = 5 s^2 + 4 + 2 a^2 + 3 mu |a|,
 *   and X Z <= (X^2 + Z^2) / 2 makes that u (E0 X^2 + E2 Z^2), E0 = e0 + exz / 2, E2 = e2 + exz / 2.  `on` checks E0 <= 96 T0 and E2 <= 96 T2
 *   numerically (true on all of [2^-6, 2]: the largest quotients are 63.6, at h = 1.81, and 30.8, at h = 2^-6; the test sweeps the range), so the elementwise
 *   errors of a chain are at most 96 u (T0 P + T2 R).
 *   Sums: every partial sum adds non-negative terms, at most 26 per lane, two butterfly steps and the sum of the two partials: at most 104 u
 *   of the exact sums, which T holds in full (a^2 P + 2 |a| s |S| + s^2 R <= (a^2 + |a| s) P + (s^2 + |a| s) R, and so on): 104 u T.
 *   The four operations of ratio: each result is at most T in magnitude: 4 u T.
 *   est itself: K0, K1, K2 carry at most 12 u of T0, T0 + T2, T2 (1 + c b is formed from c b ~ -1 + h/2: 3 u absolute, against the |a| s and
 *   s^2 that T0 and T2 hold); the three sums are fma chains of at most 26 terms and two butterfly steps, 30 u of P, (P + R) / 2, R; the fmas
 *   that join them and the two additions at most 6 u T: under 48 u T.
 *   Together (96 + 104 + 4 + 48) u T = 252 u T < 2^-45 T; the dropped second-order terms are below u of that.  Underflow: a product that goes
 *   subnormal is off by at most 2^-1074, under 600 of them per chain, against 2^-44 T >= 2^-44 |lg| >= 2^-89 (|lg| >= -log(1 - 2^-45) > 2^-46).
 *   Overflow: `on` has T0, T2 >= 1/4, so T <= 2^1000 bounds P and R by 2^1002 and every intermediate (coefficients under 2^8) stays finite;
 *   a T that is NaN, infinite or above 2^1000 — any NaN or infinity in x, z, lt, lt = -inf — answers "not certain".
 * Decision.  est + 2^-30 T <= lg, the sum and the product rounded (2 u T more), gives ratio_computed <= est + 2^-44 T < lg < 0: the kernel's own
 * test rejects.  The margin is 2^14 times the bound.  Where the accept draw is not in hand, lg is KD_LOG_UMIN_GUARD: ratio_computed <= guard
 * and the kernel rejects without drawing.  Every comparison is written so that a NaN makes it false.
 */
#ifndef KLARA_MALA_SCREEN_H
#define KLARA_MALA_SCREEN_H

#include "detmath.h"

#define KD_MALA_SCREEN_H_MIN 0.015625      /* 2^-6: the step range the bound is proven for */
#define KD_MALA_SCREEN_H_MAX 2.0
#define KD_MALA_SCREEN_MARGIN 9.313225746154785e-10     /* 2^-30 */
#define KD_MALA_SCREEN_T_MAX 1.0715086071862673e+301    /* 2^1000 */
#define KD_MALA_SCREEN_ELEM_FACTOR 96.0

typedef struct {
    double K0, K1, K2;      /* est = (gconst - lt) + K0 P + K1 S + K2 R */
    double T0, T2;          /* T = |gconst| + |lt| + |lg| + T0 P + T2 R */
    int on;                 /* launch-uniform: the bound is proven for these constants */
} kd_mala_screen_k;

KD_FN double kd_mala_screen_abs(double v) { return __builtin_fabs(v); }

/* the launch constants from the step and the kernel's own sqrt(h) and 0.5 / h */
KD_FN kd_mala_screen_k kd_mala_screen_consts(double h, double s, double c)
{
    kd_mala_screen_k k;
    const double a = 1.0 - h, a2 = a * a, b = a2 - 1.0, aa = kd_mala_screen_abs(a), ab = kd_mala_screen_abs(b);
    const double cb = c * b, one_cb = 1.0 + cb, s2 = s * s;
    k.K0 = -(a2 + cb * b);
    k.K1 = -2.0 * (a * s) * one_cb;
    k.K2 = -s2 * one_cb;
    const double cross = c * ab * aa * s;
    k.T0 = a2 + aa * s + c * (b * b) + cross;
    k.T2 = s2 + aa * s + c * s2 + cross + c * (a2 * s2);
    /* the proof's elementwise error coefficients, held against T0 and T2 */
    const double mu = h + aa;
    const double exz = s * (16.0 * mu + 8.0 * aa + c * mu * (8.0 + 6.0 * mu * aa));
    const double E0 = 11.0 * (mu * mu) + 4.0 * ab + 0.5 * exz;
    const double E2 = 5.0 * s2 + 4.0 + 2.0 * a2 + 3.0 * mu * aa + 0.5 * exz;
    const double tiny = 8.881784197001252e-16;    /* 2^-50 */
    int on = h >= KD_MALA_SCREEN_H_MIN && h <= KD_MALA_SCREEN_H_MAX;          /* (a subnormal, zero, negative, infinite or NaN step fails here) */
    on = on && kd_mala_screen_abs(s2 - h) <= tiny * h && kd_mala_screen_abs(c * h - 0.5) <= tiny;
    on = on && k.T0 >= 0.25 && k.T2 >= 0.25;
    on = on && E0 <= KD_MALA_SCREEN_ELEM_FACTOR * k.T0 && E2 <= KD_MALA_SCREEN_ELEM_FACTOR * k.T2;
    k.on = on;
    return k;
}

/* a lane's (or a chain's) share of est and of T: linear in the sums, so the shares of a chain's lanes are added up */
KD_FN double kd_mala_screen_e(double K0, double K1, double K2, double sxx, double sxz, double szz) { return kd_fma(K0, sxx, kd_fma(K1, sxz, K2 * szz)); }
KD_FN double kd_mala_screen_t(double T0, double T2, double sxx, double szz) { return kd_fma(T0, sxx, T2 * szz); }

/* e, ts: the chain's sums of the two shares.  1: the kernel's accept test certainly fails.  (est and T are handed back for the host tests.) */
KD_FN int kd_mala_screen_decide(double e, double ts, double lt, double gconst, double lg, double* est_out, double* t_out)
{
    const double est = (gconst - lt) + e;
    const double T = ((kd_mala_screen_abs(gconst) + kd_mala_screen_abs(lt)) + kd_mala_screen_abs(lg)) + ts;
    if (est_out) *est_out = est;
    if (t_out) *t_out = T;
    return (T <= KD_MALA_SCREEN_T_MAX) && (est + KD_MALA_SCREEN_MARGIN * T <= lg);
}

/* the whole screen from a chain's three sums */
KD_FN int kd_mala_screen_certain(const kd_mala_screen_k* k, double sxx, double sxz, double szz, double lt, double gconst, double lg,
                                 double* est_out, double* t_out)
{
    const int r = kd_mala_screen_decide(kd_mala_screen_e(k->K0, k->K1, k->K2, sxx, sxz, szz), kd_mala_screen_t(k->T0, k->T2, sxx, szz),
                                        lt, gconst, lg, est_out, t_out);
    return k->on && r;
}

#endif
