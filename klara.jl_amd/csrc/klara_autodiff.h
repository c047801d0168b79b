// klara_autodiff.h — forward-mode automatic differentiation of a user-defined target (KLARA_TARGET_CUSTOM), the device form of the
// reference's `diffopts=DiffOptions(mode=:forward)` (src/autodiff/forward.jl, BasicContMuvParameter.jl:627-694).
//
// A source that starts with `#define KLARA_USER_AUTODIFF 1` defines no gradient.  Its log-target is generic in its scalar type:
//
//   template <class T, class V>
//   KLARA_USER_FN T klara_user_logtarget_ad(const V& x, int D, const double* data, long long ndata);
//
// (with `#define KLARA_USER_LIKELIHOOD_PRIOR 1`: klara_user_loglikelihood_ad and klara_user_logprior_ad of the same shape).  `x` is an indexable
// view: x[i] yields a T built from the stored double, seeded where i is one of the directions in flight, so the vector never exists as duals.
// `#define KLARA_USER_AUTODIFF 2` also asks for the SMMALA metric, the upper triangle of MINUS the Hessian (forward.jl:11-16), by nested duals.
// `#define KLARA_USER_AUTODIFF_CHUNK n` fixes the width of a sweep (DiffOptions.chunksize; 0 or absent: the library's choice).
//
// This file has two parts.  The first, the dual arithmetic, is compiled BEFORE the user's text; the second (KLARA_AUTODIFF_GLUE defined, the
// file included again) AFTER it: there klara_user_logtarget / klara_user_gradlogtarget / klara_user_tensorlogtarget — the closures the
// kernels (klara_custom.h), klara_custom_compose.h and the CPU references call — are written in terms of the user's generic function.
// Both parts compile as C++17 under the run-time compiler and under a host g++ -ffp-contract=off.
//
// The contract of the rules below:
//  (A1) the value part of every rule is the operation itself, so the T = double instantiation of a user's function and the value a dual
//       carries through it are the same bits;
//  (A2) no rule mixes partials: partial k of a result is a function of the operands' values and their partials k alone, so a gradient
//       does not depend on the width of a sweep, on which lane sweeps which directions, or on the order of the sweeps.
// Every rule is plain IEEE + - * / sqrt and kd_* calls of the inner type (detmath.h); there is no libm call and nothing contracts.
#ifndef KLARA_AUTODIFF_H
#define KLARA_AUTODIFF_H
#include "detmath.h"

#if defined(__HIPCC__)
#define KAD_FN __host__ __device__ __forceinline__
#define KAD_UNROLL _Pragma("unroll")
#else
#define KAD_FN inline __attribute__((always_inline))
#define KAD_UNROLL
#endif

template <class T, int C>
struct klara_dual {
    T v;            // value
    T d[C];         // partials along the C directions in flight
    KAD_FN klara_dual() {}
    KAD_FN klara_dual(double c) : v(c) { KAD_UNROLL for (int k = 0; k < C; ++k) d[k] = T(0.0); }       // a constant
};

// ---- + - * / between duals and doubles, in either order
template <class T, int C> KAD_FN klara_dual<T, C> operator+(const klara_dual<T, C>& a, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = a.v + b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] + b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator+(const klara_dual<T, C>& a, double c)
{
    klara_dual<T, C> r; r.v = a.v + c;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator+(double c, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = c + b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator-(const klara_dual<T, C>& a)
{
    klara_dual<T, C> r; r.v = -a.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = -a.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator-(const klara_dual<T, C>& a, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = a.v - b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] - b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator-(const klara_dual<T, C>& a, double c)
{
    klara_dual<T, C> r; r.v = a.v - c;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator-(double c, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = c - b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = -b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator*(const klara_dual<T, C>& a, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = a.v * b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator*(const klara_dual<T, C>& a, double c)
{
    klara_dual<T, C> r; r.v = a.v * c;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] * c;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator*(double c, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = c * b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = c * b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator/(const klara_dual<T, C>& a, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = a.v / b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator/(const klara_dual<T, C>& a, double c)
{
    klara_dual<T, C> r; r.v = a.v / c;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] / c;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> operator/(double c, const klara_dual<T, C>& b)
{
    klara_dual<T, C> r; r.v = c / b.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = (-(r.v * b.d[k])) / b.v;
    return r;
}

// ---- comparisons: on the value
KAD_FN double klara_ad_value(double a) { return a; }
template <class T, int C> KAD_FN double klara_ad_value(const klara_dual<T, C>& a) { return klara_ad_value(a.v); }
#define KLARA_AD_COMPARE(op) \
    template <class T, int C> KAD_FN bool operator op(const klara_dual<T, C>& a, const klara_dual<T, C>& b) { return klara_ad_value(a) op klara_ad_value(b); } \
    template <class T, int C> KAD_FN bool operator op(const klara_dual<T, C>& a, double b) { return klara_ad_value(a) op b; } \
    template <class T, int C> KAD_FN bool operator op(double a, const klara_dual<T, C>& b) { return a op klara_ad_value(b); }
KLARA_AD_COMPARE(<) KLARA_AD_COMPARE(>) KLARA_AD_COMPARE(<=) KLARA_AD_COMPARE(>=) KLARA_AD_COMPARE(==) KLARA_AD_COMPARE(!=)
#undef KLARA_AD_COMPARE

// ---- sqrt, fabs (the double forms: IEEE square root, sign bit), so that a generic function may call them on either scalar type
#if !defined(__HIPCC_RTC__)
#include <cmath>
using std::sqrt;
using std::fabs;
#endif
template <class T, int C> KAD_FN klara_dual<T, C> sqrt(const klara_dual<T, C>& a)
{
    klara_dual<T, C> r; r.v = sqrt(a.v);
    const T twice = 2.0 * r.v;
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] / twice;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> fabs(const klara_dual<T, C>& a)
{
    const bool neg = klara_ad_value(a) < 0.0;
    klara_dual<T, C> r; r.v = fabs(a.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = neg ? -a.d[k] : a.d[k];
    return r;
}

// ---- kd_fma(a, b, c) = a b + c in one rounding; every mix of duals and doubles
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(const klara_dual<T, C>& a, const klara_dual<T, C>& b, const klara_dual<T, C>& c)
{
    klara_dual<T, C> r; r.v = kd_fma(a.v, b.v, c.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = kd_fma(a.d[k], b.v, kd_fma(a.v, b.d[k], c.d[k]));
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(const klara_dual<T, C>& a, const klara_dual<T, C>& b, double c)
{
    klara_dual<T, C> r; r.v = kd_fma(a.v, b.v, c);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = kd_fma(a.d[k], b.v, a.v * b.d[k]);
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(double a, const klara_dual<T, C>& b, const klara_dual<T, C>& c)
{
    klara_dual<T, C> r; r.v = kd_fma(a, b.v, c.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = kd_fma(a, b.d[k], c.d[k]);
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(const klara_dual<T, C>& a, double b, const klara_dual<T, C>& c)
{
    klara_dual<T, C> r; r.v = kd_fma(a.v, b, c.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = kd_fma(a.d[k], b, c.d[k]);
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(double a, const klara_dual<T, C>& b, double c)
{
    klara_dual<T, C> r; r.v = kd_fma(a, b.v, c);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a * b.d[k];
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(const klara_dual<T, C>& a, double b, double c)
{
    klara_dual<T, C> r; r.v = kd_fma(a.v, b, c);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] * b;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_fma(double a, double b, const klara_dual<T, C>& c)
{
    klara_dual<T, C> r; r.v = kd_fma(a, b, c.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = c.d[k];
    return r;
}

// ---- the transcendental functions of detmath.h
template <class T, int C> KAD_FN klara_dual<T, C> kd_exp(const klara_dual<T, C>& a)          // exp' = exp
{
    klara_dual<T, C> r; r.v = kd_exp(a.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] * r.v;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_log(const klara_dual<T, C>& a)          // log' = 1 / x
{
    klara_dual<T, C> r; r.v = kd_log(a.v);
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] / a.v;
    return r;
}
template <class T, int C> KAD_FN klara_dual<T, C> kd_erf(const klara_dual<T, C>& a)          // erf' = 2 / sqrt(pi) exp(-x^2)
{
    klara_dual<T, C> r; r.v = kd_erf(a.v);
    const T slope = 1.1283791670955126 * kd_exp(-(a.v * a.v));
    KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = a.d[k] * slope;
    return r;
}
// softplus' = logistic, logistic' = logistic (1 - logistic)
template <class T, int C> KAD_FN void kd_softplus_logistic_rows(const klara_dual<T, C>& a, klara_dual<T, C>* softplus, klara_dual<T, C>* logistic)
{
    T sp, lg;
    kd_softplus_logistic_rows(a.v, &sp, &lg);
    const T slope = lg * (1.0 - lg);
    softplus->v = sp; logistic->v = lg;
    KAD_UNROLL for (int k = 0; k < C; ++k) { softplus->d[k] = a.d[k] * lg; logistic->d[k] = a.d[k] * slope; }
}

// ---- the views a generic function indexes
// (T = double: the function is handed the `const double*` itself)
// first order: directions k0 .. k0 + C - 1 are in flight
template <int C>
struct klara_ad_view {
    const double* p; int k0;
    KAD_FN klara_dual<double, C> operator[](int i) const
    {
        klara_dual<double, C> r; r.v = p[i];
        KAD_UNROLL for (int k = 0; k < C; ++k) r.d[k] = (i == k0 + k) ? 1.0 : 0.0;
        return r;
    }
};
// second order: direction a outside, directions b0 .. b0 + CB - 1 inside; of a result r, r.v.v is the value, r.v.d[k] the partial along b0 + k,
// r.d[0].v the partial along a and r.d[0].d[k] the second partial along (a, b0 + k)
template <int CB>
struct klara_ad_view2 {
    const double* p; int a, b0;
    KAD_FN klara_dual<klara_dual<double, CB>, 1> operator[](int i) const
    {
        klara_dual<klara_dual<double, CB>, 1> r;
        r.v.v = p[i]; r.d[0].v = (i == a) ? 1.0 : 0.0;
        KAD_UNROLL for (int k = 0; k < CB; ++k) { r.v.d[k] = (i == b0 + k) ? 1.0 : 0.0; r.d[0].d[k] = 0.0; }
        return r;
    }
};
#endif /* KLARA_AUTODIFF_H */

// =====================================================================================================================================
// the glue: after the user's text
#if defined(KLARA_AUTODIFF_GLUE) && !defined(KLARA_AUTODIFF_GLUE_DONE)
#define KLARA_AUTODIFF_GLUE_DONE
#ifndef KLARA_USER_AUTODIFF
#error "klara_autodiff.h: the glue needs a source that starts with #define KLARA_USER_AUTODIFF 1 (or 2)"
#endif
// The width of a sweep where one lane (or the host) holds the whole vector.  Candidates 1, 2, 4, 8 and D (profiles/autodiff.txt): D — one evaluation,
// the function's transcendental parts computed once — measured fastest wherever it was tried (D = 4: 1.15 x the hand-written gradient's time against 1.46 x
// at 2; D = 9: 1.39 x against 1.97 x at 4 and 2.13 x at 8) and keeps every test target up to 16 dimensions out of scratch memory; beyond 16 dimensions D-wide
// duals spill (D = 32: 960 B of scratch against 512 B at 8, where the hand-written kernel has 496 B), so the width is 8 there.
#if !defined(KLARA_USER_AUTODIFF_CHUNK) || (KLARA_USER_AUTODIFF_CHUNK + 0) <= 0
#define KLARA_AD_USER_CHUNK 0
#define KLARA_AD_CHUNK (KLARA_D <= 16 ? KLARA_D : 8)
#else
#define KLARA_AD_USER_CHUNK (KLARA_USER_AUTODIFF_CHUNK)
#define KLARA_AD_CHUNK ((KLARA_USER_AUTODIFF_CHUNK) < KLARA_D ? (KLARA_USER_AUTODIFF_CHUNK) : KLARA_D)
#endif
#if defined(__HIPCC__) && KLARA_D <= 32
#define KLARA_AD_UNROLL_SWEEPS _Pragma("unroll")
#else
#define KLARA_AD_UNROLL_SWEEPS
#endif

// gradient of FN_AD at x (KLARA_D doubles), ceil(D / C) sweeps of C-wide duals; by (A2) the same bits at every C
#define KLARA_AD_DEFINE_GRAD(NAME, FN_AD) \
    KLARA_USER_FN void NAME(const double* x, int D, const double* data, long long ndata, double* g) \
    { \
        constexpr int C = KLARA_AD_CHUNK; \
        KLARA_AD_UNROLL_SWEEPS \
        for (int k0 = 0; k0 < KLARA_D; k0 += C) { \
            const klara_ad_view<C> view = { x, k0 }; \
            const klara_dual<double, C> r = FN_AD<klara_dual<double, C> >(view, D, data, ndata); \
            KAD_UNROLL for (int k = 0; k < C; ++k) if (k0 + k < KLARA_D) g[k0 + k] = r.d[k]; \
        } \
    }

#ifdef KLARA_USER_LIKELIHOOD_PRIOR
KLARA_USER_FN double klara_user_loglikelihood(const double* x, int D, const double* data, long long ndata)
{
    return klara_user_loglikelihood_ad<double>(x, D, data, ndata);
}
KLARA_USER_FN double klara_user_logprior(const double* x, int D, const double* data, long long ndata)
{
    return klara_user_logprior_ad<double>(x, D, data, ndata);
}
#ifndef KLARA_CUSTOM_NOGRAD
KLARA_AD_DEFINE_GRAD(klara_user_gradloglikelihood, klara_user_loglikelihood_ad)
KLARA_AD_DEFINE_GRAD(klara_user_gradlogprior, klara_user_logprior_ad)
#endif
#else
KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long ndata)
{
    return klara_user_logtarget_ad<double>(x, D, data, ndata);
}
#ifndef KLARA_CUSTOM_NOGRAD
KLARA_AD_DEFINE_GRAD(klara_user_gradlogtarget, klara_user_logtarget_ad)
#endif
#if (KLARA_USER_AUTODIFF + 0) >= 2 && defined(KLARA_SMMALA)
// the metric of the SMMALA sampler: minus the Hessian (forward.jl:11-16), row a from one evaluation with direction a outside and a chunk of
// directions inside; the row-major D x D matrix klara_user_tensorlogtarget fills (its upper triangle is read)
#ifndef KLARA_AD_CHUNK2
#define KLARA_AD_CHUNK2 KLARA_AD_CHUNK
#endif
KLARA_USER_FN void klara_user_tensorlogtarget(const double* x, int D, const double* data, long long ndata, double* G)
{
    constexpr int CB = KLARA_AD_CHUNK2;
    KLARA_AD_UNROLL_SWEEPS
    for (int a = 0; a < KLARA_D; ++a) {
        KLARA_AD_UNROLL_SWEEPS
        for (int b0 = 0; b0 < KLARA_D; b0 += CB) {
            if (b0 + CB <= a) { KAD_UNROLL for (int k = 0; k < CB; ++k) G[a * KLARA_D + b0 + k] = 0.0; continue; }      // (below the diagonal: not read)
            const klara_ad_view2<CB> view = { x, a, b0 };
            const klara_dual<klara_dual<double, CB>, 1> r = klara_user_logtarget_ad<klara_dual<klara_dual<double, CB>, 1> >(view, D, data, ndata);
            KAD_UNROLL for (int k = 0; k < CB; ++k) if (b0 + k < KLARA_D) G[a * KLARA_D + b0 + k] = -r.d[0].d[k];
        }
    }
}
#endif
#endif
#endif /* KLARA_AUTODIFF_GLUE */
