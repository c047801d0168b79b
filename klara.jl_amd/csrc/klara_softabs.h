// klara_softabs.h — the softabs transform of the SMMALA metric (src/stats/metrics.jl:1-4), one matrix per lane, in the lane's registers:
//
//     softabs(H, a) = Q diag(lambda ./ tanh(a lambda)) Q',   H = Q diag(lambda) Q'
//
// the `transform` of SMMALA(driftstep, H -> softabs(H, a)) (samplers/SMMALA.jl:129,167-168, iterate/SMMALA.jl:117-118).  It makes a positive
// definite metric of any finite symmetric matrix: an eigenvalue lambda becomes about |lambda| where |a lambda| is large and 1 / a where it is small.
//
// Plain IEEE operations and kd_* calls only (no libm, nothing that contracts: build with -ffp-contract=off), in the C subset hiprtc, hipcc
// and a host C compiler accept, so that tests/softabs_ref.c runs the same operations in the same order and a chain's bits are the same on
// the host and on the device.  Everything here is a function of ONE chain's matrix: the loops are the lane's own (a lane that has converged
// leaves the sweep loop and is masked while the wavefront's other lanes go on), no value crosses lanes, so the bits of a chain
// do not depend on the chains that share its wavefront.  With D and E constants at the call (the run-time compiled kernels: KLARA_D) every
// loop unrolls and the arrays are registers (the eigenvectors are work space of the caller's: registers, or LDS from D = 5 on — klara_kernels.h).
//
// Deviations from the reference:
//  T1  cyclic Jacobi in a fixed pivot order instead of LAPACK's eig.  softabs(H) is a function of H alone (f is applied to the spectrum), so the sign and the
//      order of the eigenvectors cannot matter; the two differ by rounding only.
//  T2  f(0) = 1 / a, the limit, where the reference computes 0 / 0.
//  T3  only the upper triangle of the matrix is read.
//  T4  a matrix with a non-finite entry (or one beyond 2^500, whose square overflows) is not transformed: the result carries a NaN, the
//      factorisation's pivot check fails and the proposal is rejected (S4) or the start state refused (S5).
//  T5  f is evaluated from t = exp(-2 |a lambda|) and a series near 0 (below), not by libm's tanh.
#ifndef KLARA_SOFTABS_H
#define KLARA_SOFTABS_H
#include "detmath.h"

#if defined(__clang__)
#define KSA_UNROLL _Pragma("unroll")
#else
#define KSA_UNROLL _Pragma("GCC unroll 8")
#endif
#define KSA_MAXD 8
// Sweeps: a sweep is the D (D - 1) / 2 rotations (p, q), p ascending, q ascending.  A lane stops before the first sweep at which
//     sum_{p<q} A_pq^2 <= 2^-106 sum_p A_pp^2,
// i.e. when the off-diagonal Frobenius norm is below sqrt(2) 2^-53 of the diagonal's: by Weyl's inequality every eigenvalue is then within that of a diagonal
// entry, which is the rounding of the diagonal entries themselves.  Cyclic Jacobi converges quadratically once the off-diagonal norm is below
// the smallest eigenvalue gap, and rotations only re-fill annihilated entries with products of small entries (no rounding floor from the diagonal), so the
// test is met; 7 sweeps are typical at D = 8 and 12 have been seen on clustered spectra.  The cap is 32 — a guard against a loop without end, not a tuning
// parameter: it costs nothing when it is not reached (tests/test_softabs_host.py asserts it never is on its matrices), and a lane that did reach it
// would carry on with an orthogonal Q and a nearly diagonal A, i.e. a symmetric positive matrix that the pivot check still examines.
#define KSA_MAX_SWEEPS 32
#define KSA_TOL2 0x1p-106
#define KSA_BIG 0x1p500
// below this |a lambda| the series, above it the exponential form
#define KSA_SMALL 0.5

KD_FN int ksa_tri(int a, int b, int E) { return a * E - (a * (a - 1)) / 2 + (b - a); }
KD_FN double ksa_abs(double v) { return v < 0.0 ? -v : v; }

// f(lambda) = lambda / tanh(a lambda), a > 0: even in lambda, 1 / a at 0, |lambda| for large |a lambda|.
//  |a lambda| >= 1/2:  |lambda| (1 + t) / (1 - t), t = kd_exp(-2 |a lambda|) <= 0.368: no cancellation (1 - t >= 0.63), and a large argument
//                      underflows to t = 0, f = |lambda| (no overflow anywhere; a lambda = inf gives t = 0 as well).
//  |a lambda| <  1/2:  u coth u = sum_n 2^2n B_2n u^2n / (2n)! = 1 + u^2/3 - u^4/45 + ..., 13 terms (the first dropped term is below 4e-21
//                      at u = 1/2), Horner in u^2 by fma, then one division by a.  The exponential form alone loses 1 / (2u) ulps here (70 at 1e-3).
//  u^2 underflows to 0 for tiny u: f = 1 / a exactly, as at 0.
// Error against the exact value: at most 4 ulps (tests/test_softabs_host.py measures it against 60-digit arithmetic).
KD_FN double ksa_f(double lam, double a)
{
    const double u = ksa_abs(a * lam);
    if (u < KSA_SMALL) {
        const double z = u * u;
        double s = -0x1.497d9033a2b5cp-39;
        s = kd_fma(s, z, 0x1.967e1f09c376fp-36);
        s = kd_fma(s, z, -0x1.f57d968caacf1p-33);
        s = kd_fma(s, z, 0x1.355871d652e9ep-29);
        s = kd_fma(s, z, -0x1.7da4e1f79955cp-26);
        s = kd_fma(s, z, 0x1.d6db2c4e09162p-23);
        s = kd_fma(s, z, -0x1.22805d644267fp-19);
        s = kd_fma(s, z, 0x1.66a8f2bf70ebep-16);
        s = kd_fma(s, z, -0x1.bbd779334ef0bp-13);
        s = kd_fma(s, z, 0x1.1566abc011567p-9);
        s = kd_fma(s, z, -0x1.6c16c16c16c17p-6);
        s = kd_fma(s, z, 0x1.5555555555555p-2);
        s = kd_fma(s, z, 1.0);
        return s / a;
    }
    const double t = kd_exp(-2.0 * u);          // (a NaN argument comes back as NaN)
    return ksa_abs(lam) * ((1.0 + t) / (1.0 - t));
}

// Cyclic Jacobi on the leading D x D block of the packed upper triangle A (entry (i, j), i <= j, at ksa_tri(i, j, E)); Q (row-major D x D, column k
// the k-th eigenvector, entry (i, k) at Q[(i * D + k) * qs]: qs = 1 for an array of the caller's, the workgroup's size where the lanes' matrices are
// interleaved in LDS) starts as the identity.  On return the diagonal of A holds the eigenvalues.  Returns the number of sweeps.
// One rotation (p, q), skipped when A_pq is exactly zero:
//     d = A_qq - A_pp, b = 2 A_pq, h = sqrt(d^2 + b^2), t = sign(d) b / (|d| + h)      [= sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = d / b]
//     c = 1 / sqrt(t^2 + 1), s = t c
// which is the textbook rotation with its numerator and denominator multiplied by |b|: two divisions and two square roots where the form in theta takes three and
// two (an f64 division is a dozen dependent instructions on this hardware and a rotation at D = 2 is little else).  |entries| <= 2^500 (T4) keeps d^2 + b^2 finite;
// where b^2 underflows, t = b / (2 |d|) is the rotation to first order in an entry below 1e-154, and d = 0 with it gives the 45 degree rotation (t = +-1).
KD_FN int ksa_jacobi(double* A, double* Q, int qs, int D, int E)
{
KSA_UNROLL
    for (int i = 0; i < D; ++i) {
KSA_UNROLL
        for (int j = 0; j < D; ++j) Q[(i * D + j) * qs] = i == j ? 1.0 : 0.0;
    }
    int sweeps = 0;
    for (;;) {
        double off = 0.0, dg = 0.0;
KSA_UNROLL
        for (int p = 0; p < D; ++p) {
            dg = dg + A[ksa_tri(p, p, E)] * A[ksa_tri(p, p, E)];
KSA_UNROLL
            for (int q = p + 1; q < D; ++q) off = off + A[ksa_tri(p, q, E)] * A[ksa_tri(p, q, E)];
        }
        if (!(off > KSA_TOL2 * dg) || sweeps == KSA_MAX_SWEEPS) break;
        ++sweeps;
KSA_UNROLL
        for (int p = 0; p < D; ++p) {
KSA_UNROLL
            for (int q = p + 1; q < D; ++q) {
                const double apq = A[ksa_tri(p, q, E)];
                if (apq != 0.0) {
                    const double app = A[ksa_tri(p, p, E)], aqq = A[ksa_tri(q, q, E)];
                    const double d = aqq - app, b = apq + apq;
                    const double h = __builtin_sqrt(d * d + b * b);
                    const double den = ksa_abs(d) + h;
                    const double num = d < 0.0 ? -b : b;
                    const double t = den > 0.0 ? num / den : (b < 0.0 ? -1.0 : 1.0);
                    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
                    const double s = t * c;
                    A[ksa_tri(p, p, E)] = app - t * apq;
                    A[ksa_tri(q, q, E)] = aqq + t * apq;
                    A[ksa_tri(p, q, E)] = 0.0;
KSA_UNROLL
                    for (int r = 0; r < D; ++r) {
                        if (r != p && r != q) {
                            const int ip = r < p ? ksa_tri(r, p, E) : ksa_tri(p, r, E), iq = r < q ? ksa_tri(r, q, E) : ksa_tri(q, r, E);
                            const double arp = A[ip], arq = A[iq];
                            A[ip] = c * arp - s * arq;
                            A[iq] = s * arp + c * arq;
                        }
                    }
KSA_UNROLL
                    for (int r = 0; r < D; ++r) {
                        const double vrp = Q[(r * D + p) * qs], vrq = Q[(r * D + q) * qs];
                        Q[(r * D + p) * qs] = c * vrp - s * vrq;
                        Q[(r * D + q) * qs] = s * vrp + c * vrq;
                    }
                }
            }
        }
    }
    return sweeps;
}

// softabs of the leading D x D block of the packed upper triangle gm (stride E: the layout of klara_kernels.h ktri), in place: the block becomes
// the upper triangle of sum_k f(lambda_k) q_k q_k' (k ascending).  Entries outside the block (the padding of D < E) are not touched.  Q, qs: D x D
// doubles of work space for the eigenvectors, as ksa_jacobi takes them.  Returns the sweeps taken, or -1 for a matrix that is not transformed (T4):
// gm[0] is then a NaN.
KD_FN int ksa_softabs_tri(double* gm, int D, int E, double a, double* Q, int qs)
{
    int fin = 1;
KSA_UNROLL
    for (int i = 0; i < D; ++i) {
KSA_UNROLL
        for (int j = i; j < D; ++j) fin = fin && (ksa_abs(gm[ksa_tri(i, j, E)]) <= KSA_BIG);      // (false for a NaN)
    }
    if (!fin) { gm[0] = kd_u2d(0x7ff8000000000000ull); return -1; }
    double w[KSA_MAXD];
    const int sweeps = ksa_jacobi(gm, Q, qs, D, E);
KSA_UNROLL
    for (int k = 0; k < D; ++k) w[k] = ksa_f(gm[ksa_tri(k, k, E)], a);
KSA_UNROLL
    for (int i = 0; i < D; ++i) {
KSA_UNROLL
        for (int j = i; j < D; ++j) {
            double t = 0.0;
KSA_UNROLL
            for (int k = 0; k < D; ++k) t = t + (w[k] * Q[(i * D + k) * qs]) * Q[(j * D + k) * qs];
            gm[ksa_tri(i, j, E)] = t;
        }
    }
    return sweeps;
}
#endif /* KLARA_SOFTABS_H */
