// klara_cov.hip — the pooled posterior covariance kernels for gfx950 and their launchers; see klara_cov.h.
#include "klara_cov.h"
#include "../../include/klara_hip.h"

#define COV_KB KLARA_COV_KB
#define COV_NT (64 * KLARA_COV_WAVES)

typedef double cov_double4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------------- geometry
long long klara_cov_slab(long long N, int D)
{
    const long long MT = (D + 15) / 16, ntiles = MT * (MT + 1) / 2;
    const size_t per = (size_t)(ntiles * 256 + 16 * MT) * sizeof(double);
    long long ch = KLARA_COV_SLAB_MIN;
    while ((size_t)((N + ch - 1) / ch) * per > KLARA_COV_WORKSPACE_BYTES) ch *= 2;
    return ch;
}

bool klara_cov_plan(long long N, int D, KCovGeom* g)
{
    if (N <= 0 || D < 1 || D > KLARA_COV_MAX_DIMS) return false;
    g->N = N; g->D = D; g->MT = (D + 15) / 16; g->DP = 16 * g->MT; g->ntiles = g->MT * (g->MT + 1) / 2;
    g->CH = klara_cov_slab(N, D);
    if (g->CH >= (1ll << 24)) return false;                      // (the kernel counts a launch's padded samples, 32 (CH + 3) at most, in 32 bits)
    g->nslabs = (N + g->CH - 1) / g->CH;
    const int per_group = KLARA_COV_WAVES * KLARA_COV_MAX_TPW;
    g->NG = (g->ntiles + per_group - 1) / per_group;
    g->TPW = (g->ntiles + KLARA_COV_WAVES * g->NG - 1) / (KLARA_COV_WAVES * g->NG);
    g->slab_elems = (size_t)g->ntiles * 256;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- update
template <int TPW>
__global__ __launch_bounds__(COV_NT) void k_cov_update(const double* __restrict__ hist, long long N, int D, int MT, int ntiles, int CH,
                                                       long long col0, int m, const double* __restrict__ pivot, double* __restrict__ S,
                                                       double* __restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) double cov_lds[];
    const int DP = 16 * MT;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long slab = blockIdx.x, c_lo = slab * CH;
    const int nc = (int)(N - c_lo < CH ? N - c_lo : CH), ncp = (nc + 3) & ~3;
    const unsigned total = (unsigned)m * (unsigned)ncp;          // the launch's samples of this slab, every saved step padded to 4 chains
    double* Ss = S + (size_t)slab * (size_t)ntiles * 256;

    // this wavefront's run of TPW consecutive upper tiles (I, J >= I), numbered row by row
    int aI[TPW], bJ[TPW];
    bool on[TPW], diag[TPW], newa[TPW];
    cov_double4 acc[TPW];
    int prevI = -1;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int id = ((int)blockIdx.y * KLARA_COV_WAVES + w) * TPW + j;
        on[j] = id < ntiles;
        int I = 0, rem = on[j] ? id : 0;
        while (rem >= MT - I) { rem -= MT - I; ++I; }
        aI[j] = 16 * I; bJ[j] = 16 * (I + rem);
        diag[j] = rem == 0;
        newa[j] = on[j] && I != prevI;
        if (on[j]) prevI = I;
        acc[j] = cov_double4{0.0, 0.0, 0.0, 0.0};
        if (on[j]) {
            const double* p = Ss + (size_t)id * 256 + lane;
            acc[j] = cov_double4{p[0], p[64], p[128], p[192]};
        }
    }
    // the pivot of the columns this lane stages: lane, lane + 64, ...
    double pv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { const int col = lane + 64 * c; pv[c] = col < D ? pivot[col] : 0.0; }
    const bool sums = blockIdx.y == 0 && tid < D;                // T_s[tid]: tile group 0 only
    double tsum = sums ? T[(size_t)slab * DP + tid] : 0.0;

    // the next KLARA_COV_KB samples travel in registers while the matrix cores work on the current ones: wavefront w takes the rows w, w + 4, w + 8, w + 12
    double nx[COV_KB / KLARA_COV_WAVES][4];
    bool nv[COV_KB / KLARA_COV_WAVES];
    const auto fetch = [&](unsigned r0) {
#pragma unroll
        for (int rr = 0; rr < COV_KB / KLARA_COV_WAVES; ++rr) {
            const unsigned r = r0 + (unsigned)(w + KLARA_COV_WAVES * rr), t = r / (unsigned)ncp, cc = r - t * (unsigned)ncp;
            nv[rr] = r < total && (int)cc < nc;
            const double* x = hist + ((size_t)(col0 + t) * (size_t)N + (size_t)(c_lo + cc)) * (size_t)D;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = lane + 64 * c;
                nx[rr][c] = (nv[rr] && col < D) ? x[col] : 0.0;
            }
        }
    };
    fetch(0);
    for (unsigned r0 = 0; r0 < total; r0 += COV_KB) {
        // stage z = x - pivot of the samples r0 .. r0 + COV_KB - 1 (padding samples and columns: zeros)
#pragma unroll
        for (int rr = 0; rr < COV_KB / KLARA_COV_WAVES; ++rr) {
            const int row = w + KLARA_COV_WAVES * rr;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = lane + 64 * c;
                if (col < DP) cov_lds[row * DP + col] = (nv[rr] && col < D) ? nx[rr][c] - pv[c] : 0.0;
            }
        }
        __syncthreads();
        if (r0 + COV_KB < total) fetch(r0 + COV_KB);
        if (sums) {
#pragma unroll
            for (int row = 0; row < COV_KB; ++row) tsum = tsum + cov_lds[row * DP + tid];
        }
#pragma unroll
        for (int kk = 0; kk < COV_KB / 4; ++kk) {
            const double* row = cov_lds + (4 * kk + q) * DP + l15;
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                if (on[j]) {
                    if (newa[j]) a = row[aI[j]];
                    if (diag[j]) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc[j], 0, 0, 0);
                    else acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, row[bJ[j]], acc[j], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j)
        if (on[j]) {
            const int id = ((int)blockIdx.y * KLARA_COV_WAVES + w) * TPW + j;
            double* p = Ss + (size_t)id * 256 + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) p[64 * r] = acc[j][r];
        }
    if (sums) T[(size_t)slab * DP + tid] = tsum;
}

template <int TPW>
static hipError_t cov_update_t(const KCovGeom& g, const double* hist, long long col0, int m, const double* pivot, double* S, double* T, hipStream_t st)
{
    const size_t lds = (size_t)COV_KB * g.DP * sizeof(double);
    hipLaunchKernelGGL((k_cov_update<TPW>), dim3((unsigned)g.nslabs, (unsigned)g.NG), dim3(COV_NT), lds, st, hist, g.N, g.D, g.MT, g.ntiles, (int)g.CH,
                       col0, m, pivot, S, T);
    return hipGetLastError();
}

hipError_t klara_cov_launch_update(const KCovGeom& g, const double* hist, long long col0, long long m, const double* pivot, double* S, double* T,
                                   hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (long long done = 0; done < m && e == hipSuccess; done += KLARA_COV_MAX_COLS) {
        const int mm = (int)(m - done < KLARA_COV_MAX_COLS ? m - done : KLARA_COV_MAX_COLS);
        const long long c0 = col0 + done;
        switch (g.TPW) {
#define COV_CASE(n) case n: e = cov_update_t<n>(g, hist, c0, mm, pivot, S, T, st); break;
        COV_CASE(1) COV_CASE(2) COV_CASE(3) COV_CASE(4) COV_CASE(5) COV_CASE(6) COV_CASE(7) COV_CASE(8) COV_CASE(9) COV_CASE(10) COV_CASE(11)
        COV_CASE(12) COV_CASE(13)
#undef COV_CASE
        default: e = hipErrorInvalidValue;
        }
    }
    return e;
}

// ------------------------------------------------------------------------------------------------------------------- finalize
__global__ __launch_bounds__(256) void k_cov_finalize(const double* __restrict__ S, const double* __restrict__ T, const double* __restrict__ pivot,
                                                      long long nslabs, int D, int MT, int ntiles, double n, double* __restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx - i * D;
    if (j < i) return;
    const int DP = 16 * MT, I = i >> 4, J = j >> 4, ii = i & 15, jj = j & 15;
    const int tile = I * MT - I * (I - 1) / 2 + (J - I);
    const size_t off = (size_t)tile * 256 + (size_t)(ii >> 2) * 64 + (size_t)(ii & 3) * 16 + jj;      // row (l >> 4) + 4 r, column l & 15 of the tile
    double s = 0.0, ti = 0.0, tj = 0.0;
    for (long long sl = 0; sl < nslabs; ++sl) {
        s = s + S[(size_t)sl * (size_t)ntiles * 256 + off];
        ti = ti + T[(size_t)sl * DP + i];
        tj = tj + T[(size_t)sl * DP + j];
    }
    // T_i T_j / n = qh + ql: the product's and the division's rounding errors carried
    const double p = ti * tj, pe = __builtin_fma(ti, tj, -p);
    const double qh = p / n, r = __builtin_fma(-qh, n, p);
    const double ql = (r + pe) / n;
    double v = (s - qh) - ql;
    double* mean = out;
    double* M = out + D;
    if (i == j) {
        if (v < 0.0) v = 0.0;
        mean[i] = pivot[i] + ti / n;
    }
    M[(size_t)i * D + j] = v;
    M[(size_t)j * D + i] = v;
}

hipError_t klara_cov_launch_finalize(const KCovGeom& g, const double* S, const double* T, const double* pivot, double n, double* out, hipStream_t st)
{
    const int nn = g.D * g.D;
    hipLaunchKernelGGL(k_cov_finalize, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, S, T, pivot, g.nslabs, g.D, g.MT, g.ntiles, n, out);
    return hipGetLastError();
}
