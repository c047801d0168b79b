// klara_zv.hip — the zero-variance control variate kernels (lzv / qzv of zv.jl) for gfx950 and their launchers; see klara_zv.h.
#include "klara_zv.h"
#include <cmath>
#include <mutex>
#include <unordered_map>

#define ZV_TB KLARA_ZV_TB
#define ZV_NT (64 * KLARA_ZV_WAVES)
#define ZV_LDS_DEFAULT_DYNAMIC 65536

typedef double zv_double4 __attribute__((ext_vector_type(4)));

// what the kernels need of KZvGeom
struct KZvDev {
    int D, K, KP, MT, XT, LDW, ntiles, WPC, C, WPA, CA, STR;
};

// ------------------------------------------------------------------------------------------------------------------- staging
// Rows [f | x] of ZV_TB saved steps t0 .. t0 + ZV_TB - 1 of the workgroup's C chains (first one: chain c0 of the handle; ncv of them
// exist) into M[(cc * ZV_TB + t) * stride + col], less meanL[cc * LDW + col] when meanL is given.  Padding columns, steps >= n and
// chains >= ncv are written as zeros, so they add nothing to any product.  Order 2 forms its control variates here, from the step's
// x and z rows staged in `raw` (16 doubles each): they exist in LDS only.
template <int ORDER>
__device__ __forceinline__ void zv_stage(double* __restrict__ M, double* __restrict__ raw, const double* __restrict__ meanL,
                                         const double* __restrict__ hx, const double* __restrict__ hg, long long N, const KZvDev& g, int C,
                                         int stride, long long c0, int ncv, long long t0, long long n)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int D = g.D, K = g.K, KP = g.KP, LDW = g.LDW;
    if (ORDER == 2) {
        for (int idx = tid; idx < C * ZV_TB * 32; idx += nt) {
            const int e = idx & 31, t = (idx >> 5) % ZV_TB, cc = idx / (32 * ZV_TB), d = e & 15;
            double v = 0.0;
            if (d < D && cc < ncv && t0 + t < n) {
                const size_t off = ((size_t)(t0 + t) * (size_t)N + (size_t)(c0 + cc)) * (size_t)D + (size_t)d;
                v = e < 16 ? hx[off] : -0.5 * hg[off];
            }
            raw[idx] = v;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < C * ZV_TB * LDW; idx += nt) {
        const int col = idx % LDW, row = idx / LDW, t = row % ZV_TB, cc = row / ZV_TB;
        double v = 0.0;
        bool ok = cc < ncv && t0 + t < n;
        if (ok) {
            if (ORDER == 1) {
                const int d = col < KP ? col : col - KP;
                ok = d < D;
                if (ok) {
                    const size_t off = ((size_t)(t0 + t) * (size_t)N + (size_t)(c0 + cc)) * (size_t)D + (size_t)d;
                    v = col < KP ? -0.5 * hg[off] : hx[off];
                }
            } else {
                const double* xr = raw + (size_t)row * 32;
                const double* zr = xr + 16;
                if (col >= KP) { ok = col - KP < D; if (ok) v = xr[col - KP]; }
                else if (col < D) v = zr[col];
                else if (col < 2 * D) v = 2.0 * zr[col - D] * xr[col - D] - 1.0;
                else if (col < K) {
                    int p = col - 2 * D, i = 0;
                    while (p >= D - 1 - i) { p -= D - 1 - i; ++i; }
                    const int j = i + 1 + p;
                    v = xr[i] * zr[j] + xr[j] * zr[i];
                } else ok = false;
            }
            if (ok && meanL) v -= meanL[cc * LDW + col];
        }
        M[(size_t)row * stride + col] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------- stage 1
template <int ORDER, int TPW>
__global__ __launch_bounds__(ZV_NT) void k_zv_gram(const double* __restrict__ hx, const double* __restrict__ hg, long long N, long long n,
                                                   long long c0, long long nc, KZvDev g, double* __restrict__ S, double* __restrict__ meanbuf,
                                                   int means_only)
{
    extern __shared__ __attribute__((aligned(16))) double zv_lds[];
    const int C = g.C, LDW = g.LDW;
    double* M = zv_lds;
    double* meanL = M + (size_t)C * ZV_TB * LDW;
    double* raw = meanL + (size_t)C * LDW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const long long cb = (long long)blockIdx.x * C;              // first chain of the workgroup within the chunk
    const int ncv = (int)(nc - cb < C ? nc - cb : C);
    const bool colthread = tid < C * LDW;                        // one thread per (chain, column) for the means
    const int mcc = colthread ? tid / LDW : 0, mcol = colthread ? tid % LDW : 0;

    // pass 1: mean of every column as first sample + sum (value - first sample) / n, summed in step order
    double shift = 0.0, csum = 0.0;
    for (long long t0 = 0; t0 < n; t0 += ZV_TB) {
        zv_stage<ORDER>(M, raw, nullptr, hx, hg, N, g, C, LDW, c0 + cb, ncv, t0, n);
        __syncthreads();
        if (colthread) {
            const double* col = M + (size_t)mcc * ZV_TB * LDW + mcol;
            if (t0 == 0) shift = col[0];
            const int tn = (int)(n - t0 < ZV_TB ? n - t0 : ZV_TB);
            for (int t = 0; t < tn; ++t) csum += col[(size_t)t * LDW] - shift;
        }
        __syncthreads();
    }
    if (colthread) {
        const double m = shift + csum / (double)n;
        meanL[tid] = m;
        if (mcc < ncv) meanbuf[(size_t)(cb + mcc) * LDW + mcol] = m;
    }
    __syncthreads();
    if (means_only) return;

    // pass 2: this wavefront's tiles of Fc' [Fc | Xc]
    const int cc = w / g.WPC, wl = w % g.WPC;
    const double* Mc = M + (size_t)(cc < C ? cc : 0) * ZV_TB * LDW;
    int aoff[TPW], boff[TPW];
    bool on[TPW];
    zv_double4 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        int id = wl + j * g.WPC;
        on[j] = cc < C && id < g.ntiles;
        int rt = 0;
        if (on[j]) while (id >= g.MT + g.XT - rt) { id -= g.MT + g.XT - rt; ++rt; }
        aoff[j] = on[j] ? 16 * rt + l15 : 0;                     // row tile rt of Fc'
        boff[j] = on[j] ? 16 * (rt + id) + l15 : 0;              // column tile rt + id of [Fc | Xc]  (KP = 16 MT: the x tiles follow)
        acc[j] = zv_double4{0.0, 0.0, 0.0, 0.0};
    }
    for (long long t0 = 0; t0 < n; t0 += ZV_TB) {
        zv_stage<ORDER>(M, raw, meanL, hx, hg, N, g, C, LDW, c0 + cb, ncv, t0, n);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < ZV_TB / 4; ++kk) {
            const double* row = Mc + (size_t)(4 * kk + q) * LDW;
#pragma unroll
            for (int j = 0; j < TPW; ++j)
                if (on[j]) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[aoff[j]], row[boff[j]], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
    if (cc < ncv) {
        double* Sc = S + (size_t)(cb + cc) * (size_t)g.KP * LDW;
#pragma unroll
        for (int j = 0; j < TPW; ++j)
            if (on[j]) {
                const int r0 = aoff[j] - l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) Sc[(size_t)(r0 + q + 4 * r) * LDW + boff[j]] = acc[j][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------- stage 2
// S: per chain KP x LDW (row-major) with the upper triangle tiles of S_ff and S_fx filled.  coef: per chain K x D.
__global__ void k_zv_solve(const double* __restrict__ S, size_t s_elems, int K, int KP, int LDW, int D, double* __restrict__ coef,
                           int* __restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double zv_lds[];
    double* L = zv_lds;                                  // lower triangle, packed by rows: L[r][c] at r (r + 1) / 2 + c
    double* B = L + (size_t)K * (K + 1) / 2;             // K x 16 block of right-hand sides
    const int tid = threadIdx.x, nt = blockDim.x;
    const double* Sc = S + (size_t)blockIdx.x * s_elems;
    double* cf = coef + (size_t)blockIdx.x * (size_t)K * D;
    for (int p = tid; p < K * K; p += nt) {
        const int r = p / K, c = p % K;
        if (c <= r) L[r * (r + 1) / 2 + c] = Sc[(size_t)c * LDW + r];
    }
    __syncthreads();
    const int tc = tid & 15, tr = tid >> 4, G = nt >> 4;
    bool bad = false;
    for (int j = 0; j < K; ++j) {
        const double d = L[j * (j + 1) / 2 + j];
        if (!(d > 0.0) || !(d < INFINITY)) { bad = true; break; }      // (the same value in every thread: a uniform exit)
        const double s = sqrt(d);
        __syncthreads();
        for (int r = j + tid; r < K; r += nt) L[r * (r + 1) / 2 + j] = r == j ? s : L[r * (r + 1) / 2 + j] / s;
        __syncthreads();
        for (int r = j + 1 + tr; r < K; r += G) {
            const double lrj = L[r * (r + 1) / 2 + j];
            for (int c = j + 1 + tc; c <= r; c += 16) L[r * (r + 1) / 2 + c] -= lrj * L[c * (c + 1) / 2 + j];
        }
        __syncthreads();
    }
    if (bad) {
        for (int p = tid; p < K * D; p += nt) cf[p] = NAN;
        if (tid == 0) info[blockIdx.x] = 1;
        return;
    }
    if (tid == 0) info[blockIdx.x] = 0;
    for (int cb0 = 0; cb0 < D; cb0 += 16) {
        for (int p = tid; p < K * 16; p += nt) B[p] = Sc[(size_t)(p >> 4) * LDW + KP + cb0 + (p & 15)];
        __syncthreads();
        for (int j = 0; j < K; ++j) {                                   // L Y = B, column oriented; row j is final when step j reads it
            const double y = B[j * 16 + tc] / L[j * (j + 1) / 2 + j];
            for (int r = j + 1 + tr; r < K; r += G) B[r * 16 + tc] -= L[r * (r + 1) / 2 + j] * y;
            __syncthreads();
        }
        for (int p = tid; p < K * 16; p += nt) { const int k = p >> 4; B[p] /= L[k * (k + 1) / 2 + k]; }
        __syncthreads();
        for (int j = K - 1; j >= 0; --j) {                              // L' A = Y
            const double a = B[j * 16 + tc] / L[j * (j + 1) / 2 + j];
            for (int r = tr; r < j; r += G) B[r * 16 + tc] -= L[j * (j + 1) / 2 + r] * a;
            __syncthreads();
        }
        for (int p = tid; p < K * 16; p += nt) {
            const int k = p >> 4, i = cb0 + (p & 15);
            if (i < D) cf[(size_t)k * D + i] = -(B[p] / L[k * (k + 1) / 2 + k]);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------- stage 3
template <int ORDER, int NKK>
__global__ __launch_bounds__(ZV_NT) void k_zv_apply(const double* __restrict__ hx, const double* __restrict__ hg, long long N, long long n,
                                                    long long c0, long long nc, KZvDev g, const double* __restrict__ meanbuf,
                                                    const double* __restrict__ coef, size_t coef_stride, double* __restrict__ zv_mean,
                                                    double* __restrict__ zv_var, double* __restrict__ series)
{
    extern __shared__ __attribute__((aligned(16))) double zv_lds[];
    const int C = g.CA, LDW = g.LDW, STR = g.STR, D = g.D, K = g.K, KP = g.KP;
    double* M = zv_lds;
    double* meanL = M + (size_t)C * ZV_TB * STR;
    double* red = meanL + (size_t)C * LDW;               // 8 wavefronts x 64 lanes x {sum, sum of squares}
    double* raw = red + 2 * ZV_NT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const long long cb = (long long)blockIdx.x * C;
    const int ncv = (int)(nc - cb < C ? nc - cb : C);
    for (int p = tid; p < C * LDW; p += ZV_NT) meanL[p] = p / LDW < ncv ? meanbuf[(size_t)cb * LDW + p] : 0.0;
    __syncthreads();

    const int cc = w / g.WPA, ct = w % g.WPA;
    const bool active = cc < ncv && ct < g.XT;           // (ncv <= C)
    const int i = 16 * ct + l15;                         // the lane's dimension
    const bool idim = active && i < D;
    const double* cf = coef + (size_t)(cb + (active ? cc : 0)) * coef_stride;
    const int nkk = KP / 4;
    double bfrag[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        const int k = 4 * kk + q;
        bfrag[kk] = (idim && k < K) ? cf[(size_t)k * D + i] : 0.0;
    }
    double base = 0.0;                                   // mean(x_i) + mean(f) A[:, i]
    if (idim) {
        base = meanL[cc * LDW + KP + i];
        for (int k = 0; k < K; ++k) base += meanL[cc * LDW + k] * cf[(size_t)k * D + i];
    }
    const double* Mc = M + (size_t)(active ? cc : 0) * ZV_TB * STR;
    double sum = 0.0, sumsq = 0.0;
    for (long long t0 = 0; t0 < n; t0 += ZV_TB) {
        zv_stage<ORDER>(M, raw, meanL, hx, hg, N, g, C, STR, c0 + cb, ncv, t0, n);
        __syncthreads();
        if (active) {
            zv_double4 acc = zv_double4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk)
                if (kk < nkk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Mc[(size_t)l15 * STR + 4 * kk + q], bfrag[kk], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = q + 4 * r;
                const double v = acc[r] + Mc[(size_t)t * STR + KP + i];      // Xc + Fc A  (zero rows beyond n)
                sum += v; sumsq += v * v;
                if (series && i < D && t0 + t < n) series[(size_t)(t0 + t) * D + i] = base + v;
            }
        }
        __syncthreads();
    }
    red[2 * tid] = sum; red[2 * tid + 1] = sumsq;
    __syncthreads();
    if (idim && q == 0) {
        const double* rw = red + 2 * (64 * w + l15);
        const double s = ((rw[0] + rw[32]) + rw[64]) + rw[96], ss = ((rw[1] + rw[33]) + rw[65]) + rw[97];
        const size_t o = (size_t)(cb + cc) * D + i;
        if (zv_mean) zv_mean[o] = base + s / (double)n;
        if (zv_var) {
            double v = (ss - s * s / (double)n) / (double)(n - 1);
            if (v < 0.0) v = 0.0;                        // (rounding of a series that is constant to the last bit; NaN stays NaN)
            zv_var[o] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- pooled
// Chan's update of (count, mean, centred cross-products) with the nc chains of a chunk in ascending order, one thread per element of
// the KP x LDW matrix (tiles below the diagonal of S_ff are not kept).  Each thread carries the two means its element needs; the
// pooled means are read from pmean_in and written to pmean_out (two buffers, so no thread reads what another has just written).
__global__ __launch_bounds__(256) void k_zv_merge(const double* __restrict__ S, const double* __restrict__ meanbuf, long long nc, int KP, int LDW,
                                                  double n_per, double count0, const double* __restrict__ pmean_in,
                                                  double* __restrict__ pmean_out, double* __restrict__ pS)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= KP * LDW) return;
    const int r = e / LDW, col = e % LDW;
    if (col / 16 < r / 16) return;
    const size_t se = (size_t)KP * LDW;
    double mr = pmean_in[r], mc = pmean_in[col], s = count0 > 0.0 ? pS[e] : 0.0, na = count0;
    for (long long c = 0; c < nc; ++c) {
        const double sc = S[(size_t)c * se + e], a = meanbuf[(size_t)c * LDW + r], b = meanbuf[(size_t)c * LDW + col];
        const double dr = a - mr, dc = b - mc, tot = na + n_per;
        s = s + sc + dr * dc * (na * n_per / tot);
        mr += dr * (n_per / tot);
        mc += dc * (n_per / tot);
        na = tot;
    }
    pS[e] = s;
    if (r == 0) pmean_out[col] = mc;
}

// ------------------------------------------------------------------------------------------------------------------- host
bool klara_zv_plan(int order, int D, KZvGeom* g)
{
    if ((order != 1 && order != 2) || D < 1) return false;
    const long long K = order == 1 ? D : (long long)D * (D + 3) / 2;
    if (K > 128) return false;
    g->order = order; g->D = D; g->K = (int)K;
    g->MT = (g->K + 15) / 16; g->XT = (D + 15) / 16; g->KP = 16 * g->MT; g->LDW = 16 * (g->MT + g->XT);
    g->ntiles = g->MT * (g->MT + 1) / 2 + g->MT * g->XT;
    g->WPC = 1;
    while ((g->ntiles + g->WPC - 1) / g->WPC > KLARA_ZV_MAX_TPW) g->WPC *= 2;      // <= 8: 100 tiles at most
    g->C = KLARA_ZV_WAVES / g->WPC;
    while (g->C > 1 && g->C * g->LDW > ZV_NT) g->C /= 2;                            // one thread per (chain, column) in the mean pass
    const int need = (g->ntiles + g->WPC - 1) / g->WPC;
    g->TPW = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : KLARA_ZV_MAX_TPW;
    g->WPA = 1;
    while (g->WPA < g->XT) g->WPA *= 2;
    g->CA = KLARA_ZV_WAVES / g->WPA;
    while (g->CA > 1 && g->CA * g->LDW > ZV_NT) g->CA /= 2;
    g->NKK = g->MT <= 1 ? 4 : g->MT <= 2 ? 8 : g->MT <= 4 ? 16 : 32;
    g->STR = g->LDW + 2;                                                           // rows of the apply pass are read down a column
    const size_t raw = order == 2 ? (size_t)ZV_TB * 32 : 0;
    g->gram_lds = ((size_t)g->C * ZV_TB * g->LDW + (size_t)g->C * g->LDW + g->C * raw) * sizeof(double);
    g->apply_lds = ((size_t)g->CA * ZV_TB * g->STR + (size_t)g->CA * g->LDW + 2 * ZV_NT + g->CA * raw) * sizeof(double);
    g->solve_threads = g->K <= 32 ? 64 : 256;
    g->solve_lds = ((size_t)g->K * (g->K + 1) / 2 + (size_t)g->K * 16) * sizeof(double);
    g->s_elems = (size_t)g->KP * g->LDW;
    g->chain_bytes = (g->s_elems + g->LDW + (size_t)g->K * D + 2 * (size_t)D) * sizeof(double) + sizeof(int);
    return true;
}

long long klara_zv_chunk(const KZvGeom& g, long long nchains)
{
    // the pooled triple and one series are small beside it: 2 MiB are set aside for them
    long long c = (long long)((KLARA_ZV_WORKSPACE_BYTES - ((size_t)2 << 20)) / g.chain_bytes);
    c -= c % KLARA_ZV_WAVES;                                                       // whole workgroups
    if (c < KLARA_ZV_WAVES) c = KLARA_ZV_WAVES;
    return c < nchains ? c : nchains;
}

static KZvDev dev_geom(const KZvGeom& g)
{
    KZvDev d;
    d.D = g.D; d.K = g.K; d.KP = g.KP; d.MT = g.MT; d.XT = g.XT; d.LDW = g.LDW; d.ntiles = g.ntiles; d.WPC = g.WPC; d.C = g.C;
    d.WPA = g.WPA; d.CA = g.CA; d.STR = g.STR;
    return d;
}

// a kernel's dynamic LDS limit is raised once per process and size, not at every launch (the largest size asked for so far is kept)
template <class Kern>
static hipError_t raise_lds(Kern k, size_t lds)
{
    if (lds <= ZV_LDS_DEFAULT_DYNAMIC) return hipSuccess;
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> raised;
    std::lock_guard<std::mutex> g(mu);
    size_t& have = raised[(const void*)k];
    if (have >= lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) have = lds;
    return e;
}

template <int ORDER, int TPW>
static hipError_t go_gram(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                          double* S, double* meanbuf, int means_only, hipStream_t st)
{
    hipError_t e = raise_lds(k_zv_gram<ORDER, TPW>, g.gram_lds);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((nc + g.C - 1) / g.C);
    hipLaunchKernelGGL((k_zv_gram<ORDER, TPW>), dim3(grid), dim3(ZV_NT), g.gram_lds, st, hist, hist_g, N, n, c0, nc, dev_geom(g), S, meanbuf,
                       means_only);
    return hipGetLastError();
}

template <int ORDER>
static hipError_t go_gram_o(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                            double* S, double* meanbuf, int means_only, hipStream_t st)
{
    switch (g.TPW) {
    case 1: return go_gram<ORDER, 1>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
    case 2: return go_gram<ORDER, 2>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
    case 4: return go_gram<ORDER, 4>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
    case 8: return go_gram<ORDER, 8>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
    case KLARA_ZV_MAX_TPW: return go_gram<ORDER, KLARA_ZV_MAX_TPW>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t klara_zv_launch_gram(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                                double* S, double* meanbuf, int means_only, hipStream_t st)
{
    if (nc <= 0 || n < 1 || c0 < 0 || c0 + nc > N) return hipErrorInvalidValue;
    return g.order == 1 ? go_gram_o<1>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st)
                        : go_gram_o<2>(g, hist, hist_g, N, n, c0, nc, S, meanbuf, means_only, st);
}

hipError_t klara_zv_launch_solve(const KZvGeom& g, const double* S, long long nchains, double* coef, int* info, hipStream_t st)
{
    if (nchains <= 0) return hipErrorInvalidValue;
    hipError_t e = raise_lds(k_zv_solve, g.solve_lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_zv_solve, dim3((unsigned)nchains), dim3(g.solve_threads), g.solve_lds, st, S, g.s_elems, g.K, g.KP, g.LDW, g.D, coef, info);
    return hipGetLastError();
}

template <int ORDER, int NKK>
static hipError_t go_apply(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                           const double* meanbuf, const double* coef, size_t coef_stride, double* zv_mean, double* zv_var, double* series,
                           hipStream_t st)
{
    hipError_t e = raise_lds(k_zv_apply<ORDER, NKK>, g.apply_lds);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((nc + g.CA - 1) / g.CA);
    hipLaunchKernelGGL((k_zv_apply<ORDER, NKK>), dim3(grid), dim3(ZV_NT), g.apply_lds, st, hist, hist_g, N, n, c0, nc, dev_geom(g), meanbuf, coef,
                       coef_stride, zv_mean, zv_var, series);
    return hipGetLastError();
}

hipError_t klara_zv_launch_apply(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                                 const double* meanbuf, const double* coef, size_t coef_stride, double* zv_mean, double* zv_var, double* series,
                                 hipStream_t st)
{
    if (nc <= 0 || n < 2 || c0 < 0 || c0 + nc > N || (series && nc != 1)) return hipErrorInvalidValue;
#define ZV_APPLY(O, NK) return go_apply<O, NK>(g, hist, hist_g, N, n, c0, nc, meanbuf, coef, coef_stride, zv_mean, zv_var, series, st)
    if (g.order == 1) {
        switch (g.NKK) { case 4: ZV_APPLY(1, 4); case 8: ZV_APPLY(1, 8); case 16: ZV_APPLY(1, 16); case 32: ZV_APPLY(1, 32); }
    } else {
        switch (g.NKK) { case 4: ZV_APPLY(2, 4); case 8: ZV_APPLY(2, 8); case 16: ZV_APPLY(2, 16); case 32: ZV_APPLY(2, 32); }
    }
#undef ZV_APPLY
    return hipErrorInvalidValue;
}

hipError_t klara_zv_launch_merge(const KZvGeom& g, const double* S, const double* meanbuf, long long nc, double n_per, double count0,
                                 const double* pmean_in, double* pmean_out, double* pS, hipStream_t st)
{
    if (nc <= 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((g.s_elems + 255) / 256);
    hipLaunchKernelGGL(k_zv_merge, dim3(grid), dim3(256), 0, st, S, meanbuf, nc, g.KP, g.LDW, n_per, count0, pmean_in, pmean_out, pS);
    return hipGetLastError();
}
