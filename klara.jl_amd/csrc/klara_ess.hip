// klara_ess.hip — the pooled effective sample size's kernels (klara_ess.h): every unit's lagged sums c_u(k) from the streamed autocovariance state, summed
// over the units in two stages of fixed shape — no floating-point atomics — and the units' (mu, c(0)) through R-hat's own reduction (klara_rhat.hip).
#include "klara_handle.h"
#include "klara_rhat.h"
#include "klara_ess.h"

struct EssSrc {
    const double *S[2], *head[2], *tail[2], *total[2];
    int per;                                                                // 1: unit-series e is series e of state 0; 2: unit 2 c + half is chain c of state `half`
};

// One unit-series' lags k0 .. k0 + nl - 1 into the lane's accumulators.  FULL: all 32 of the block — no branch between the lags, so that their 96 loads
// can be in flight together; otherwise the last, partial block of the window, lag by lag.
template <bool FULL>
__device__ __forceinline__ void ess_lags(double (&acc)[32], const double* __restrict__ S, const double* __restrict__ head, const double* __restrict__ tail,
                                         long long nd, int nl, bool first, double tot, double mean, double pivot, double& hs, double& ts, double& nk,
                                         double* __restrict__ umu, double* __restrict__ uc0)
{
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        if (FULL || r < nl) {
            const double c = (*S - mean * ((tot - ts) + (tot - hs))) + (nk * mean) * mean;
            nk = nk - 1.0;
            acc[r] = acc[r] + c;
            if (r == 0 && first) { *umu = pivot + mean; *uc0 = c; }
            hs = hs + (*head - pivot);
            ts = ts + *tail;
            S += nd; head += nd; tail += nd;
        }
    }
}

// Stage 1 (the hot path: S, head and tail are read once, coalesced — consecutive lanes, consecutive series).  See klara_ess.h for the order of operations.
// ckpt: hs[E] | ts[E], touched only when L >= 32; every unit-series is read and written by one lane only.
__global__ __launch_bounds__(256) void k_ess_stage1(EssSrc src, long long n, int L, long long nd, int D, long long E, long long V,
                                                    double* __restrict__ ckpt, double* __restrict__ partial, double* __restrict__ umu,
                                                    double* __restrict__ uc0)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= V) return;
    const double dn = (double)n;
    for (int k0 = 0; k0 <= L; k0 += 32) {
        const int nl = L + 1 - k0 < 32 ? L + 1 - k0 : 32;                  // this block's lags
        double acc[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) acc[r] = 0.0;
        for (long long e = g; e < E; e += V) {
            long long i = e;
            int s = 0;
            if (src.per == 2) {
                const long long u = e / D, j = e - u * D;
                s = (int)(u & 1); i = (u >> 1) * D + j;
            }
            const double pivot = src.head[s][i], tot = src.total[s][i], mean = tot / dn;
            const long long at = (long long)k0 * nd + i;                   // (the three rows advance by nd per lag: one running offset, not 32 products)
            const double* __restrict__ S = src.S[s] + at;
            const double* __restrict__ head = src.head[s] + at;
            const double* __restrict__ tail = src.tail[s] + at;
            double hs = 0.0, ts = 0.0, nk = (double)(n - k0);              // nk = (double)(n - k), stepped down by 1.0 (exact) per lag ...
            asm volatile("" : "+v"(nk));                                    // ... per unit-series: 32 converted constants held across the loop would cost 64 registers
            int nle = nl;
            asm volatile("" : "+s"(nle));                                   // (likewise: 32 lane masks of r < nl held across the loop would cost 64 scalar registers)
            if (k0 > 0) { hs = ckpt[e]; ts = ckpt[E + e]; }
            if (nle == 32) ess_lags<true>(acc, S, head, tail, nd, nle, k0 == 0, tot, mean, pivot, hs, ts, nk, umu + e, uc0 + e);
            else ess_lags<false>(acc, S, head, tail, nd, nle, k0 == 0, tot, mean, pivot, hs, ts, nk, umu + e, uc0 + e);
            if (k0 + 32 <= L) { ckpt[e] = hs; ckpt[E + e] = ts; }
        }
        double* __restrict__ out = partial + (long long)k0 * V + g;
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            if (r < nl) *out = acc[r];
            out += V;
        }
    }
}

// Stage 2, workgroup (k, jt): lag k, for D > 256 the dimensions 256 jt ...  csum[j (L + 1) + k]
__global__ __launch_bounds__(256) void k_ess_stage2(const double* __restrict__ partial, long long V, int D, int L, double* __restrict__ csum)
{
    __shared__ double lane[256];
    const int k = blockIdx.x, t = threadIdx.x;
    const double* __restrict__ row = partial + (long long)k * V;
    if (D > 256) {
        const int j = blockIdx.y * 256 + t;
        if (j >= D) return;
        double a = 0.0;
        for (long long g = j; g < V; g += D) a = a + row[g];
        csum[(long long)j * (L + 1) + k] = a;
        return;
    }
    const int V2 = D * (256 / D);
    double a = 0.0;
    if (t < V2)
        for (long long g = t; g < V; g += V2) a = a + row[g];
    lane[t] = a;
    __syncthreads();
    if (t < D) {
        double s = 0.0;
        for (int q = t; q < V2; q += D) s = s + lane[q];
        csum[(long long)t * (L + 1) + k] = s;
    }
}

size_t klara_ess_ws_elems(long long E, int D, int W)
{
    return (size_t)4 * (size_t)E + (size_t)W * (size_t)klara_ess_lanes(E, D) + klara_rhat_partial_elems(D);
}

hipError_t ess_reduce_async(hipStream_t stream, const EssState* st, int per, long long n, int W, long long nd, int D, double* ws, double* meanb, double* x)
{
    if (n < 1 || W < 1 || (per != 1 && per != 2)) return hipErrorInvalidValue;
    const long long E = (long long)per * nd, V = klara_ess_lanes(E, D);
    const int L = (int)((long long)(W - 1) < n - 1 ? (long long)(W - 1) : n - 1);
    double *umu = ws, *uc0 = ws + E, *ckpt = ws + 2 * E, *partial = ws + 4 * E, *rpartial = partial + (size_t)W * (size_t)V;
    EssSrc src;
    for (int s = 0; s < 2; ++s) {
        const EssState& a = st[s < per ? s : 0];
        src.S[s] = a.S; src.head[s] = a.head; src.tail[s] = a.tail; src.total[s] = a.total;
    }
    src.per = per;
    hipLaunchKernelGGL(k_ess_stage1, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, src, n, L, nd, D, E, V, ckpt, partial, umu, uc0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ess_stage2, dim3((unsigned)(L + 1), (unsigned)(D > 256 ? (D + 255) / 256 : 1)), dim3(256), 0, stream, partial, V, D, L, x + D);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rhat_units_async(stream, umu, uc0, E / D, D, rpartial, meanb, x);
}

hipError_t ess_alloc_states(DeviceArrays& mem, int per, int W, long long nd, EssState* st)
{
    const size_t ws = (size_t)W * (size_t)nd;
    hipError_t e = hipSuccess;
    for (int s = 0; s < per && e == hipSuccess; ++s) {
        st[s] = EssState{ nullptr, nullptr, nullptr, nullptr, nullptr };
        e = mem.alloc(&st[s].S, ws);
        if (e == hipSuccess) e = mem.alloc(&st[s].head, ws);
        if (e == hipSuccess) e = mem.alloc(&st[s].tail, ws);
        if (e == hipSuccess) e = mem.alloc(&st[s].total, (size_t)nd);
        if (e == hipSuccess && W > 32) e = mem.alloc(&st[s].near, (size_t)32 * (size_t)nd);
    }
    return e;
}

hipError_t ess_feed_history_async(hipStream_t stream, const double* hist, long long ncols, long long nd, int W, int per, const EssState* st)
{
    const size_t ws = (size_t)W * (size_t)nd * sizeof(double);
    const long long len = per == 2 ? ncols / 2 : ncols;
    hipError_t e = hipSuccess;
    for (int s = 0; s < per && e == hipSuccess; ++s) {
        const long long first = s == 0 ? 0 : ncols - len;
        e = hipMemsetAsync(st[s].S, 0, ws, stream);                         // (what klara_set_state / klara_reset leave)
        if (e == hipSuccess) e = hipMemsetAsync(st[s].head, 0, ws, stream);
        if (e == hipSuccess) e = hipMemsetAsync(st[s].tail, 0, ws, stream);
        if (e == hipSuccess) e = hipMemsetAsync(st[s].total, 0, (size_t)nd * sizeof(double), stream);
        for (long long done = 0; done < len && e == hipSuccess; done += KLARA_ESS_FEED_COLS) {
            const long long m = len - done < KLARA_ESS_FEED_COLS ? len - done : KLARA_ESS_FEED_COLS;
            e = launch_acov_update(stream, hist, st[s].S, st[s].head, st[s].tail, st[s].near, st[s].total, done, W, nd, first + done, m);
        }
    }
    return e;
}
