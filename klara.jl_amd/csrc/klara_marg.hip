// klara_marg.hip — the pooled marginal histogram kernel for gfx950, its launcher, the host-only quantile call and the self test of the ranks' agreement step; see klara_marg.h.
#include "klara_marg.h"
#include "klara_marg_host.h"
#include "../../include/klara_hip.h"
#include <vector>

// ------------------------------------------------------------------------------------------------------------------- geometry
bool klara_marg_plan(long long N, int D, long long nbins, KMargGeom* g)
{
    if (N <= 0 || D < 1 || D > 1024 || nbins < 1 || nbins > KLARA_MARG_MAX_BINS) return false;
    g->N = N; g->D = D; g->nbins = (int)nbins;
    g->stride = (int)(nbins + 2) | 1;
    int db = KLARA_MARG_LDS_BYTES / (4 * g->stride);
    if (db > KLARA_MARG_MAX_DB) db = KLARA_MARG_MAX_DB;
    if (db > D) db = D;
    g->DB = db; g->NDB = (D + db - 1) / db;
    g->CH = (long long)KLARA_MARG_SLAB_UNIT * ((nbins + 2 + KLARA_MARG_SLAB_UNIT - 1) / KLARA_MARG_SLAB_UNIT);
    g->nslabs = (N + g->CH - 1) / g->CH;
    g->lds_bytes = (size_t)4 * (size_t)db * (size_t)g->stride;
    return g->nslabs * g->NDB < (1ll << 31);
}

// ------------------------------------------------------------------------------------------------------------------- update
// the slot of a saved sample x (include/klara_hip.h, klara_gather_histogram).  (x - lo) * inv_w is a subtraction followed by a multiplication: there is no
// fused form of that pair, so nothing here can contract to an fma (and the library is built with -ffp-contract=off).  The minimum is taken in double before
// the conversion — the same value as 1 + min(nbins - 1, (int)floor(.)) wherever that conversion is defined, and defined where x - lo overflows as well.
__device__ __forceinline__ int klara_marg_slot(double x, double lo, double hi, double inv_w, int nbins)
{
    if (x < lo) return 0;
    if (!(x < hi)) return nbins + 1;                             // x >= hi, +inf, NaN
    const double f = __builtin_floor((x - lo) * inv_w);
    return 1 + (int)__builtin_fmin((double)(nbins - 1), f);
}

__global__ __launch_bounds__(KLARA_MARG_THREADS) void k_marg_update(const double* __restrict__ hist, long long N, int D, int nbins, int stride, int DB,
                                                                     int NDB, int CH, long long col0, int m, const double* __restrict__ par,
                                                                     unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned marg_lds[];
    const int tid = threadIdx.x;
    const long long slab = (long long)blockIdx.x / NDB;
    const int db = (int)((long long)blockIdx.x - slab * NDB);
    const int d0 = db * DB, nd = D - d0 < DB ? D - d0 : DB;      // this block's dimensions [d0, d0 + nd)
    const long long c_lo = slab * CH;
    const int nc = (int)(N - c_lo < CH ? N - c_lo : CH);         // this slab's chains
    for (int i = tid; i < nd * stride; i += KLARA_MARG_THREADS) marg_lds[i] = 0u;
    __syncthreads();

    const int CP = KLARA_MARG_THREADS / nd;                      // chains of a pass (>= 4)
    const int dl = tid % nd, cl = tid / nd;
    if (cl < CP) {
        const double lo = par[d0 + dl], hi = par[D + d0 + dl], inv_w = par[2 * D + d0 + dl];
        unsigned* const tab = marg_lds + dl * stride;
        for (int t = 0; t < m; ++t) {
            const double* const col = hist + ((size_t)(col0 + t) * (size_t)N + (size_t)c_lo) * (size_t)D + (size_t)(d0 + dl);
            for (int c = cl; c < nc; c += KLARA_MARG_UNROLL * CP) {
                double x[KLARA_MARG_UNROLL];
#pragma unroll
                for (int u = 0; u < KLARA_MARG_UNROLL; ++u) {
                    const int cc = c + u * CP;
                    x[u] = cc < nc ? col[(size_t)cc * (size_t)D] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < KLARA_MARG_UNROLL; ++u)
                    if (c + u * CP < nc) (void)__hip_atomic_fetch_add(tab + klara_marg_slot(x[u], lo, hi, inv_w, nbins), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    // fold the non-zero words into the table: 64-bit integer adds, exact in any order
    const int S = nbins + 2;
    for (int i = tid; i < nd * stride; i += KLARA_MARG_THREADS) {
        const int d = i / stride, s = i - d * stride;
        const unsigned v = marg_lds[i];
        if (s < S && v != 0u)
            (void)__hip_atomic_fetch_add(counts + (size_t)(d0 + d) * (size_t)S + (size_t)s, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

hipError_t klara_marg_launch_update(const KMargGeom& g, const double* hist, long long col0, long long m, const double* par, unsigned long long* counts,
                                    hipStream_t st)
{
    hipError_t e = hipSuccess;
    for (long long done = 0; done < m && e == hipSuccess; done += KLARA_MARG_MAX_COLS) {
        const int mm = (int)(m - done < KLARA_MARG_MAX_COLS ? m - done : KLARA_MARG_MAX_COLS);
        hipLaunchKernelGGL(k_marg_update, dim3((unsigned)(g.nslabs * g.NDB)), dim3(KLARA_MARG_THREADS), g.lds_bytes, st, hist, g.N, g.D, g.nbins, g.stride,
                           g.DB, g.NDB, (int)g.CH, col0 + done, mm, par, counts);
        e = hipGetLastError();
    }
    return e;
}

// ------------------------------------------------------------------------------------------------------------------- quantiles (host only)
extern "C" klara_status klara_histogram_quantiles(const uint64_t* counts, int32_t ndims, int64_t nbins, const double* lo, const double* hi, int32_t nprobs,
                                                  const double* probs, double* out)
{
    return klara_marg_quantiles(counts, ndims, nbins, lo, hi, nprobs, probs, out) == 0 ? KLARA_OK : KLARA_ERR_INVALID_ARG;
}

// ------------------------------------------------------------------------------------------------------------------- the ranks' agreement (host only)
// klara_gather_histogram's first step over simulated ranks: every rank's words as it stages them, the maximum all-reduce replaced by a host maximum over the
// ranks, the verdict every rank would then reach
extern "C" klara_status klara_selftest_histogram_ranks(int32_t nranks, int32_t ndims, const int64_t* nbins, const double* lo, const double* hi)
{
    if (!nbins || !lo || !hi || nranks < 1 || ndims < 1 || ndims > 1024) return KLARA_ERR_INVALID_ARG;
    const size_t D = (size_t)ndims, NV = 2 * D + 1;
    std::vector<uint64_t> mine(2 * NV), red(2 * NV, 0);
    for (int32_t r = 0; r < nranks; ++r) {
        klara_marg_agreement_words(nbins[r], lo + (size_t)r * D, hi + (size_t)r * D, ndims, mine.data());
        for (size_t i = 0; i < 2 * NV; ++i) if (mine[i] > red[i]) red[i] = mine[i];
    }
    return klara_marg_words_agree(red.data(), NV) ? KLARA_OK : KLARA_ERR_STATE;
}
