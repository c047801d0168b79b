// klara_derived.h — derived quantities (klara_desc.derived_nout > 0): one user closure y = klara_user_derived(x), K = derived_nout outputs, evaluated on
// every saved sample of every chain after each launch, from the value ring; per chain the running sums of y and y * y, and — when histograms of the
// outputs were asked for — the values of a launch's columns staged as [column][chain][K] for k_marg_update (klara_marg.h).  The contract is stated at
// klara_desc.derived_src (include/klara_hip.h).  This file is read twice: by the library (geometry and host launcher, below) and by the run-time compiler,
// where klara_jit.hip puts it behind the fixed-width typedefs, detmath.h and the user's text and defines KLARA_DERIVED_KERNEL (the kernel, at the end).
//
// Geometry, a function of (N, D, K) alone — never of the device or the environment (ADVICE.md on klara_split_lds_bytes):
//   stride  = D | 1                                          doubles of LDS per chain row: odd, so that the lanes of one ds_read_b64 — adjacent chains at the
//                                                            same element — fall into 32 different bank pairs (a half-wave per pass, no conflict)
//   CH      = min(256, KLARA_DERIVED_LDS_BYTES / (8 stride)) chains of a workgroup: 256 up to D = 29, 76 at D = 100, 7 at D = 1024
//   threads = 64 ceil(CH / 64)
//   workgroup g owns chains [g CH, min(N, (g + 1) CH)); dynamic LDS bytes = 8 CH stride <= 60 KiB
// A closure that names a kd_ function adds detmath.h's 8 KB of static tables: up to 69,504 B in all (D = 479), more than the 64 KB a launch gets without
// asking through the runtime's launch API (klara_launch.h) — a module launch (hipModuleLaunchKernel) is bound by the 160 KB a gfx950 workgroup may hold,
// nothing else, and tests/test_gpu_derived.py runs that shape.  The rows are the kernel's only dynamic LDS: the kd_* functions that read kd_screm_lds
// (kd_sincos2pi_tab20 and the transition kernels' table gathers) would read chain rows as table entries and are not for closures (include/klara_hip.h names the ones that are).
//
// Update, k_derived_update (at most KLARA_DERIVED_MAX_COLS = 32 columns per kernel launch, as the marginals; longer updates in pieces).  Lane l < live owns
// chain g CH + l: it reads the chain's K + K accumulators once, before the first column, and writes them once, after the last.  Per column the workgroup
// copies its chains' rows — one contiguous run of live * D doubles of the column — into LDS, lane after lane (a wavefront's load is 512 contiguous bytes,
// four loads in flight per lane), synchronises, every live lane calls the closure on its LDS row, adds y and y * y (the product rounded, then added: the
// translation unit is built with -ffp-contract=off) in ascending saved step, stores y to the staging column when staging is compiled in, and the workgroup
// synchronises before the next column overwrites the rows.  A chain's result depends on that chain alone; no atomics of any kind.
#pragma once

#define KLARA_DERIVED_LDS_BYTES 61440  // a workgroup's rows at most
#define KLARA_DERIVED_MAX_CH 256       // chains (= lanes that evaluate) of a workgroup at most
#define KLARA_DERIVED_MAX_COLS 32      // saved steps one kernel launch consumes at most (= KLARA_MARG_MAX_COLS: the staging array's columns)

#ifndef KLARA_DERIVED_KERNEL
#include <stddef.h>

struct KDerivedGeom {
    long long N, nwg;                  // chains, workgroups
    int D, K, stride, CH, threads;     // dimensions, outputs, doubles per LDS row, chains per workgroup, threads per workgroup
    size_t lds_bytes;
};

// false: N <= 0, D outside 1 .. 1024, K outside 1 .. 64, or more workgroups than a grid holds
inline bool klara_derived_plan(long long N, int D, int K, KDerivedGeom* g)
{
    if (N <= 0 || D < 1 || D > 1024 || K < 1 || K > 64) return false;
    g->N = N; g->D = D; g->K = K;
    g->stride = D | 1;
    int ch = KLARA_DERIVED_LDS_BYTES / (8 * g->stride);
    if (ch > KLARA_DERIVED_MAX_CH) ch = KLARA_DERIVED_MAX_CH;
    g->CH = ch;
    g->threads = 64 * ((ch + 63) / 64);
    g->nwg = (N + ch - 1) / ch;
    g->lds_bytes = (size_t)8 * (size_t)ch * (size_t)g->stride;
    return g->nwg < (1ll << 31);
}

#else  // ---------------------------------------------------------------------------------------------------------- the kernel (run-time compiled)

// KLARA_D, KLARA_K, KLARA_DERIVED_THREADS, KLARA_DERIVED_STAGE (0 / 1) and, when the user's text names a kd_ function, KLARA_DERIVED_TABLES are defined by
// klara_jit.hip; klara_user_derived is the user's.  hist: column t at hist + t N D, chain c's D values contiguous.  stage: [m][N][K].
__global__ __launch_bounds__(KLARA_DERIVED_THREADS) void k_derived_update(const double* __restrict__ hist, long long N, int CH, long long col0, int m,
                                                                          const double* __restrict__ data, long long ndata, double* __restrict__ dsum,
                                                                          double* __restrict__ dsumsq, double* __restrict__ stage)
{
    extern __shared__ double der_rows[];
#ifdef KLARA_DERIVED_TABLES
    kd_tables_to_lds();
#endif
    constexpr int D = KLARA_D, K = KLARA_K, STRIDE = KLARA_D | 1, UNROLL = 4;
    const int tid = (int)threadIdx.x;
    const long long c_lo = (long long)blockIdx.x * CH;
    const int live = (int)(N - c_lo < CH ? N - c_lo : CH);       // this workgroup's chains
    const bool mine = tid < live;
    const size_t acc = (size_t)(c_lo + tid) * (size_t)K;
    double s[K], q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { s[k] = mine ? dsum[acc + k] : 0.0; q[k] = mine ? dsumsq[acc + k] : 0.0; }
    const int n = live * D;                                       // doubles of a column that are this workgroup's
    for (int t = 0; t < m; ++t) {
        const double* const col = hist + ((size_t)(col0 + t) * (size_t)N + (size_t)c_lo) * (size_t)D;
        for (int i0 = tid; i0 < n; i0 += UNROLL * KLARA_DERIVED_THREADS) {
            double v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = i0 + u * KLARA_DERIVED_THREADS;
                v[u] = i < n ? col[i] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = i0 + u * KLARA_DERIVED_THREADS;
                if (i < n) { const int r = i / D; der_rows[r * STRIDE + (i - r * D)] = v[u]; }
            }
        }
        __syncthreads();
        if (mine) {
            double y[K];
            klara_user_derived(der_rows + tid * STRIDE, D, data, ndata, y, K);
#pragma unroll
            for (int k = 0; k < K; ++k) { s[k] = s[k] + y[k]; q[k] = q[k] + y[k] * y[k]; }
#if KLARA_DERIVED_STAGE
            double* const o = stage + ((size_t)t * (size_t)N + (size_t)(c_lo + tid)) * (size_t)K;
#pragma unroll
            for (int k = 0; k < K; ++k) o[k] = y[k];
#endif
        }
        __syncthreads();
    }
    if (mine) {
#pragma unroll
        for (int k = 0; k < K; ++k) { dsum[acc + k] = s[k]; dsumsq[acc + k] = q[k]; }
    }
}
#endif
