// klara_cov.h — the pooled posterior covariance (KLARA_MON_COVARIANCE, klara_gather_covariance): over every chain c of a handle and every
// saved step t, mean[D] and M[D x D] = sum (x - mean)(x - mean)', accumulated while sampling on the FP64 matrix cores.  Geometry of the
// kernels and their host launchers.
//
// Shift.  z = x - pivot, pivot[D] = the first saved sample of local chain 0 (copied out of the value ring before the first update): the sums
// do not grow with the offset of the posterior, and chains that all sit at one point give z = 0, hence M = 0 and mean = x exactly.
//
// Slabs.  The N chains are cut into slabs of CH = klara_cov_slab(N, D) consecutive chains: CH = 64, doubled while the
// ceil(N / CH) slabs' accumulators — per slab ntiles 16 x 16 tiles of doubles and 16 MT doubles of T, MT = ceil(D / 16),
// ntiles = MT (MT + 1) / 2 — exceed KLARA_COV_WORKSPACE_BYTES.  A function of (N, D) alone: never of the device or the environment.
// Slab s keeps S_s = the upper tiles of sum z z' and T_s = sum z in device memory between launches; nothing is added atomically.
//
// Update, k_cov_update (after every launch that saved m > 0 columns; at most 32 columns per kernel launch).  One workgroup of 4 wavefronts
// per (slab, tile group).  The slab's samples are taken in the order (saved step ascending, then chain ascending), every saved step padded
// with z = 0 to a multiple of 4 chains, so that a k-step of v_mfma_f64_16x16x4_f64 (4 samples) never straddles a saved step; KLARA_COV_KB
// samples at a time are staged in LDS as rows of 16 MT doubles (columns >= D: zeros) while the next ones travel in registers.  The upper tiles (I, J >= I), numbered row by row,
// are dealt to the wavefronts in runs of TPW consecutive tiles (TPW <= 13 accumulators in registers, tile group g = a workgroup's 4 TPW
// tiles; D = 256: 136 tiles = 3 groups of 4 x 12).  A = lane l: column 16 I + (l & 15) of the row of sample 4 kk + (l >> 4); B likewise for
// J — for a diagonal tile the same register.  The accumulators start from S_s and go back to it, so an element of S_s is ONE fma chain
// over the slab's samples in that order whatever the split of the saved steps over launches: padding adds fma(0, 0, acc) = acc.
// T_s[d] is a plain sum in the same order (tile group 0, thread d).
//
// Finalize, k_cov_finalize (at gather time; the accumulators are only read).  Thread (i, j >= i): S = sum of S_s, T_i, T_j = sums of
// T_s over the slabs in ascending order from 0.0; mean_i = pivot_i + T_i / n; M_ij = (S - qh) - ql with T_i T_j / n = qh + ql carried in
// double-double (two-prod of the product, remainder of the division by fma); the diagonal is clamped at 0; M_ji = M_ij.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define KLARA_COV_WAVES 4              // wavefronts of an update workgroup
#define KLARA_COV_KB 16                // samples staged per round (four MFMA k-steps)
#define KLARA_COV_MAX_TPW 13           // accumulator tiles a wavefront holds at most (104 VGPRs)
#define KLARA_COV_SLAB_MIN 64          // chains of a slab at least
#define KLARA_COV_MAX_COLS 32          // saved steps one kernel launch consumes at most
#define KLARA_COV_WORKSPACE_BYTES ((size_t)480 << 20)    // the slabs' accumulators at most (as KLARA_ZV_WORKSPACE_BYTES)

struct KCovGeom {
    long long N, CH, nslabs;           // chains, chains per slab, slabs
    int D, MT, DP, ntiles;             // dimensions, row tiles, 16 MT, upper tiles
    int TPW, NG;                       // tiles per wavefront, tile groups (grid.y)
    size_t slab_elems;                 // 256 ntiles doubles of S per slab (T: DP per slab)
};

// false: D outside 1 .. KLARA_COV_MAX_DIMS or N <= 0
bool klara_cov_plan(long long N, int D, KCovGeom* g);
long long klara_cov_slab(long long N, int D);
inline size_t klara_cov_S_elems(const KCovGeom& g) { return (size_t)g.nslabs * g.slab_elems; }
inline size_t klara_cov_T_elems(const KCovGeom& g) { return (size_t)g.nslabs * (size_t)g.DP; }

// columns [col0, col0 + m) of hist (column t at hist + t N D, chain c's D values contiguous) into S / T, in pieces of KLARA_COV_MAX_COLS columns
hipError_t klara_cov_launch_update(const KCovGeom& g, const double* hist, long long col0, long long m, const double* pivot, double* S, double* T,
                                   hipStream_t st);
// out = mean[D], M[D x D] from the accumulators of n = saved steps x N samples (n > 0)
hipError_t klara_cov_launch_finalize(const KCovGeom& g, const double* S, const double* T, const double* pivot, double n, double* out, hipStream_t st);
