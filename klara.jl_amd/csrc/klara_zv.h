// klara_zv.h — zero-variance control variates (lzv / qzv, src/stats/variance/zv.jl, Mira, Solgi & Imparato 2013) over the stored
// value and gradient histories, for every chain of a handle at once.  Geometry of the kernels and their host launchers.
//
// One chain, n saved steps: z = -g / 2, control variates f (n x K; order 1: f = z, K = D; order 2: K = D (D + 3) / 2 columns
// z_i | 2 z_i x_i - 1 | x_i z_j + x_j z_i for i < j, i outer), coefficients A (K x D) from  S_ff A = -S_fx  with the CENTRED
// cross-products S_ff = Fc' Fc, S_fx = Fc' Xc, corrected series c = x + f A.
//
// Stage 1, k_zv_gram.  Time is the reduction dimension of v_mfma_f64_16x16x4_f64: a workgroup stages KLARA_ZV_TB saved steps of its
// chains in LDS as rows [ f (padded to KP = 16 MT columns) | x (padded to 16 XT columns) ] of LDW doubles, centred, and every wavefront
// accumulates its share of the 16 x 16 tiles of  Fc' [Fc | Xc]:  the upper triangle of S_ff (MT (MT + 1) / 2 tiles) and all of S_fx
// (MT XT tiles).  A = a 16-row tile of Fc' (lane l: column 16 rt + (l & 15) of the row of step 4 kk + (l >> 4)), B = a 16-column tile
// of [Fc | Xc] read the same way; the accumulator of lane l holds rows (l >> 4) + 4 r, column l & 15 of the tile.  Centring is two
// passes over the history: the first forms every column's mean as  first sample + sum (value - first sample) / n  (exact for a
// column that never changes), the second accumulates the centred products.  WPC wavefronts share a chain's tiles (TPW tiles each, in
// registers), C = 8 / WPC chains share a workgroup of 8 wavefronts, so D = 4 runs 8 chains per workgroup and K = D = 128 one chain
// whose 100 tiles lie 13 to a wavefront.  An output element is one fma chain over the saved steps in ascending order: it depends on
// the chain's own history alone, not on the number of chains, the chunking or chain_offset.
//
// Stage 2, k_zv_solve.  One workgroup per chain: right-looking Cholesky of S_ff packed in LDS (K = 128: 66,048 B), then forward and
// back substitution for the D right-hand sides in blocks of 16 columns.  A pivot that is not a positive finite number ends the chain
// with info = 1 and NaN coefficients.
//
// Stage 3, k_zv_apply.  Stages the centred rows again and forms the centred corrected series  r = Xc + Fc A  on the matrix cores
// (A = 16 saved steps x 4 columns of Fc, B = the lane's fragments of the coefficients, held in registers), from which
// zv_mean = mean(x) + mean(f) A + mean(r)  and  zv_var = (sum r^2 - (sum r)^2 / n) / (n - 1); optionally writes the series itself.
//
// Pooled form: k_zv_merge folds the chains' (count, mean vector, centred cross-products) into one triple in ascending chain order
// with Chan's update, one thread per matrix element, so the pooled result does not depend on the chunking either.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define KLARA_ZV_TB 16                 // saved steps staged per round (four MFMA k-steps)
#define KLARA_ZV_WAVES 8               // wavefronts of a Gram / apply workgroup
#define KLARA_ZV_MAX_TPW 13            // accumulator tiles a wavefront holds at most (104 VGPRs)
#define KLARA_ZV_WORKSPACE_BYTES ((size_t)480 << 20)    // temporary device memory of one call, everything included (<= 512 MiB)

struct KZvGeom {
    int order, D, K;
    int MT, XT, KP, LDW, ntiles;       // row tiles of f, column tiles of x, 16 MT, 16 (MT + XT), tiles accumulated per chain
    int WPC, C, TPW;                   // Gram: wavefronts per chain, chains per workgroup, tiles per wavefront (instantiated: 1 2 4 8 13)
    int WPA, CA, NKK, STR;             // apply: wavefronts per chain, chains per workgroup, instantiated k-steps (4 8 16 32), LDS row stride
    int solve_threads;
    size_t gram_lds, apply_lds, solve_lds;
    size_t s_elems;                    // KP * LDW doubles of cross-products per chain
    size_t chain_bytes;                // workspace per chain of a chunk
};

// false: more than KLARA_ZV_MAX_TERMS control variates (or an order other than 1, 2)
bool klara_zv_plan(int order, int D, KZvGeom* g);
// chains of one chunk such that the call's workspace stays within KLARA_ZV_WORKSPACE_BYTES
long long klara_zv_chunk(const KZvGeom& g, long long nchains);

hipError_t klara_zv_launch_gram(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                                double* S, double* meanbuf, int means_only, hipStream_t st);
hipError_t klara_zv_launch_solve(const KZvGeom& g, const double* S, long long nchains, double* coef, int* info, hipStream_t st);
hipError_t klara_zv_launch_apply(const KZvGeom& g, const double* hist, const double* hist_g, long long N, long long n, long long c0, long long nc,
                                 const double* meanbuf, const double* coef, size_t coef_stride, double* zv_mean, double* zv_var, double* series,
                                 hipStream_t st);
hipError_t klara_zv_launch_merge(const KZvGeom& g, const double* S, const double* meanbuf, long long nc, double n_per, double count0,
                                 const double* pmean_in, double* pmean_out, double* pS, hipStream_t st);
