// klara_marg.h — the pooled marginal histograms (klara_desc.marg_nbins > 0, klara_gather_histogram): per dimension d, the saved samples of every chain of
// a handle counted into nbins equal bins over [lo[d], hi[d]) plus an underflow and an overflow slot, after every launch, from the value ring.  Geometry of
// the kernel and its host launcher.  The slot rule is stated once, at klara_gather_histogram (include/klara_hip.h), and implemented once, klara_marg_slot.
//
// Geometry, a function of (N, D, nbins) alone — never of the device or the environment (ADVICE.md on klara_split_lds_bytes):
//   stride = (nbins + 2) | 1    32-bit words of LDS per dimension: odd, so that the lanes of one instruction — adjacent dimensions — that fall into the
//                               same slot of their tables sit in different banks
//   DB  = min(D, 64, KLARA_MARG_LDS_BYTES / (4 stride))     dimensions of a workgroup: 64 up to nbins = 237, 14 at nbins = 1024
//   NDB = ceil(D / DB)                                      dimension blocks
//   CH  = KLARA_MARG_SLAB_UNIT ceil((nbins + 2) / KLARA_MARG_SLAB_UNIT)   chains of a slab: 256 up to nbins = 254, 1280 at nbins = 1024 — a workgroup sees
//                                                           at least one sample per slot and saved step before it folds its table into memory
//   LDS bytes = 4 DB stride <= KLARA_MARG_LDS_BYTES = 60 KiB (two workgroups per compute unit at any nbins)
//
// Update, k_marg_update (after every launch that saved m > 0 columns; at most KLARA_MARG_MAX_COLS = 32 columns per kernel launch, longer updates in
// pieces).  One workgroup of 256 threads per (slab, dimension block), the dimension block the fast index of the grid so that workgroups that touch the
// same cache lines run together.  Thread t takes dimension d0 + t % nd of chain t / nd of a pass of floor(256 / nd) chains (nd = the block's dimensions):
// adjacent lanes read adjacent doubles of one chain's row, a wavefront's load is contiguous — the whole row at D <= 64.  Column t is at hist + t N D.
// Eight passes' loads are issued before their counts.  A count is one 32-bit integer add in LDS (ds_add_u32, no return); when D >= 64 the lanes of one
// instruction fall into 64 different tables, at D < 64 lanes of the same dimension and slot are serialised by the LDS, which stays correct.
// Overflow: a word of a workgroup's table counts at most CH x 32 <= 1280 x 32 = 40,960 samples in one kernel launch, far below 2^32.
// Fold: the workgroup's non-zero words go into the global uint64 [D][nbins + 2] table with 64-bit integer atomic adds (no return).  Integer sums are
// exact in any order: the table is the same for every cut of the saved steps into launches and every geometry.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define KLARA_MARG_THREADS 256         // threads of an update workgroup
#define KLARA_MARG_MAX_DB 64           // dimensions of a workgroup at most: one wavefront's lanes
#define KLARA_MARG_LDS_BYTES 61440     // a workgroup's table at most
#define KLARA_MARG_SLAB_UNIT 256       // chains of a slab: this times ceil((nbins + 2) / this)
#define KLARA_MARG_MAX_COLS 32         // saved steps one kernel launch consumes at most
#define KLARA_MARG_UNROLL 8            // passes whose loads are in flight together

struct KMargGeom {
    long long N, CH, nslabs;           // chains, chains per slab, slabs
    int D, nbins, stride, DB, NDB;     // dimensions, bins, LDS words per dimension, dimensions per workgroup, dimension blocks
    size_t lds_bytes;
};

// false: N <= 0, D outside 1 .. 1024, nbins outside 1 .. KLARA_MARG_MAX_BINS, or more workgroups than a grid holds
bool klara_marg_plan(long long N, int D, long long nbins, KMargGeom* g);
inline size_t klara_marg_count_elems(const KMargGeom& g) { return (size_t)g.D * (size_t)(g.nbins + 2); }

// par = lo[D] | hi[D] | inv_w[D] on the device; columns [col0, col0 + m) of hist (column t at hist + t N D, chain c's D values contiguous) into counts
hipError_t klara_marg_launch_update(const KMargGeom& g, const double* hist, long long col0, long long m, const double* par, unsigned long long* counts,
                                    hipStream_t st);

// inv_w[d] = nbins / (hi[d] - lo[d]), in double: the one place the host forms it
inline double klara_marg_inv_w(long long nbins, double lo, double hi) { return (double)nbins / (hi - lo); }
