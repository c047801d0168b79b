// klara_merge.h — internal, host only (included by klara_handle.h): the between-rank merge (Chan) that ends the pooled moments and the pooled
// covariance.  Rank r holds (mean_r, M_r) over its n_r samples; over the ranks mean = sum n_r mean_r / sum n_r, M = sum M_r + n_r (mean_r - mean)(mean_r - mean)'.
// One staging layout and one sequence of three reductions: klara_gather_moments / klara_gather_covariance run it on one buffer with RCCL all-reduces,
// klara_selftest_pooled / klara_selftest_covariance on one buffer per simulated rank with host sums — the same code, only the collective swapped.
// klara_gather_rhat / klara_selftest_rhat run it too, with chains where the samples stand: rank r holds (mean of its m_r units' means, Bsum_r) and the
// merge is the same; its Wsum_r are X = D further doubles that are only summed over the ranks, in a fourth reduction that a layout with X = 0 never enters.
#pragma once

// One rank's staging buffer, in doubles, for D means and K second-moment elements (K = D: the diagonal, the pooled moments; K = D D: the matrix):
//   [0, D) mean_r | [D, D + K) M_r -> M | 4 u64 counters | D doubles n_r mean_r -> their sum | D doubles mean | X doubles, plain sums over the ranks
// pool_moments_async's output (mean_r, M2_r, the u64 accept total) is the head of the K = D form as it stands: the accept total is counter slot 0.
struct MergeLayout {
    size_t D, K, X = 0;
    enum { ACCEPTED = 0, TRANSITIONS = 1, SAMPLES = 2, CHAINS = 3, NCOUNTERS = 4 };   // the counter slots; SAMPLES summed over the ranks is the merge's ntot
    // R-hat's use of the slots: the merge's samples are its units, so UNITS sits where SAMPLES does; the other two carry the check that every rank holds
    // the same number n_r of samples per unit: (sum m_r n_r)^2 = sum m_r * sum m_r n_r^2 exactly when the n_r are all equal
    enum { UNIT_SAMPLES = 0, UNIT_SAMPLES_SQ = 1, UNITS = 2 };
    size_t mean_r() const { return 0; }
    size_t M() const { return D; }
    size_t counters() const { return D + K; }
    size_t wsum() const { return counters() + NCOUNTERS; }
    size_t mean() const { return wsum() + D; }
    size_t extra() const { return mean() + D; }
    size_t size() const { return extra() + X; }
};

// ---- klara_comm.hip: the rank-local steps on one staging buffer
// buf[wsum + j] = n_r mean_r[j]
hipError_t merge_scale_async(hipStream_t st, const MergeLayout& L, double* buf, double n_r);
// with wsum and the counters summed over the ranks: mean[i] = wsum[i] / ntot (0 when ntot is 0), M[i][j] (K = D: j = i only) += n_r d_i d_j, d = mean_r - mean
hipError_t merge_between_async(hipStream_t st, const MergeLayout& L, double* buf, double n_r);

// The exchange, over the nlocal staging buffers this process holds (n_r[r]: the samples behind buf[r]).  reduce(offset, count, is_u64) sums that slice
// of the buffers over ALL the ranks, in place, and returns false when it failed.  Once the first reduction is entered every later one is entered too —
// a rank that left at its first local failure would leave the others waiting in theirs; false: something failed on the way.
template <class Reduce>
static bool merge_ranks(hipStream_t st, const MergeLayout& L, int nlocal, double* const* buf, const double* n_r, Reduce&& reduce)
{
    bool ok = true;
    for (int r = 0; r < nlocal; ++r) ok &= merge_scale_async(st, L, buf[r], n_r[r]) == hipSuccess;
    ok &= reduce(L.counters(), (size_t)MergeLayout::NCOUNTERS, true);
    ok &= reduce(L.wsum(), L.D, false);
    for (int r = 0; r < nlocal; ++r) ok &= merge_between_async(st, L, buf[r], n_r[r]) == hipSuccess;
    ok &= reduce(L.M(), L.K, false);
    if (L.X) ok &= reduce(L.extra(), L.X, false);
    return ok;
}
