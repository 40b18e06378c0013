// Running mean / variance bookkeeping shared by every kernel that keeps one (K5's trackers, the environment filters, the
// value normaliser of K12 / K15 / K22).  Each rank reduces its batch to a float64 record (n, mean, M2); the records are
// merged with Chan's formula in rank order -- equal to the moments of the concatenated batch the reference gathers
// (utils/stats.py:47-54) -- and integrated into the float32 state with the reference's own update (utils/stats.py:73-94).
// One copy of the arithmetic: the kernels must agree bitwise with each other and with the reference.
#pragma once
#include <hip/hip_runtime.h>

namespace ppoaf {

// one record (nb, mb, m2b) into the running triple; an empty record changes nothing
__device__ __forceinline__ void chan_merge(double& n, double& mean, double& M2, const double nb, const double mb, const double m2b) {
    if (nb <= 0.0) return;
    const double d = mb - mean, nn = n + nb;
    mean += d * (nb / nn);
    M2 += m2b + d * d * n * nb / nn;
    n = nn;
}

// the merged batch (n, bm, M2) into the state: batch mean / population variance in the data's dtype (stats.py:52-54),
// then stats.py:73-94 in its expression order; mean / var float32, counts float64.  For n > 0 only: an empty batch
// leaves the state alone, and the caller asks (a test in here moves the block in every caller's instruction stream)
__device__ __forceinline__ void running_integrate(float& mean, float& var, double& count, const double n, const double bm, const double M2) {
    const float batch_mean = (float)bm, batch_var = (float)(M2 / n);
    const float delta = batch_mean - mean;
    const double new_count = count + n;
    const float new_mean = (float)((double)mean + (double)delta * (n / new_count));
    const double m_2 = (double)var * count + (double)batch_var * n + (double)(delta * delta) * count * n / (count + n);
    mean = new_mean; var = (float)(m_2 / (count + n)); count = new_count;
}

// the value normaliser's state for mini-batch `mb`: slot mb & 1 of the double-buffered state, advanced by the mini-batch's
// u.n_ranks records (the caller publishes it and stores the other slot)
template <typename U>
__device__ __forceinline__ void minibatch_vn_state(const U& u, const long mb, float& m, float& v, double& cnt) {
    const int slot = (int)(mb & 1);
    m = u.vn_mean[slot]; v = u.vn_var[slot]; cnt = u.vn_count[slot];
    if (u.normalize_values) {
        double n = 0.0, bm = 0.0, M2 = 0.0;
        for (int r = 0; r < u.n_ranks; ++r) {
            const double* rec = u.vn_records + (mb * u.n_ranks + r) * 3;
            chan_merge(n, bm, M2, rec[0], rec[1], rec[2]);
        }
        if (n > 0.0) running_integrate(m, v, cnt, n, bm, M2);
    }
}

// a mini-batch's advantage record (n, mean, M2) -> mean and sample standard deviation (ppo.py:2326-2333)
__device__ __forceinline__ void adv_mean_std(const double* rec, float& mean, float& std) {
    mean = (float)rec[1];
    std = (float)sqrt(rec[2] / (rec[0] - 1.0));
}

}  // namespace ppoaf
