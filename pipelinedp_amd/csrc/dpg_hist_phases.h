// dpg_hist_phases.h -- what the dataset histograms need beyond dpg_hist.h to
// run in three phases (dpg_hist_pairs, dpg_hist_partitions, dpg_hist_sums;
// DESIGN.md section 14): between the phases several ranks merge the
// per-partition totals and the range of the pair sums, so both have to leave
// and re-enter the device code as plain arrays.  The passes over the pairs are
// dpg_hist.h's own kernels (k_hist_pairs, k_hist_lowers, k_hist_sums,
// k_hist_finish), unchanged.
#pragma once

#include "dpg_hist.h"

namespace dpg {

// The P-sized pass of dpg_hist_pairs: the segmented scan's records per
// partition and the partition starts as the two int64 arrays
// dpg_pack_partials reads (rows = pairs, count = records), and the min / max
// keys as doubles ((+inf, -inf): no pair).  n_pairs == 0: pstart is not read.
__global__ __launch_bounds__(kHistThreads) void k_hist_totals(const int64_t *pstart, int64_t P,
                                                              int64_t n_pairs, HistArgs a,
                                                              int64_t *rows, int64_t *count,
                                                              double *range) {
    for (int64_t k = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; k < P;
         k += (int64_t)gridDim.x * kHistThreads) {
        const int64_t np = n_pairs > 0 ? pstart[k + 1] - pstart[k] : 0;
        rows[k] = np > 0 ? np : 0;
        count[k] = np > 0 ? (int64_t)a.pcount[k] : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long k0 = a.minmax[0], k1 = a.minmax[1];
        const bool none = k0 == ~0ull;  // untouched: no double's key is all ones
        range[0] = none ? HUGE_VAL : dkey_inv(k0);
        range[1] = none ? -HUGE_VAL : dkey_inv(k1);
    }
}

// k_hist_parts over given totals (dpg_hist_partitions): rows / count of n
// partitions, merged over ranks by the caller; rows == 0 opens no bin.
__global__ __launch_bounds__(kHistThreads) void k_hist_parts_totals(const int64_t *rows,
                                                                    const int64_t *count,
                                                                    int64_t n, HistArgs a) {
    __shared__ unsigned int small[2][kHiExact];
    for (int i = threadIdx.x; i < 2 * kHiExact; i += kHistThreads) (&small[0][0])[i] = 0;
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; k < n;
         k += (int64_t)gridDim.x * kHistThreads) {
        const int64_t np = rows[k];
        if (np <= 0) continue;
        hi_add(small[0], a, 3, (uint64_t)count[k]);
        hi_add(small[1], a, 4, (uint64_t)np);
    }
    __syncthreads();
    hi_flush(small[0], a, 3);
    hi_flush(small[1], a, 4);
}

// dpg_hist_sums: the range of the whole dataset (doubles) as the ordered keys
// k_hist_lowers reads; dkey_inv(dkey(x)) is x bit for bit.  min > max (no pair
// anywhere): the keys of (0, 0), whose edges are all 0.0 -- the zero fill.
__global__ void k_hist_range_keys(const double *range, HistArgs a) {
    const double lo = range[0], hi = range[1];
    const bool any = lo <= hi;
    a.minmax[0] = dkey(any ? lo : 0.0);
    a.minmax[1] = dkey(any ? hi : 0.0);
}

}  // namespace dpg
