// dpg_sample.h -- the partition sampler of the utility analysis and the
// public-partitions summary.
//
// k_sample_partitions: one key per lane.  The lane hashes its key
// (dpg_sha1.h: SHA-1 of the decimal repr, first 64 bits) and votes
// H < bound; the wave's 64 votes are one ballot, which is exactly the 8 mask
// bytes of keys 64w .. 64w + 63 (bit i of the mask = bit i & 7 of byte
// i >> 3 = bit i & 63 of little-endian word i >> 6).  Lane 0 stores the word:
// no atomics, no read-modify-write, and the tail bits of the last word are
// the zero votes of the lanes past n.
//
// k_summary_mark / k_summary_count: presence bytes of the partitions the
// data touches, then one pass over the partitions counting the three classes
// of PublicPartitionsSummary.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpg_sha1.h"

namespace dpg {

constexpr int kSampleThreads = 256;  // 4 waves: 4 mask words per workgroup pass

__global__ __launch_bounds__(kSampleThreads) void k_sample_partitions(
    const int64_t *keys, uint64_t key_lo, uint64_t key_stride, int64_t n, uint64_t bound,
    int keep_all, unsigned long long *mask, unsigned long long *hashes) {
    // base is wave-uniform (64 consecutive threads share it), so whole waves
    // enter and leave the loop together and the ballot sees all 64 lanes
    const int lane = threadIdx.x & 63;
    for (int64_t base = ((int64_t)blockIdx.x * kSampleThreads + (threadIdx.x & ~63)); base < n;
         base += (int64_t)gridDim.x * kSampleThreads) {
        const int64_t i = base + lane;
        bool keep = false;
        if (i < n) {
            // dense ids: key_lo + i * key_stride, in wrapping arithmetic
            const int64_t key = keys ? keys[i] : (int64_t)(key_lo + (uint64_t)i * key_stride);
            const uint64_t h = sha1_key_hash(key);
            if (hashes) hashes[i] = h;
            keep = keep_all || h < bound;
        }
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) mask[base >> 6] = votes;
    }
}

constexpr int kSummaryThreads = 256;

// present[k] = 1 for every key of pk; keys outside [0, P) set *bad instead.
// Plain byte stores: every writer of a byte writes the same value.
__global__ __launch_bounds__(kSummaryThreads) void k_summary_mark(const int64_t *pk, int64_t n,
                                                                  int64_t P, uint8_t *present,
                                                                  uint32_t *bad) {
    for (int64_t i = (int64_t)blockIdx.x * kSummaryThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kSummaryThreads) {
        const int64_t k = pk[i];
        if ((uint64_t)k >= (uint64_t)P)
            *bad = 1;
        else
            present[k] = 1;
    }
}

// counts[0] += present and public, [1] += present and not public, [2] +=
// public and not present, over the partitions [0, P): per-lane counters, a
// wave reduction, an LDS combine of the 4 waves and one atomicAdd per
// counter and workgroup.
__global__ __launch_bounds__(kSummaryThreads) void k_summary_count(
    const uint8_t *present, const uint8_t *public_mask, int64_t P, unsigned long long *counts) {
    unsigned int c0 = 0, c1 = 0, c2 = 0;  // < 2^32 partitions
    for (int64_t k = (int64_t)blockIdx.x * kSummaryThreads + threadIdx.x; k < P;
         k += (int64_t)gridDim.x * kSummaryThreads) {
        const bool here = present[k] != 0;
        const bool pub = (public_mask[k >> 3] >> (k & 7)) & 1;
        c0 += here && pub;
        c1 += here && !pub;
        c2 += !here && pub;
    }
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_down(c0, off, 64);
        c1 += __shfl_down(c1, off, 64);
        c2 += __shfl_down(c2, off, 64);
    }
    __shared__ unsigned int part[kSummaryThreads / 64][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = c0;
        part[wave][1] = c1;
        part[wave][2] = c2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long t = 0;
        for (int w = 0; w < kSummaryThreads / 64; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(&counts[threadIdx.x], t);
    }
}

}  // namespace dpg
