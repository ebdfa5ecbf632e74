// dpg_rsort.h -- stable LSD radix sort of (uint64 key, uint32 payload) (gfx950).
//
// The kept-record route (dpg_records.h) and the quantile tree (dpg_quantile.h)
// order records by wide keys; this is their sort.  8-bit digits on the count /
// scan / scatter skeleton of dpg_shard.h:
//   hist     one pass over the input keys fills the histogram of every digit
//            of [begin_bit, end_bit); k_rs_plan then decides on the device,
//            without a host round trip, which passes run: a digit with one
//            occupied value orders nothing and its pass is skipped.  The plan
//            also routes the buffers (input -> ... -> output, through one
//            temporary) so that the last pass that runs writes the output.
//   count    per pass: one workgroup per tile of DPG_SHARD_TILE records
//            writes the tile's records per digit value to tcnt[d][tile]
//   scan     the exclusive scan of tcnt in that (digit-major) order
//            (dpg_shard.h's scan kernels)
//   scatter  the same tiling ranks every record and writes it to its place
//
// Stability comes from ownership, as in dpg_shard.h: each of the 4 waves of a
// workgroup owns a contiguous quarter of the tile and walks it 64 records at
// a time; a lane's rank among the lanes of its digit value is 8 ballots and
// one mbcnt (shard_step), the wave's running counts live in a 256-entry LDS
// row only that wave touches (no LDS atomics).  Writes are staged through LDS
// digit-major, one column at a time, so that consecutive lanes store runs.
//
// The record count may live on the device (n_dev): the launches are sized by
// the host's upper bound and tiles past the device count write zero counts
// and return.
#pragma once

#include "dpg_shard.h"

namespace dpg {

constexpr uint32_t kRsDigits = 256;
constexpr uint32_t kRsMaxPasses = 8;

// One pass as k_rs_plan routes it: buffers 0 = input, 1 = temporary,
// 2 = output.
struct RsPass {
    uint32_t skip, src, dst, pad;
};
struct RsPlan {
    RsPass pass[kRsMaxPasses];
    uint32_t n_run;  // passes that run; 0: the input is copied to the output
    uint32_t pad[3];
};

struct RsBufs {
    const uint64_t *kin;
    const uint32_t *vin;  // NULL: keys only
    uint64_t *ktmp, *kout;
    uint32_t *vtmp, *vout;
    __device__ __forceinline__ const uint64_t *keys(uint32_t b) const {
        return b == 0 ? kin : (b == 1 ? ktmp : kout);
    }
    __device__ __forceinline__ const uint32_t *vals(uint32_t b) const {
        return b == 0 ? vin : (b == 1 ? vtmp : vout);
    }
};

__device__ __forceinline__ uint32_t rs_count(uint32_t n_max, const int64_t *n_dev) {
    if (!n_dev) return n_max;
    const int64_t v = *n_dev;
    return v < 0 ? 0u : (v > (int64_t)n_max ? n_max : (uint32_t)v);
}

__device__ __forceinline__ uint32_t rs_digit(uint64_t key, uint32_t shift, uint32_t mask) {
    return (uint32_t)(key >> shift) & mask;
}

// hist[p][d] += keys whose digit p is d (zeroed by the caller).
__global__ __launch_bounds__(kShThreads) void k_rs_hist(const uint64_t *keys, uint32_t n_max,
                                                        const int64_t *n_dev, uint32_t begin_bit,
                                                        uint32_t end_bit, uint32_t npass,
                                                        uint32_t *hist) {
    __shared__ uint32_t h[kRsMaxPasses][kRsDigits];
    const uint32_t n = rs_count(n_max, n_dev);
    for (uint32_t j = threadIdx.x; j < kRsMaxPasses * kRsDigits; j += kShThreads)
        (&h[0][0])[j] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kShThreads + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * kShThreads) {
        const uint64_t key = keys[i];
        for (uint32_t p = 0; p < npass; ++p) {
            const uint32_t shift = begin_bit + 8u * p;
            const uint32_t w = min(8u, end_bit - shift);
            const uint32_t d = rs_digit(key, shift, (1u << w) - 1u);
            // a digit the whole wave agrees on (the constant ones a pass is
            // skipped for) costs one LDS atomic, not 64 to one address
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
            const uint64_t act = __ballot(1);
            if (__ballot(d == d0) == act) {
                if (lanes_below(act) == 0) atomicAdd(&h[p][d0], (uint32_t)__popcll(act));
            } else {
                atomicAdd(&h[p][d], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < npass * kRsDigits; j += kShThreads) {
        const uint32_t c = (&h[0][0])[j];
        if (c) atomicAdd(&hist[j], c);
    }
}

// One workgroup of kRsDigits threads: which passes run, and their buffers.
__global__ __launch_bounds__(kRsDigits) void k_rs_plan(const uint32_t *hist, uint32_t n_max,
                                                       const int64_t *n_dev, uint32_t npass,
                                                       RsPlan *plan) {
    __shared__ uint32_t skip[kRsMaxPasses];
    const uint32_t n = rs_count(n_max, n_dev);
    if (threadIdx.x < kRsMaxPasses) skip[threadIdx.x] = n == 0 ? 1u : 0u;
    __syncthreads();
    for (uint32_t p = 0; p < npass; ++p)
        if (hist[p * kRsDigits + threadIdx.x] == n) skip[p] = 1u;  // every writer writes 1
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t k = 0;
    for (uint32_t p = 0; p < npass; ++p) k += skip[p] ? 0u : 1u;
    uint32_t j = 0, cur = 0;
    for (uint32_t p = 0; p < kRsMaxPasses; ++p) {
        RsPass r{1u, 0u, 0u, 0u};
        if (p < npass && !skip[p]) {
            ++j;
            r.skip = 0;
            r.src = cur;
            r.dst = ((k - j) & 1u) ? 1u : 2u;  // the k-th pass that runs writes the output
            cur = r.dst;
        }
        plan->pass[p] = r;
    }
    plan->n_run = k;
}

// No pass runs: output = input.
__global__ __launch_bounds__(kShThreads) void k_rs_copy(RsBufs b, uint32_t n_max,
                                                        const int64_t *n_dev, const RsPlan *plan) {
    if (plan->n_run != 0) return;
    const uint32_t n = rs_count(n_max, n_dev);
    for (uint64_t i = (uint64_t)blockIdx.x * kShThreads + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * kShThreads) {
        b.kout[i] = b.kin[i];
        if (b.vin) b.vout[i] = b.vin[i];
    }
}

// The rank of this lane's record among the wave's records of digit d so far
// (shard_step over 8 digit bits; cnt is the wave's own 256-entry row).
__device__ __forceinline__ uint32_t rs_step(uint32_t *cnt, uint32_t d, bool valid) {
    return shard_step(cnt, d, valid, 8u);
}

__global__ __launch_bounds__(kShThreads) void k_rs_count(RsBufs b, uint32_t n_max,
                                                         const int64_t *n_dev, const RsPlan *plan,
                                                         uint32_t p, uint32_t shift, uint32_t mask,
                                                         uint32_t ntiles, uint32_t *tcnt) {
    __shared__ uint32_t wcnt[kShWaves][kRsDigits];
    const RsPass ps = plan->pass[p];
    if (ps.skip) return;
    const uint32_t n = rs_count(n_max, n_dev);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    if ((uint64_t)t * DPG_SHARD_TILE >= n) {  // past the device count: an empty tile
        tcnt[(size_t)tid * ntiles + t] = 0;
        return;
    }
    const uint64_t *keys = b.keys(ps.src);
#pragma unroll
    for (uint32_t j = 0; j < kRsDigits / 64; ++j) wcnt[w][lane + 64u * j] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    uint64_t key[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) key[k] = i0 + 64u * k < n ? keys[i0 + 64u * k] : 0;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        rs_step(wcnt[w], valid ? rs_digit(key[k], shift, mask) : 0u, valid);
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (uint32_t v = 0; v < kShWaves; ++v) c += wcnt[v][tid];
    tcnt[(size_t)tid * ntiles + t] = c;
}

__global__ __launch_bounds__(kShThreads) void k_rs_scatter(RsBufs b, uint32_t n_max,
                                                           const int64_t *n_dev,
                                                           const RsPlan *plan, uint32_t p,
                                                           uint32_t shift, uint32_t mask,
                                                           uint32_t ntiles,
                                                           const uint32_t *tbase) {
    __shared__ uint32_t wcnt[kShWaves][kRsDigits];
    __shared__ uint32_t soff[kRsDigits];  // LDS slot = output index + soff[d]
    __shared__ uint32_t wtot[kShWaves];
    __shared__ uint64_t sbuf[DPG_SHARD_TILE];
    __shared__ uint32_t sdst[DPG_SHARD_TILE];
    const RsPass ps = plan->pass[p];
    if (ps.skip) return;
    const uint32_t n = rs_count(n_max, n_dev);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    if ((uint64_t)t * DPG_SHARD_TILE >= n) return;
    const uint64_t *keys = b.keys(ps.src);
    const uint32_t *vals = b.vals(ps.src);
    uint64_t *okeys = ps.dst == 1 ? b.ktmp : b.kout;
    uint32_t *ovals = ps.dst == 1 ? b.vtmp : b.vout;
#pragma unroll
    for (uint32_t j = 0; j < kRsDigits / 64; ++j) wcnt[w][lane + 64u * j] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    uint64_t key[kShSteps];
    uint32_t val[kShSteps], d[kShSteps], g[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) key[k] = i0 + 64u * k < n ? keys[i0 + 64u * k] : 0;
    // the payload loads while the ranks are worked out
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) val[k] = vals && i0 + 64u * k < n ? vals[i0 + 64u * k] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        d[k] = valid ? rs_digit(key[k], shift, mask) : 0u;
        g[k] = rs_step(wcnt[w], d[k], valid);
    }
    __syncthreads();
    // thread = digit value: the counts of the 4 waves become their output
    // bases on top of the tile's base
    {
        const uint32_t tb = tbase[(size_t)tid * ntiles + t];
        uint32_t run = tb;
#pragma unroll
        for (uint32_t v = 0; v < kShWaves; ++v) {
            const uint32_t c = wcnt[v][tid];
            wcnt[v][tid] = run;
            run += c;
        }
        uint32_t tot;
        const uint32_t ex = shard_block_scan(run - tb, wtot, tot);  // syncs the workgroup
        soff[tid] = ex - tb;
    }
    __syncthreads();
    const uint32_t nt = min((uint32_t)DPG_SHARD_TILE, n - t * (uint32_t)DPG_SHARD_TILE);
    uint32_t slot[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        slot[k] = 0;
        if (i0 + 64u * k >= n) continue;
        g[k] += wcnt[w][d[k]];
        slot[k] = g[k] + soff[d[k]];  // < nt
        sdst[slot[k]] = g[k];
        sbuf[slot[k]] = key[k];
    }
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) okeys[sdst[j]] = sbuf[j];
    if (!vals) return;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k)
        if (i0 + 64u * k < n) sbuf[slot[k]] = val[k];
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) ovals[sdst[j]] = (uint32_t)sbuf[j];
}

}  // namespace dpg
