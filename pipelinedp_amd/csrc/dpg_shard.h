// dpg_shard.h -- stable multi-way split of records by owner rank (gfx950).
//
// dpg_shard_records orders the records of one rank destination-major before
// the record all-to-all of a multi-GPU release (distributed.shuffle_records):
// destination d = shard(pid) = umulhi((uint32)pid * 0x9E3779B1, R), the
// device form of distributed.shard_of -- or, for wide privacy ids
// (dpg_shard_records_wide), ((fmix64(pid) >> 32) * R) >> 32, the device form
// of distributed.shard_of_wide -- and the records of one destination keep
// their input order.
//
// Three stream-ordered steps, nothing through the host:
//   count    one workgroup per tile of DPG_SHARD_TILE records reads pid only
//            and writes the tile's records per destination to tcnt[d][tile]
//   scan     an exclusive scan of tcnt in that (destination-major) order:
//            tcnt[d][tile] becomes the output index of the tile's first
//            record of destination d
//   scatter  the same tiling reads pid, pk and value and writes every record
//            to its place
//
// Stability comes from ownership, not from atomics: each of the 4 waves of a
// workgroup owns a contiguous quarter of the tile and walks it 64 records at
// a time.  Within one step a lane's rank among the lanes of the same
// destination is ceil(log2 R) ballots (the lanes that agree with it on every
// destination bit) and one mbcnt; the wave's running count per destination
// lives in an LDS row only that wave touches (read by all lanes, written by
// the first lane of each destination: program order, no LDS atomics).  The
// rows of the 4 waves are then scanned on top of the tile's base.
//
// Writes: lanes of one destination write consecutive addresses, so a step of
// a wave stores R runs of ~64 / R records.  The staged form (kStage) first
// orders the tile destination-major in LDS, one 8-byte column at a time
// through one 16 KB buffer, and stores runs of ~DPG_SHARD_TILE / R records
// with consecutive lanes (DESIGN.md section 5 has the measurement).
#pragma once

#include "dpg_wave.h"

#define DPG_SHARD_TILE 2048

namespace dpg {

constexpr uint32_t kShThreads = 256;
constexpr uint32_t kShWaves = kShThreads / 64;
constexpr uint32_t kShRun = DPG_SHARD_TILE / kShWaves;  // records one wave owns
constexpr uint32_t kShSteps = kShRun / 64;
constexpr uint32_t kShMaxR = 64;                        // DPG_SHARD_MAX_RANKS
static_assert(kShRun % 64 == 0 && kShSteps >= 1, "a wave walks whole steps");

__device__ __forceinline__ uint32_t shard_dest(int64_t pid, uint32_t R) {
    return __umulhi((uint32_t)pid * 0x9E3779B1u, R);
}

// The destination function is a template parameter of the kernels below.
// ShardLow32 is shard_dest, the owner of privacy ids that span at most 2^32
// values (dpg_shard_records, dpg_check_shard).  ShardWide hashes all 64 bits:
// the high half of fmix64, as the key dictionary's owner
// (distributed.shard_of_wide = distributed.key_owner), for
// ColumnarData(wide_privacy_ids=True) (dpg_shard_records_wide,
// dpg_check_shard_wide) -- ids that differ only above bit 31 spread over the
// ranks instead of meeting on one.
struct ShardLow32 {
    static __device__ __forceinline__ uint32_t of(int64_t pid, uint32_t R) {
        return shard_dest(pid, R);
    }
};
struct ShardWide {
    static __device__ __forceinline__ uint32_t of(int64_t pid, uint32_t R) {
        return (uint32_t)(((fmix64((uint64_t)pid) >> 32) * R) >> 32);
    }
};

// One step of a wave: the position of this lane's record among the wave's
// records of destination d so far; cnt (the wave's own LDS row) advances by
// the step's records.  Every lane of the wave calls it; lanes past the end of
// the input pass valid = false (d = 0) and get a position nobody uses.
__device__ __forceinline__ uint32_t shard_step(uint32_t *cnt, uint32_t d, bool valid,
                                               uint32_t bits) {
    uint64_t m = __ballot(valid);
    for (uint32_t b = 0; b < bits; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    const uint32_t before = cnt[d];
    wave_sync();
    const uint32_t rank = lanes_below(m);
    if (valid && rank == 0) cnt[d] = before + (uint32_t)__popcll(m);
    wave_sync();
    return before + rank;
}

template <class Dest>
__global__ __launch_bounds__(kShThreads) void k_shard_count(const int64_t *pid, uint32_t n,
                                                            uint32_t R, uint32_t bits,
                                                            uint32_t ntiles, uint32_t *tcnt) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    int64_t p[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) p[k] = i0 + 64u * k < n ? pid[i0 + 64u * k] : 0;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        shard_step(wcnt[w], valid ? Dest::of(p[k], R) : 0u, valid, bits);
    }
    __syncthreads();
    if (tid < R) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t v = 0; v < kShWaves; ++v) c += wcnt[v][tid];
        tcnt[(size_t)tid * ntiles + t] = c;
    }
}

template <bool kStage, class Dest>
__global__ __launch_bounds__(kShThreads) void k_shard_scatter(
    const int64_t *pid, const int64_t *pk, const double *value, uint32_t n, uint32_t R,
    uint32_t bits, uint32_t ntiles, const uint32_t *tbase, int64_t *out_pid, int64_t *out_pk,
    double *out_value) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    __shared__ uint32_t soff[kShMaxR];  // staged: LDS slot = output index + soff[d]
    __shared__ uint64_t sbuf[kStage ? DPG_SHARD_TILE : 1];
    __shared__ uint32_t sdst[kStage ? DPG_SHARD_TILE : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    int64_t p[kShSteps], kk[kShSteps];
    double vv[kShSteps];
    uint32_t d[kShSteps], g[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) p[k] = i0 + 64u * k < n ? pid[i0 + 64u * k] : 0;
    // the other columns load while the ranks are worked out
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        kk[k] = valid ? pk[i0 + 64u * k] : 0;
        vv[k] = valid && value ? value[i0 + 64u * k] : 0.0;
    }
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        d[k] = valid ? Dest::of(p[k], R) : 0u;
        g[k] = shard_step(wcnt[w], d[k], valid, bits);
    }
    __syncthreads();
    // wave 0, lane = destination: the counts of the 4 waves become their
    // output bases on top of the tile's base
    if (tid < 64) {
        const uint32_t tb = tid < R ? tbase[(size_t)tid * ntiles + t] : 0u;
        uint32_t run = tb;
#pragma unroll
        for (uint32_t v = 0; v < kShWaves; ++v) {
            const uint32_t c = wcnt[v][tid];
            wcnt[v][tid] = run;
            run += c;
        }
        if (kStage) {
            uint32_t tot;
            const uint32_t ex = wave_excl_scan(run - tb, tot);
            soff[tid] = ex - tb;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) g[k] += wcnt[w][d[k]];
    if (!kStage) {
#pragma unroll
        for (uint32_t k = 0; k < kShSteps; ++k) {
            if (i0 + 64u * k >= n) continue;
            out_pid[g[k]] = p[k];
            out_pk[g[k]] = kk[k];
            if (value) out_value[g[k]] = vv[k];
        }
        return;
    }
    const uint32_t nt = min((uint32_t)DPG_SHARD_TILE, n - t * (uint32_t)DPG_SHARD_TILE);
    uint32_t slot[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        slot[k] = 0;
        if (i0 + 64u * k >= n) continue;
        slot[k] = g[k] + soff[d[k]];  // < nt
        sdst[slot[k]] = g[k];
        sbuf[slot[k]] = (uint64_t)p[k];
    }
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) out_pid[sdst[j]] = (int64_t)sbuf[j];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k)
        if (i0 + 64u * k < n) sbuf[slot[k]] = (uint64_t)kk[k];
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) out_pk[sdst[j]] = (int64_t)sbuf[j];
    if (!value) return;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k)
        if (i0 + 64u * k < n) sbuf[slot[k]] = (uint64_t)__double_as_longlong(vv[k]);
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads)
        out_value[sdst[j]] = __longlong_as_double((long long)sbuf[j]);
}

// ---- exclusive scan of a[0, M) in place: chunk sums, one workgroup over the
// chunk sums, then every chunk again on top of its base
constexpr uint32_t kScanPer = 8;
constexpr uint32_t kScanChunk = kShThreads * kScanPer;

// Exclusive scan of x over the workgroup (kShThreads threads, all of them
// call it); wtot: kShWaves shared words.
__device__ __forceinline__ uint32_t shard_block_scan(uint32_t x, uint32_t *wtot, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t wt;
    const uint32_t e = wave_excl_scan(x, wt);
    if (lane == 0) wtot[w] = wt;
    __syncthreads();
    uint32_t add = 0;
    total = 0;
#pragma unroll
    for (uint32_t v = 0; v < kShWaves; ++v) {
        const uint32_t c = wtot[v];
        add += v < w ? c : 0u;
        total += c;
    }
    __syncthreads();
    return e + add;
}

__global__ __launch_bounds__(kShThreads) void k_shard_scan_sums(const uint32_t *a, uint32_t M,
                                                                uint32_t *sums) {
    __shared__ uint32_t wtot[kShWaves];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) s += i0 + j < M ? a[i0 + j] : 0u;
    uint32_t total;
    shard_block_scan(s, wtot, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kShThreads) void k_shard_scan_top(uint32_t *sums, uint32_t nchunks) {
    __shared__ uint32_t wtot[kShWaves];
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < nchunks; c0 += kShThreads) {
        const uint32_t i = c0 + threadIdx.x;
        uint32_t total;
        const uint32_t e = shard_block_scan(i < nchunks ? sums[i] : 0u, wtot, total);
        if (i < nchunks) sums[i] = carry + e;
        carry += total;
    }
}

__global__ __launch_bounds__(kShThreads) void k_shard_scan_apply(uint32_t *a, uint32_t M,
                                                                 const uint32_t *sums) {
    __shared__ uint32_t wtot[kShWaves];
    const uint32_t i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
    uint32_t x[kScanPer], s = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        x[j] = i0 + j < M ? a[i0 + j] : 0u;
        s += x[j];
    }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + shard_block_scan(s, wtot, total);
#pragma unroll
    for (uint32_t j = 0; j < kScanPer; ++j) {
        if (i0 + j < M) a[i0 + j] = run;
        run += x[j];
    }
}

// counts[d] = records of destination d, from the scanned tile bases.
__global__ void k_shard_totals(const uint32_t *tbase, uint32_t n, uint32_t R, uint32_t ntiles,
                               int64_t *counts) {
    const uint32_t d = threadIdx.x;
    if (d >= R) return;
    const uint32_t end = d + 1 < R ? tbase[(size_t)(d + 1) * ntiles] : n;
    counts[d] = (int64_t)(end - tbase[(size_t)d * ntiles]);
}

// *n_bad += records whose destination is not `rank` (zeroed by the caller).
template <class Dest>
__global__ __launch_bounds__(kShThreads) void k_check_shard(const int64_t *pid, int64_t n,
                                                            uint32_t R, uint32_t rank,
                                                            unsigned long long *n_bad) {
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kShThreads + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * kShThreads)
        bad += Dest::of(pid[i], R) != rank ? 1u : 0u;
    uint32_t total;
    wave_excl_scan(bad, total);
    if ((threadIdx.x & 63u) == 0 && total) atomicAdd(n_bad, (unsigned long long)total);
}

}  // namespace dpg
