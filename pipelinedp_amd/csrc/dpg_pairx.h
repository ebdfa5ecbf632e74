// dpg_pairx.h -- the pair exchange of a multi-GPU utility analysis (gfx950).
//
// The per-partition utility combiners need all (privacy id, partition) pairs
// of a partition in one place, so every rank's pre-aggregate (24-byte
// dpg_pair_entry, sorted by partition key) travels to the partitions' owners
// (pk % R, distributed.exchange_owner_pairs).  Two device steps frame the
// all-to-all:
//
//   dpg_owner_split_pairs   the sender orders its pairs destination-major,
//                           input order kept inside a destination, and
//                           rewrites pk to the owner's local id pk / R
//   dpg_merge_pair_runs     the owner merges the R pk-sorted runs it received
//                           into one pk-sorted pre-aggregate with its
//                           partition_start
//
// The split is the count / scan / scatter skeleton of dpg_shard.h /
// dpg_owner.h (one workgroup per tile of DPG_SHARD_TILE entries, each wave
// owns a quarter, ballots + mbcnt ranks, LDS rows only their wave touches).
// What differs is the entry: 24 bytes, moved whole.  A lane loads its entry
// in one piece (16 + 8 bytes, not three strided 8-byte columns), the tile is
// ordered destination-major in LDS (2048 x 24 B = 48 KB) and consecutive lanes
// store consecutive whole entries of a run.  Only pk changes; the other 20
// bytes are copied as bits.  The count pass reads pk alone, but at a 24-byte
// stride that is every cache line: the split moves 72 B per pair, 48 of them
// in the scatter.
//
// The merge is a counting placement, not a sort: the runs are sorted already.
//   bounds   a pair is a segment head if its run starts there or its
//            predecessor has another pk, a tail likewise; head and tail add
//            -position and position + 1 to cnt[pk][run] (integer atomics, two
//            per segment, no contention) and the head records its position
//   scan     cnt, partition-major, through dpg_shard.h's scan kernels: the
//            output base of every (partition, run) segment, and with it the
//            partition starts
//   place    out[base[pk][run] + position - head position] = pair
// O(n + runs x P) work, no floating point touched, the same output on every
// execution.  A pair with pk >= P, or with a pk below that of an in-range
// predecessor in its run, is bad: counted, never written.
#pragma once

#include "dpg_shard.h"

namespace dpg {

// One entry moved as three 8-byte words, which the compiler merges into a
// 16-byte and an 8-byte access (a 24-byte struct copy becomes two overlapping
// 16-byte ones: 32 bytes moved per entry).
__device__ __forceinline__ void pair_copy(ItemPA *dst, const ItemPA *src) {
    uint64_t a, b, c;
    const char *s = reinterpret_cast<const char *>(src);
    char *d = reinterpret_cast<char *>(dst);
    __builtin_memcpy(&a, s, 8);
    __builtin_memcpy(&b, s + 8, 8);
    __builtin_memcpy(&c, s + 16, 8);
    __builtin_memcpy(d, &a, 8);
    __builtin_memcpy(d + 8, &b, 8);
    __builtin_memcpy(d + 16, &c, 8);
}

// ---------------------------------------------------------------- the split
__global__ __launch_bounds__(kShThreads) void k_pairx_count(const ItemPA *pairs, uint32_t n,
                                                            uint32_t R, uint32_t bits,
                                                            uint32_t ntiles, uint32_t *tcnt) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    uint32_t pk[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) pk[k] = i0 + 64u * k < n ? pairs[i0 + 64u * k].pk : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        shard_step(wcnt[w], valid ? pk[k] % R : 0u, valid, bits);
    }
    __syncthreads();
    if (tid < R) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t v = 0; v < kShWaves; ++v) c += wcnt[v][tid];
        tcnt[(size_t)tid * ntiles + t] = c;
    }
}

__global__ __launch_bounds__(kShThreads) void k_pairx_scatter(const ItemPA *pairs, uint32_t n,
                                                              uint32_t R, uint32_t bits,
                                                              uint32_t ntiles,
                                                              const uint32_t *tbase,
                                                              ItemPA *out) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    __shared__ uint32_t soff[kShMaxR];  // LDS slot = output index + soff[d]
    __shared__ ItemPA sbuf[DPG_SHARD_TILE];
    __shared__ uint32_t sdst[DPG_SHARD_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    ItemPA e[kShSteps];
    uint32_t d[kShSteps], g[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k)
        e[k] = i0 + 64u * k < n ? pairs[i0 + 64u * k] : ItemPA{0, 0, 0.0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        const uint32_t local = e[k].pk / R;
        d[k] = valid ? e[k].pk - local * R : 0u;
        e[k].pk = local;
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
        uint32_t tot;
        const uint32_t ex = wave_excl_scan(run - tb, tot);
        soff[tid] = ex - tb;
    }
    __syncthreads();
    const uint32_t nt = min((uint32_t)DPG_SHARD_TILE, n - t * (uint32_t)DPG_SHARD_TILE);
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        if (i0 + 64u * k >= n) continue;
        const uint32_t o = g[k] + wcnt[w][d[k]];  // output index, < n
        const uint32_t slot = o + soff[d[k]];     // < nt
        sdst[slot] = o;
        sbuf[slot] = e[k];
    }
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) pair_copy(&out[sdst[j]], &sbuf[j]);
}

// ---------------------------------------------------------------- the merge
struct PairRuns {
    uint32_t nruns;
    uint32_t start[kShMaxR + 1];  // run r is [start[r], start[r + 1])
};

// The run of position i: the last r with start[r] <= i (empty runs skipped).
__device__ __forceinline__ uint32_t pairx_run_of(const PairRuns &rs, uint32_t i) {
    uint32_t lo = 0, hi = rs.nruns;  // start[lo] <= i < start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rs.start[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// What both passes of the merge agree on about pair i of run r.
struct PairSeg {
    bool ok;       // in range and not below an in-range predecessor of its run
    bool head;     // first pair of its (partition, run) segment
    bool tail;     // last one
    uint32_t pk;
};

__device__ __forceinline__ PairSeg pairx_seg(const ItemPA *pairs, const PairRuns &rs, uint32_t i,
                                             uint32_t r, uint32_t P) {
    PairSeg s;
    s.pk = pairs[i].pk;
    const bool first = i == rs.start[r], last = i + 1 == rs.start[r + 1];
    const uint32_t prev = first ? 0u : pairs[i - 1].pk;
    const uint32_t next = last ? 0u : pairs[i + 1].pk;
    s.ok = s.pk < P && (first || prev >= P || prev <= s.pk);
    s.head = first || prev != s.pk;
    s.tail = last || next != s.pk;
    return s;
}

// cnt[pk * nruns + r] += block length (tail position + 1 - head position,
// wrapping uint32 sums) for every block of equal in-range pks of run r (one
// per partition in an ascending run: the segment), first[pk * nruns + r] =
// head position; *n_bad += bad pairs.  cnt is zeroed by the caller.
__global__ __launch_bounds__(kShThreads) void k_pairx_bounds(const ItemPA *pairs, PairRuns rs,
                                                             uint32_t n, uint32_t P,
                                                             uint32_t *cnt, uint32_t *first,
                                                             unsigned long long *n_bad) {
    uint32_t bad = 0;
    for (uint32_t i = blockIdx.x * kShThreads + threadIdx.x; i < n; i += gridDim.x * kShThreads) {
        const uint32_t r = pairx_run_of(rs, i);
        const PairSeg s = pairx_seg(pairs, rs, i, r, P);
        if (!s.ok) ++bad;
        // A bad pair in range heads its block of equal pks (its predecessor is
        // larger).  Alone in the block it counts nothing; in front of a longer
        // block it is counted with it, a slot nobody writes: cnt stays a sum
        // of lengths of disjoint blocks whatever the input, so the starts
        // ascend and end at or below n.
        if (s.pk >= P || (!s.ok && s.tail)) continue;
        const size_t m = (size_t)s.pk * rs.nruns + r;
        if (s.head) {
            first[m] = i;
            atomicSub(&cnt[m], i);
        }
        if (s.tail) atomicAdd(&cnt[m], i + 1u);
    }
    uint32_t total;
    wave_excl_scan(bad, total);
    if ((threadIdx.x & 63u) == 0 && total) atomicAdd(n_bad, (unsigned long long)total);
}

// base: the scanned cnt (M + 1 entries, base[M] = slots laid out, <= n).
__global__ __launch_bounds__(kShThreads) void k_pairx_place(const ItemPA *pairs, PairRuns rs,
                                                            uint32_t n, uint32_t P,
                                                            const uint32_t *base,
                                                            const uint32_t *first, ItemPA *out) {
    for (uint32_t i = blockIdx.x * kShThreads + threadIdx.x; i < n; i += gridDim.x * kShThreads) {
        const uint32_t r = pairx_run_of(rs, i);
        const PairSeg s = pairx_seg(pairs, rs, i, r, P);
        if (!s.ok) continue;
        const size_t m = (size_t)s.pk * rs.nruns + r;
        const uint32_t o = base[m] + (i - first[m]);
        // always true for ascending runs; a run that is not (n_bad > 0) can
        // hold several blocks of one partition, whose pairs must still be
        // written inside the output
        if (o < n) pair_copy(&out[o], &pairs[i]);
    }
}

// partition_start[p] = base[p * nruns], p <= P.
__global__ __launch_bounds__(kShThreads) void k_pairx_starts(const uint32_t *base, uint32_t nruns,
                                                             int64_t P, int64_t *partition_start) {
    for (int64_t p = (int64_t)blockIdx.x * kShThreads + threadIdx.x; p <= P;
         p += (int64_t)gridDim.x * kShThreads)
        partition_start[p] = (int64_t)base[(size_t)p * nruns];
}

}  // namespace dpg
