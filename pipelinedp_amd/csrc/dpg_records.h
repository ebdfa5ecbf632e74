// dpg_records.h -- the kept RECORDS of contribution bounding (gfx950).
//
// The bounding kernels emit one item per kept (privacy id, partition) pair;
// percentiles (dpg_quantile.h) need the kept records themselves.  This is a
// second, independent, sort-based route to the same kept set, in the
// oracle's order (oracle/dp_oracle.c dpo_bound_aggregate_ids):
//   pairs of a privacy id ascending by (pair_prio << 32 | pk), first mpc kept;
//   records of a pair ascending by the 64-bit rec_prio, first mcpp kept.
//
// The composite key (pid - pid_min, pair_prio, pk, rec_prio) is 160 bits; the
// stable sort of dpg_rsort.h takes it least-significant part first, 64 bits
// at a time, the payload being the record's index: by rec_prio, then by
// (pair_prio << 32 | pk), then by pid - pid_min (k_rec_key computes each
// part from the payload).  Records of non-public partitions (and records
// with keys out of range, which also raise the error bit) get the largest
// pair key, so they sort behind every real pair of their privacy id, take no
// rank from it and are never kept.
//
// One marking pass over the sorted sequence raises pair-start and pid-start
// flags (from the sorted pid keys and one gather of pk; a flag byte per
// record hands them to the apply pass); a device-wide scan (count / top /
// apply over tiles of 2048) carries (pair starts so far, the pair ordinal at
// the last pid start, the position of the last pair start), from which
//   pair rank   = pair ordinal - ordinal at the pid's start
//   record rank = position - the pair's start
// and keep[index] = pair rank < mpc && record rank < mcpp.
#pragma once

#include "dpg_rsort.h"

namespace dpg {

struct RecArgs {
    const int64_t *pid, *pk;
    const uint8_t *pub;  // bitmap of P bits or NULL
    uint64_t pid_min, U; // U == 0: no declared range (any 64-bit id)
    uint64_t P;
    uint64_t seed;       // stream seed
    uint64_t rec_id_offset;
    uint32_t mpc, mcpp;  // saturated to 2^32 - 1
    uint32_t cross;      // DPG_MODE_CROSS_PARTITION: every record of a kept pair
};

// 0: a record bounding sees; 1: of a non-public partition; 2: key out of range
__device__ __forceinline__ uint32_t rec_dropped(const RecArgs &a, int64_t pid, int64_t pk) {
    if ((uint64_t)pk >= a.P) return 2u;
    if (a.U && (uint64_t)pid - a.pid_min >= a.U) return 2u;
    if (a.pub && !((a.pub[pk >> 3] >> (pk & 7)) & 1)) return 1u;
    return 0u;
}

// kPart 0: rec_prio of record i (and the identity payload), from the input
// order; 1: the pair key, 2: pid - pid_min, of the record the payload names.
template <int kPart>
__global__ __launch_bounds__(256) void k_rec_key(RecArgs a, uint32_t n, const uint32_t *idx_in,
                                                 uint64_t *keys, uint32_t *idx_out,
                                                 uint32_t *err) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n;
         j += (uint64_t)gridDim.x * 256) {
        const uint32_t i = idx_in ? idx_in[j] : (uint32_t)j;
        const int64_t p = a.pid[i], k = a.pk[i];
        if constexpr (kPart == 0) {
            if (rec_dropped(a, p, k) == 2u) atomicOr(err, 1u);
            idx_out[j] = i;
            keys[j] = rec_prio_h(pid_hash(a.seed, (uint64_t)p), (uint32_t)k, a.rec_id_offset + i);
        } else if constexpr (kPart == 1) {
            keys[j] = rec_dropped(a, p, k)
                          ? ~0ull
                          : ((uint64_t)pair_prio_h(pid_hash(a.seed, (uint64_t)p), (uint32_t)k) << 32) |
                                (uint32_t)k;
        } else {
            keys[j] = (uint64_t)p - a.pid_min;
        }
    }
}

constexpr uint32_t kRmPer = DPG_SHARD_TILE / kShThreads;  // consecutive records of a thread
static_assert(kRmPer == 8, "a thread's flag bytes fill one 64-bit word");

// Maximum of x over the workgroup (all kShThreads threads call it).
__device__ __forceinline__ uint32_t rec_block_max(uint32_t x, uint32_t *wtot) {
    for (int o = 32; o > 0; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
    if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t m = 0;
#pragma unroll
    for (uint32_t v = 0; v < kShWaves; ++v) m = max(m, wtot[v]);
    __syncthreads();
    return m;
}

// Exclusive prefix maximum of x over the workgroup (identity 0).
__device__ __forceinline__ uint32_t rec_block_excl_max(uint32_t x, uint32_t *wtot,
                                                       uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = x;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= (uint32_t)o) inc = max(inc, y);
    }
    uint32_t ex = (uint32_t)__shfl_up((int)inc, 1);
    if (lane == 0) ex = 0;
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t v = 0; v < kShWaves; ++v) {
        const uint32_t c = wtot[v];
        before = max(before, v < w ? c : 0u);
        total = max(total, c);
    }
    __syncthreads();
    return max(ex, before);
}

// Flag bits of one record of the sorted sequence (k_rec_mark_count writes
// them, one byte per record, so that the apply pass gathers nothing).
constexpr uint32_t kRfPair = 1u, kRfPid = 2u, kRfDrop = 4u;

// The flags of the kRmPer records of this thread, packed one byte each
// (byte r: record j0 + r), from the sorted pid keys (sequential) and the pk
// of the record each payload names (gathered, once).
__device__ __forceinline__ uint64_t rec_flags(const RecArgs &a, const uint64_t *skey,
                                              const uint32_t *idx, uint32_t n, uint32_t j0) {
    uint64_t f = 0;
    uint64_t pp = 0;
    int64_t pkk = 0;
    if (j0 > 0 && j0 < n) {
        pp = skey[j0 - 1];
        pkk = a.pk[idx[j0 - 1]];
    }
#pragma unroll
    for (uint32_t r = 0; r < kRmPer; ++r) {
        if (j0 + r >= n) continue;
        const uint64_t p = skey[j0 + r];
        const int64_t k = a.pk[idx[j0 + r]];
        const bool ps = j0 + r == 0 || p != pp;
        const bool ks = ps || k != pkk;
        bool drop = (uint64_t)k >= a.P || (a.U && p >= a.U);
        if (!drop && a.pub) drop = !((a.pub[k >> 3] >> (k & 7)) & 1);
        f |= (uint64_t)((ks ? kRfPair : 0u) | (ps ? kRfPid : 0u) | (drop ? kRfDrop : 0u)) << (8u * r);
        pp = p;
        pkk = k;
    }
    return f;
}

// bit r of the result: byte r of f has `bit` set
__device__ __forceinline__ uint32_t rec_flag_bits(uint64_t f, uint32_t bit) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < kRmPer; ++r) m |= (uint32_t)((f >> (8u * r)) & bit ? 1u : 0u) << r;
    return m;
}

// Per tile: pair starts, the tile-local inclusive pair ordinal at its last
// pid start (0: none) and the position + 1 of its last pair start (0: none);
// per record its flag byte (flags holds whole groups of kRmPer bytes).
__global__ __launch_bounds__(kShThreads) void k_rec_mark_count(RecArgs a, const uint64_t *skey,
                                                               const uint32_t *idx, uint32_t n,
                                                               uint64_t *flags, uint32_t *tsum,
                                                               uint32_t *tord, uint32_t *tpos) {
    __shared__ uint32_t wtot[kShWaves];
    const uint32_t j0 = blockIdx.x * (uint32_t)DPG_SHARD_TILE + threadIdx.x * kRmPer;
    const uint64_t f = rec_flags(a, skey, idx, n, j0);
    if (j0 < n) flags[j0 / kRmPer] = f;
    const uint32_t pairbits = rec_flag_bits(f, kRfPair), pidbits = rec_flag_bits(f, kRfPid);
    const uint32_t cnt = (uint32_t)__popc(pairbits);
    uint32_t total;
    const uint32_t e = shard_block_scan(cnt, wtot, total);
    uint32_t ord = 0, pos = 0;
    if (pidbits) {
        const uint32_t r = 31u - (uint32_t)__clz((int)pidbits);
        ord = e + (uint32_t)__popc(pairbits & ((2u << r) - 1u));
    }
    if (pairbits) pos = j0 + (31u - (uint32_t)__clz((int)pairbits)) + 1u;
    ord = rec_block_max(ord, wtot);
    pos = rec_block_max(pos, wtot);
    if (threadIdx.x == 0) {
        tsum[blockIdx.x] = total;
        tord[blockIdx.x] = ord;
        tpos[blockIdx.x] = pos;
    }
}

// One workgroup: the tiles' triples become what precedes each tile.
__global__ __launch_bounds__(kShThreads) void k_rec_mark_top(uint32_t ntiles, uint32_t *tsum,
                                                             uint32_t *tord, uint32_t *tpos) {
    __shared__ uint32_t wtot[kShWaves];
    uint32_t csum = 0, cord = 0, cpos = 0;
    for (uint32_t c0 = 0; c0 < ntiles; c0 += kShThreads) {
        const uint32_t i = c0 + threadIdx.x;
        const bool in = i < ntiles;
        const uint32_t s = in ? tsum[i] : 0u, o = in ? tord[i] : 0u, q = in ? tpos[i] : 0u;
        uint32_t total, omax, qmax;
        const uint32_t e = shard_block_scan(s, wtot, total);
        const uint32_t oe = rec_block_excl_max(o ? csum + e + o : 0u, wtot, omax);
        const uint32_t qe = rec_block_excl_max(q, wtot, qmax);
        if (in) {
            tsum[i] = csum + e;
            tord[i] = max(cord, oe);
            tpos[i] = max(cpos, qe);
        }
        csum += total;
        cord = max(cord, omax);
        cpos = max(cpos, qmax);
    }
}

__global__ __launch_bounds__(kShThreads) void k_rec_mark_apply(RecArgs a, const uint32_t *idx,
                                                               uint32_t n, const uint64_t *flags,
                                                               const uint32_t *tsum,
                                                               const uint32_t *tord,
                                                               const uint32_t *tpos,
                                                               uint8_t *keep) {
    __shared__ uint32_t wtot[kShWaves];
    const uint32_t j0 = blockIdx.x * (uint32_t)DPG_SHARD_TILE + threadIdx.x * kRmPer;
    const uint64_t f = j0 < n ? flags[j0 / kRmPer] : 0ull;
    const uint32_t pairbits = rec_flag_bits(f, kRfPair), pidbits = rec_flag_bits(f, kRfPid);
    const uint32_t dropbits = rec_flag_bits(f, kRfDrop);
    const uint32_t base = tsum[blockIdx.x];
    uint32_t total;
    const uint32_t e = shard_block_scan((uint32_t)__popc(pairbits), wtot, total);
    uint32_t ord = 0, pos = 0;
    if (pidbits) {
        const uint32_t r = 31u - (uint32_t)__clz((int)pidbits);
        ord = base + e + (uint32_t)__popc(pairbits & ((2u << r) - 1u));
    }
    if (pairbits) pos = j0 + (31u - (uint32_t)__clz((int)pairbits)) + 1u;
    uint32_t t0, t1;
    uint32_t pidord = max(tord[blockIdx.x], rec_block_excl_max(ord, wtot, t0));
    uint32_t pairpos = max(tpos[blockIdx.x], rec_block_excl_max(pos, wtot, t1));
    uint32_t run = base + e;
#pragma unroll
    for (uint32_t r = 0; r < kRmPer; ++r) {
        if (j0 + r >= n) continue;
        if ((pairbits >> r) & 1u) {
            ++run;
            pairpos = j0 + r + 1u;
        }
        if ((pidbits >> r) & 1u) pidord = run;
        const uint32_t pair_rank = run - pidord, rec_rank = j0 + r + 1u - pairpos;
        const bool k = !((dropbits >> r) & 1u) && pair_rank < a.mpc &&
                       (a.cross || rec_rank < a.mcpp);
        keep[idx[j0 + r]] = k ? 1 : 0;
    }
}

}  // namespace dpg
