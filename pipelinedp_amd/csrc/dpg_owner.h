// dpg_owner.h -- stable split of partition-keyed items by owner rank (gfx950).
//
// A multi-GPU release with percentiles or VECTOR_SUM moves per-partition items
// (the kept tree keys pk << 16 | leaf, or the occupied partitions pk of the
// per-rank vector sums) to the rank that owns their partition
// (distributed.exchange_owner_keys).  dpg_owner_split_keys orders one rank's
// keys destination-major for that all-to-all:
//   pk    = key >> low_bits
//   owner = pk % R                        (distributed.owner_of)
//   key'  = (pk / R) << low_bits | low    the key in the owner's local ids
// and keeps the keys of one destination in their input order.  The optional
// payload is the input position of every output entry, by which the caller
// gathers whatever travels with the keys.
//
// The count / scan / scatter skeleton, shard_step and the scan kernels are
// dpg_shard.h's: one workgroup per tile of DPG_SHARD_TILE keys, each of the 4
// waves owns a contiguous quarter and walks it 64 keys at a time, a lane's
// rank inside its destination is ceil(log2 R) ballots and one mbcnt, the
// wave's running counts live in an LDS row only that wave touches (no
// atomics: stability comes from ownership), and the tile is ordered
// destination-major in LDS before consecutive lanes store runs of
// ~DPG_SHARD_TILE / R entries.
//
// What differs from the record split: the destination and the re-based key
// are one 32-bit division by the wave-uniform R; the key count lives on the
// device, as in dpg_rsort.h (the launches are sized by the host's bound n_max,
// a tile past the count writes zero counts and returns); the payload is one
// uint32 column, staged beside the keys, so the scatter needs no second trip
// through the LDS buffer.
#pragma once

#include "dpg_rsort.h"

namespace dpg {

// pk / R and pk % R of the key's partition; R is wave-uniform.
__device__ __forceinline__ uint32_t owner_dest(uint64_t key, uint32_t low_bits, uint32_t R,
                                               uint32_t &local) {
    const uint32_t pk = (uint32_t)(key >> low_bits);
    local = pk / R;
    return pk - local * R;
}

__global__ __launch_bounds__(kShThreads) void k_owner_count(const uint64_t *keys, uint32_t n_max,
                                                            const int64_t *n_dev,
                                                            uint32_t low_bits, uint32_t R,
                                                            uint32_t bits, uint32_t ntiles,
                                                            uint32_t *tcnt) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    const uint32_t n = rs_count(n_max, n_dev);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    if ((uint64_t)t * DPG_SHARD_TILE >= n) {  // past the device count: an empty tile
        if (tid < R) tcnt[(size_t)tid * ntiles + t] = 0;
        return;
    }
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    uint64_t key[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) key[k] = i0 + 64u * k < n ? keys[i0 + 64u * k] : 0;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        uint32_t local;
        const uint32_t d = owner_dest(key[k], low_bits, R, local);
        shard_step(wcnt[w], valid ? d : 0u, valid, bits);
    }
    __syncthreads();
    if (tid < R) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t v = 0; v < kShWaves; ++v) c += wcnt[v][tid];
        tcnt[(size_t)tid * ntiles + t] = c;
    }
}

// kSrc: out_src is written too.
template <bool kSrc>
__global__ __launch_bounds__(kShThreads) void k_owner_scatter(
    const uint64_t *keys, uint32_t n_max, const int64_t *n_dev, uint32_t low_bits, uint32_t R,
    uint32_t bits, uint32_t ntiles, const uint32_t *tbase, uint64_t *out_keys,
    uint32_t *out_src) {
    __shared__ uint32_t wcnt[kShWaves][kShMaxR];
    __shared__ uint32_t soff[kShMaxR];  // LDS slot = output index + soff[d]
    __shared__ uint64_t sbuf[DPG_SHARD_TILE];
    __shared__ uint32_t sdst[DPG_SHARD_TILE];
    __shared__ uint32_t ssrc[kSrc ? DPG_SHARD_TILE : 1];
    const uint32_t n = rs_count(n_max, n_dev);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t = blockIdx.x;
    if ((uint64_t)t * DPG_SHARD_TILE >= n) return;
    wcnt[w][lane] = 0;
    wave_sync();
    const uint32_t i0 = t * (uint32_t)DPG_SHARD_TILE + w * kShRun + lane;
    const uint64_t lowm = (1ull << low_bits) - 1ull;  // low_bits <= 32
    uint64_t key[kShSteps];
    uint32_t d[kShSteps], g[kShSteps];
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) key[k] = i0 + 64u * k < n ? keys[i0 + 64u * k] : 0;
#pragma unroll
    for (uint32_t k = 0; k < kShSteps; ++k) {
        const bool valid = i0 + 64u * k < n;
        uint32_t local;
        d[k] = owner_dest(key[k], low_bits, R, local);
        d[k] = valid ? d[k] : 0u;
        key[k] = ((uint64_t)local << low_bits) | (key[k] & lowm);
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
        sbuf[slot] = key[k];
        if (kSrc) ssrc[slot] = i0 + 64u * k;
    }
    __syncthreads();
    for (uint32_t j = tid; j < nt; j += kShThreads) {
        const uint32_t o = sdst[j];
        out_keys[o] = sbuf[j];
        if (kSrc) out_src[o] = ssrc[j];
    }
}

// counts[d] = keys of destination d, from the scanned tile bases; the total
// is the device count (k_shard_totals takes it from the host).
__global__ void k_owner_totals(const uint32_t *tbase, uint32_t n_max, const int64_t *n_dev,
                               uint32_t R, uint32_t ntiles, int64_t *counts) {
    const uint32_t d = threadIdx.x;
    if (d >= R) return;
    const uint32_t n = rs_count(n_max, n_dev);
    const uint32_t end = d + 1 < R ? tbase[(size_t)(d + 1) * ntiles] : n;
    counts[d] = (int64_t)(end - tbase[(size_t)d * ntiles]);
}

}  // namespace dpg
