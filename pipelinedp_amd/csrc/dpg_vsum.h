// dpg_vsum.h -- per-partition vector sums over the kept records (gfx950).
//
// Replaces the reference's VectorSumCombiner (pipeline_dp/combiners.py): the
// accumulator is the coordinate-wise sum of the kept records' vectors of a
// partition, the release clips the summed vector to a norm and adds noise to
// every coordinate.
//
// dpg_vector_index writes one key pk << 31 | i per kept record i and sorts
// the keys (dpg_rsort.h).  The record index makes every key unique, so the
// sorted sequence is a pure function of (pk, keep), whatever places the
// compaction's counter handed out.  The sorted keys are the inverted index:
// partition k owns a run of consecutive positions, ascending by record index.
//
// k_vsum_chunks sums without atomics.  The sorted positions are cut into
// chunks of DPG_VSUM_CHUNK; one wave takes one chunk and sums it segment by
// segment (a segment: the positions of one partition inside the chunk), so a
// wave's work is bounded by the chunk however the records spread over the
// partitions.  A segment that touches neither edge of its chunk is the whole
// partition and is stored to out[k].  A segment that starts at the chunk's
// first position is stored to the chunk's head partial, one that starts later
// and ends at the chunk's last position to its tail partial (two rows of D
// per chunk in the workspace, with the partition each belongs to).
// k_vsum_merge then adds, for every partition with partials, the partials in
// chunk order.
//
// Summation order (the contract: a fixed function of the sorted keys and D,
// independent of the grid, of n_cu and of which wave took which chunk).  Let
// Dp = min(64, D rounded up to a power of two) and R = 64 / Dp.  A lane is
// (sub-slot s = lane / Dp, coordinate d = piece * 64 + lane % Dp); for D > 64
// the coordinates are taken in pieces of 64 and R = 1.  For a segment of
// rows r_0 .. r_{m-1} (ascending position, i.e. ascending record index):
//   1. sub-slot s adds, starting from 0.0 and left to right, the rows
//      r_s, r_{s+R}, r_{s+2R}, ...                       (kVsFlight loads of a
//      sub-slot are issued before its adds; the adds keep this order);
//   2. the R sub-slot sums are combined by the butterfly x += shfl_xor(x, m)
//      for m = Dp, 2 Dp, ..., 32  (IEEE addition commutes, so every lane of
//      a coordinate ends with the same bits);
//   3. a partition cut by chunk edges is  (..((p_0 + p_1) + p_2).. + p_j)
//      over its per-chunk partials p in chunk order, each p by 1. and 2.
#pragma once

#include "dpg_quantile.h"
#include "dpg_rsort.h"

namespace dpg {

constexpr uint32_t kVsChunk = DPG_VSUM_CHUNK;
constexpr uint32_t kVsFlight = 4;  // rows in flight per sub-slot
constexpr uint32_t kVsNone = 0xFFFFFFFFu;  // no partition (P < 2^32 - 1)
constexpr uint64_t kVsIdxMask = 0x7FFFFFFFull;
static_assert(kVsChunk == 512, "k_vsum_chunks holds a chunk as 8 keys per lane");

// keys[*n_keys ...] = pk << 31 | i of every record i with keep[i] != 0 and pk
// in [0, P), in any order (the keys are sorted next); *n_keys is zeroed by
// the caller.  The block-wide reservation of k_quantile_keys.
__global__ __launch_bounds__(256) void k_vector_keys(const int64_t *pk, const uint8_t *keep,
                                                     uint32_t n, uint64_t P, uint64_t *keys,
                                                     unsigned long long *n_keys) {
    __shared__ uint32_t wsum[4];
    __shared__ unsigned long long sbase;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t tile = 256ull * kQkPer;
    for (uint64_t t0 = (uint64_t)blockIdx.x * tile; t0 < n; t0 += (uint64_t)gridDim.x * tile) {
        uint64_t key[kQkPer];
        uint32_t off[kQkPer];
        bool take[kQkPer];
        uint32_t wcount = 0;
#pragma unroll
        for (uint32_t r = 0; r < kQkPer; ++r) {
            const uint64_t i = t0 + 256ull * r + threadIdx.x;
            take[r] = false;
            key[r] = 0;
            if (i < n && keep[i]) {
                const int64_t k = pk[i];
                if ((uint64_t)k < P) {
                    take[r] = true;
                    key[r] = ((uint64_t)k << 31) | i;
                }
            }
            const uint64_t b = __ballot(take[r]);
            off[r] = wcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            wcount += (uint32_t)__popcll(b);
        }
        if (lane == 0) wsum[w] = wcount;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            sbase = total ? atomicAdd(n_keys, (unsigned long long)total) : 0ull;
        }
        __syncthreads();
        unsigned long long base = sbase;
        for (uint32_t v = 0; v < w; ++v) base += wsum[v];
#pragma unroll
        for (uint32_t r = 0; r < kQkPer; ++r)
            if (take[r]) keys[base + off[r]] = key[r];
        __syncthreads();  // wsum and sbase are rewritten by the next round
    }
}

__device__ __forceinline__ uint32_t vs_count(const int64_t *n_keys, uint32_t n) {
    const int64_t v = *n_keys;
    return v < 0 ? 0u : (v > (int64_t)n ? n : (uint32_t)v);
}

__device__ __forceinline__ double vs_shfl_xor(double x, uint32_t m) {
    const long long u = __double_as_longlong(x);
    const int lo = __shfl_xor((int)(uint32_t)u, (int)m);
    const int hi = __shfl_xor((int)(uint32_t)((uint64_t)u >> 32), (int)m);
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

// First position p > a of the chunk with flag[p] set (flags: 8 wave-uniform
// words, bit l of word r = position 64 r + l), or cnt if there is none.
__device__ __forceinline__ uint32_t vs_next_flag(const uint64_t (&flag)[8], uint32_t a,
                                                 uint32_t cnt) {
    const uint32_t from = a + 1u;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
        uint64_t x = flag[r];
        if (r < (from >> 6)) x = 0;
        else if (r == (from >> 6)) x &= ~0ull << (from & 63u);
        if (x) return 64u * r + (uint32_t)__builtin_ctzll(x);
    }
    return cnt;
}

// Blocks of 256 threads: wave = chunk (grid stride).  part: [2 * chunk +
// (0 head, 1 tail)][D]; hpk / tpk: the partition of the chunk's head / tail
// partial, kVsNone when it has none.  out is zero-filled by the caller.
__global__ __launch_bounds__(256) void k_vsum_chunks(const uint64_t *keys, const int64_t *n_keys,
                                                     const double *value, uint32_t n, uint32_t D,
                                                     uint64_t P, double *out, double *part,
                                                     uint32_t *hpk, uint32_t *tpk) {
    __shared__ uint32_t s_idx[4][kVsChunk];
    __shared__ uint32_t s_pk[4][kVsChunk];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t nk = vs_count(n_keys, n);
    const uint32_t nchunks = (nk + kVsChunk - 1u) / kVsChunk;
    uint32_t Dp = 1;
    while (Dp < D && Dp < 64u) Dp <<= 1;
    const uint32_t R = 64u / Dp, sub = lane / Dp, dl = lane % Dp;
    uint32_t *idx = s_idx[w], *spk = s_pk[w];
    for (uint32_t c = blockIdx.x * 4u + w; c < nchunks; c += gridDim.x * 4u) {  // wave-uniform
        const uint32_t base = c * kVsChunk;
        const uint32_t cnt = min(kVsChunk, nk - base);
        // ---- the chunk's keys: record index and partition to LDS, segment starts as flags
        uint64_t flag[8];
        uint32_t prev_last = kVsNone;
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
            const uint32_t p = 64u * r + lane;
            const bool valid = p < cnt;
            const uint64_t key = valid ? keys[(uint64_t)base + p] : ~0ull;
            const uint32_t k = (uint32_t)(key >> 31);
            idx[p] = (uint32_t)(key & kVsIdxMask);
            spk[p] = k;
            uint32_t before = (uint32_t)__shfl_up((int)k, 1);
            if (lane == 0) before = prev_last;
            flag[r] = __ballot(valid && (p == 0 || k != before));
            prev_last = (uint32_t)__builtin_amdgcn_readlane((int)k, 63);
        }
        wave_sync();
        uint32_t head_pk = kVsNone, tail_pk = kVsNone;
        uint32_t a = 0;
        while (a < cnt) {  // wave-uniform
            const uint32_t b = vs_next_flag(flag, a, cnt);
            const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)spk[a]);
            double *dst;
            if (a == 0) {
                dst = part + (uint64_t)(2u * c) * D;
                head_pk = k;
            } else if (b == cnt) {
                dst = part + (uint64_t)(2u * c + 1u) * D;
                tail_pk = k;
            } else {
                dst = out + (uint64_t)k * D;
            }
            const bool dst_ok = (uint64_t)k < P;  // keys of dpg_vector_index always are
            for (uint32_t d0 = 0; d0 < D; d0 += 64u) {  // one piece when D <= 64
                const uint32_t d = d0 + dl;
                const bool lane_ok = d < D;
                double acc = 0.0;
                for (uint32_t j0 = a; j0 < b; j0 += kVsFlight * R) {  // wave-uniform
                    double v[kVsFlight];
                    bool ok[kVsFlight];
#pragma unroll
                    for (uint32_t f = 0; f < kVsFlight; ++f) {
                        const uint32_t j = j0 + f * R + sub;
                        ok[f] = false;
                        v[f] = 0.0;
                        if (lane_ok && j < b) {
                            const uint32_t i = idx[j];
                            if (i < n) {
                                ok[f] = true;
                                v[f] = value[(uint64_t)i * D + d];
                            }
                        }
                    }
#pragma unroll
                    for (uint32_t f = 0; f < kVsFlight; ++f)
                        if (ok[f]) acc += v[f];
                }
                for (uint32_t m = Dp; m < 64u; m <<= 1) acc += vs_shfl_xor(acc, m);
                if (dst_ok && lane_ok && sub == 0) dst[d] = acc;
            }
            a = b;
        }
        if (lane == 0) {
            hpk[c] = head_pk;
            tpk[c] = tail_pk;
        }
        wave_sync();  // the next chunk rewrites idx / spk
    }
}

// The partials of a partition are consecutive in the sequence head(0),
// tail(0), head(1), tail(1), ...: a tail partial starts a partition's run, a
// head partial starts one when the chunk before ends with another partition,
// and the run goes on through the head partials of the following chunks for
// as long as they carry the same partition.  A group of G = min(64, Dp)
// lanes (a wave for D > 64) serves one chunk: it sums the runs that start
// there and stores them to out.  The loads of a run do not depend on each
// other: kVsFlight chunks ahead are read before they are added.
__global__ __launch_bounds__(256) void k_vsum_merge(const int64_t *n_keys, uint32_t n, uint32_t D,
                                                    uint64_t P, const double *part,
                                                    const uint32_t *hpk, const uint32_t *tpk,
                                                    double *out) {
    const uint32_t nk = vs_count(n_keys, n);
    const uint32_t nchunks = (nk + kVsChunk - 1u) / kVsChunk;
    uint32_t G = 1;
    while (G < D && G < 64u) G <<= 1;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t ngroups = (uint64_t)gridDim.x * 256u / G;
    const uint32_t dl = (uint32_t)(t % G);
    for (uint64_t c = t / G; c < nchunks; c += ngroups) {
        for (uint32_t which = 0; which < 2u; ++which) {
            const uint32_t k = which ? tpk[c] : hpk[c];
            if (k == kVsNone || (uint64_t)k >= P) continue;
            if (!which && c > 0) {
                const uint32_t tp = tpk[c - 1], hp = hpk[c - 1];
                if ((tp != kVsNone ? tp : hp) == k) continue;  // the run started earlier
            }
            // a head run goes on only if its chunk has no tail (one segment)
            const bool open = which || tpk[c] == kVsNone;
            for (uint32_t d = dl; d < D; d += G) {
                double acc = part[(2u * c + which) * (uint64_t)D + d];
                uint64_t c1 = c + 1;
                bool more = open;
                while (more) {
                    double v[kVsFlight];
                    bool ok[kVsFlight];
#pragma unroll
                    for (uint32_t f = 0; f < kVsFlight; ++f) {
                        ok[f] = more && c1 + f < nchunks && hpk[c1 + f] == k;
                        v[f] = ok[f] ? part[2u * (c1 + f) * (uint64_t)D + d] : 0.0;
                        // the run ends with a chunk that has a tail of its own
                        more = ok[f] && tpk[c1 + f] == kVsNone;
                    }
#pragma unroll
                    for (uint32_t f = 0; f < kVsFlight; ++f)
                        if (ok[f]) acc += v[f];
                    c1 += kVsFlight;
                }
                out[(uint64_t)k * D + d] = acc;
            }
        }
    }
}

struct VcArgs {
    uint32_t D;
    int32_t norm_kind, noise_kind;
    double max_norm, scale;
    int64_t pk_offset, pk_stride;
    uint64_t seed;  // stream seed
};

// Blocks of 256 threads; wave = partition (grid stride).  A lane owns the
// coordinates lane, lane + 64, ...: it reads them all before it writes any,
// so out may be sums.  The norm: per lane left to right over its
// coordinates, then the butterfly over the 64 lanes (m = 1, 2, ..., 32).
__global__ __launch_bounds__(256) void k_vector_clip_noise(const double *sums, uint64_t P, VcArgs a,
                                                           const uint8_t *keep_partition,
                                                           double *out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    const Gran G = gran_of(a.noise_kind == DPG_NOISE_NONE ? 0.0 : a.scale);
    for (uint64_t k = wave; k < P; k += nwaves) {  // wave-uniform
        if (keep_partition && !keep_partition[k]) continue;
        const uint64_t gk = (uint64_t)(a.pk_offset + (int64_t)k * a.pk_stride);
        const double *row = sums + k * (uint64_t)a.D;
        double factor = 1.0;
        if (a.norm_kind != DPG_NORM_LINF) {
            double s = 0.0;
            for (uint32_t d = lane; d < a.D; d += 64u) {
                const double x = row[d];
                s += a.norm_kind == DPG_NORM_L1 ? fabs(x) : x * x;
            }
            for (uint32_t m = 1; m < 64u; m <<= 1) s += vs_shfl_xor(s, m);
            const double norm = a.norm_kind == DPG_NORM_L1 ? s : sqrt(s);
            if (norm > a.max_norm) factor = a.max_norm / norm;  // norm == 0: 1, never 0 / 0
        }
        for (uint32_t d = lane; d < a.D; d += 64u) {
            const double x = row[d];
            const double c = a.norm_kind == DPG_NORM_LINF ? clampd(x, -a.max_norm, a.max_norm)
                                                          : x * factor;
            out[k * (uint64_t)a.D + d] =
                add_noise(a.noise_kind, c, a.scale, G, a.seed, gk, DPG_SLOT_VEC0 + d);
        }
    }
}

}  // namespace dpg
