// dpg_quantile.h -- DP quantile tree per partition (gfx950).
//
// Replaces the reference's QuantileCombiner (pipeline_dp/combiners.py:532-611,
// PyDP QuantileTree): a 16-ary tree of height 4 over [lo, hi] (65536 leaves)
// whose node counts get keyed additive noise, walked once per quantile.
//
// The tree is never materialised.  dpg_quantile_keys writes one key
// pk << 16 | leaf per kept, non-NaN record and sorts the keys (dpg_rsort.h);
// the count of any node of any partition is then the distance between two
// lower bounds in the sorted keys.  k_quantile_walk serves one partition per
// wave at a time: 64 lanes = 4 quantile slots (DPP rows) x 16 children.  Per
// level a lane finds its child's first key inside the parent's key range
// (which shrinks every level), takes the next child's boundary by a DPP row
// shift (the 17th boundary is the parent's end), adds the node's noise --
// a pure function of (stream seed, partition, node): Philox slot
// DPG_SLOT_QNODE0 + node -- clamps at 0, and the row applies Google's walk:
// drop children below alpha of the row total, pick the first child whose
// inclusive share reaches the rank (row scan by DPP row_shr 1/2/4/8, ballot
// masked to the row), rescale the rank and descend.  No LDS.
#pragma once

#include "dpg_common.h"

namespace dpg {

constexpr uint32_t kQtHeight = 4, kQtBranch = 16, kQtLeaves = 65536;
constexpr double kQtAlpha = 0.0075, kQtTol = 1e-6;

struct QtArgs {
    double lo, hi;
    int32_t noise_kind;
    int32_t nq;
    double scale;
    double q[16];
    int64_t pk_offset, pk_stride;
    uint64_t seed;  // stream seed
};

__device__ __forceinline__ uint32_t qt_leaf(double v, double lo, double hi) {
    if (!(hi > lo)) return 0u;
    const double c = clampd(v, lo, hi);
    const double x = floor((c - lo) * (double)kQtLeaves / (hi - lo));
    return x >= (double)(kQtLeaves - 1) ? kQtLeaves - 1 : (uint32_t)x;
}

// keys[*n_keys ...] = pk << 16 | leaf of every kept, non-NaN record, in any
// order (equal keys are indistinguishable and the keys are sorted next);
// *n_keys is zeroed by the caller.  A workgroup takes kQkPer * 256 records at
// a time and reserves their places with one atomic.
constexpr uint32_t kQkPer = 8;
__global__ __launch_bounds__(256) void k_quantile_keys(const int64_t *pk, const double *value,
                                                       const uint8_t *keep, uint32_t n, uint64_t P,
                                                       double lo, double hi, uint64_t *keys,
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
                const double v = value[i];
                const int64_t k = pk[i];
                if (v == v && (uint64_t)k < P) {
                    take[r] = true;
                    key[r] = ((uint64_t)k << 16) | qt_leaf(v, lo, hi);
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

// First position in [a, b) whose key is >= x.
__device__ __forceinline__ uint32_t qt_lower_bound(const uint64_t *keys, uint32_t a, uint32_t b,
                                                   uint64_t x) {
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (keys[m] < x) a = m + 1;
        else b = m;
    }
    return a;
}

template <int kCtrl>
__device__ __forceinline__ double qt_row_shr(double x) {  // lane i <- lane i - k of its row, else 0
    const long long u = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, kCtrl, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)u >> 32), kCtrl, 0xf,
                                               0xf, true);
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

// Inclusive sum over the lanes 0..i of a row of 16 (all lanes active).
__device__ __forceinline__ double qt_row_scan(double x) {
    x += qt_row_shr<0x111>(x);
    x += qt_row_shr<0x112>(x);
    x += qt_row_shr<0x114>(x);
    x += qt_row_shr<0x118>(x);
    return x;
}

__device__ __forceinline__ double qt_shfl(double x, int src) {
    const long long u = __double_as_longlong(x);
    const int lo = __shfl((int)(uint32_t)u, src);
    const int hi = __shfl((int)(uint32_t)((uint64_t)u >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo));
}

// Blocks of 256 threads; wave = partition (grid stride), row = quantile slot.
__global__ __launch_bounds__(256) void k_quantile_walk(const uint64_t *keys,
                                                       const unsigned long long *n_keys_dev,
                                                       uint64_t P, QtArgs a,
                                                       const uint8_t *keep_partition,
                                                       double *out) {
    const uint32_t lane = threadIdx.x & 63u, row = lane >> 4, child = lane & 15u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    const unsigned long long nk64 = *n_keys_dev;
    const uint32_t nk = nk64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)nk64;
    const Gran G = gran_of(a.noise_kind == DPG_NOISE_NONE ? 0.0 : a.scale);
    const double w = (a.hi - a.lo) / (double)kQtLeaves;
    for (uint64_t k = wave; k < P; k += nwaves) {  // wave-uniform
        if (keep_partition && !keep_partition[k]) continue;
        const uint64_t gk = (uint64_t)(a.pk_offset + (int64_t)k * a.pk_stride);
        const uint32_t p_lo = qt_lower_bound(keys, 0u, nk, k << 16);
        const uint32_t p_hi = qt_lower_bound(keys, p_lo, nk, (k + 1) << 16);
        for (int q0 = 0; q0 < a.nq; q0 += 4) {  // wave-uniform
            const int qi = q0 + (int)row;
            const bool live = qi < a.nq;
            double rank = live ? a.q[qi] : 0.0;
            // the current node: level, index within the level, key positions
            uint32_t level = 0, node = 0, n_lo = p_lo, n_hi = p_hi;
            bool done = false;
#pragma unroll 1
            for (uint32_t l = 1; l <= kQtHeight; ++l) {
                const uint32_t span = 1u << (4u * (kQtHeight - l));  // leaves of a child
                const uint32_t cj = node * kQtBranch + child;        // child's index in level l
                const uint32_t b0 =
                    qt_lower_bound(keys, n_lo, n_hi, (k << 16) | ((uint64_t)cj * span));
                // the next child's boundary; the 17th is the parent's end
                const uint32_t b1 = (uint32_t)__builtin_amdgcn_update_dpp(
                    (int)n_hi, (int)b0, 0x101 /* row_shl:1 */, 0xf, 0xf, false);
                const uint32_t nu = ((1u << (4u * l)) - 1u) / (kQtBranch - 1u) + cj;
                const double noised = add_noise(a.noise_kind, (double)(b1 - b0), a.scale, G,
                                                a.seed, gk, DPG_SLOT_QNODE0 + nu);
                const double c = noised > 0.0 ? noised : 0.0;
                const int last = (int)(lane | 15u);
                const double T = qt_shfl(qt_row_scan(c), last);
                const double cf = c >= kQtAlpha * T ? c : 0.0;
                const double S = qt_row_scan(cf);
                const double Tf = qt_shfl(S, last);
                const bool stop = done || !(Tf > 0.0);
                const bool hit = S / Tf >= rank - kQtTol;
                const uint32_t m = (uint32_t)(__ballot(hit) >> (row * 16u)) & 0xFFFFu;
                const uint32_t pick = m ? (uint32_t)__ffs((int)m) - 1u : kQtBranch - 1u;
                const int src = (int)((lane & 48u) | pick);
                const double c_i = qt_shfl(cf, src), S_i = qt_shfl(S, src);
                const uint32_t s_lo = (uint32_t)__shfl((int)b0, src);
                const uint32_t s_hi = (uint32_t)__shfl((int)b1, src);
                if (!stop) {
                    double r = c_i > 0.0 ? (rank - (S_i - c_i) / Tf) / (c_i / Tf) : 0.0;
                    rank = r < 0.0 ? 0.0 : (r > 1.0 ? 1.0 : r);
                    level = l;
                    node = node * kQtBranch + pick;
                    n_lo = s_lo;
                    n_hi = s_hi;
                }
                done = stop;
            }
            if (live && child == 0) {
                const uint32_t span = 1u << (4u * (kQtHeight - level));
                const double left = a.lo + (double)((uint64_t)node * span) * w;
                const double right = a.lo + (double)((uint64_t)(node + 1u) * span) * w;
                out[k * (uint64_t)a.nq + (uint64_t)qi] = (1.0 - rank) * left + rank * right;
            }
        }
    }
}

}  // namespace dpg
