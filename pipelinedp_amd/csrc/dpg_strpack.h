// dpg_strpack.h -- strings of a column gathered into a packed column, and the
// check that every run of equal keys holds one string (gfx950).
//
// The global string dictionary (distributed.build_string_dictionary; DESIGN.md
// section 19) moves strings three times -- the representatives to their
// owners, the owners' heads into the owned table, the kept partitions to the
// host -- and compares them once more at the owner, where two ranks' strings
// with one 64-bit key first meet.  Three kernels:
//
//   k_string_lengths      out_len[j] = byte length of record records[j]
//   k_string_pack         out_data[out_offsets[j], out_offsets[j + 1]) = its bytes
//   k_string_verify_runs  head[j] = keys[j] starts a run; a record of a run is
//                         compared with the record before it
//
// After k_string_verify_runs counted no difference every record of a run is
// byte-equal to its predecessor, hence (a chain) to the run's head: equal key
// <=> equal string among the arrivals, the argument of dpg_strkey.h with the
// predecessor in the place of the slot's representative.
//
// Shape, as dpg_strkey.h: one lane per string, a loop over its 8-byte words
// with unaligned loads and stores (gfx950 global accesses take any address).
// The tail of a string of 8 or more bytes is its LAST 8 bytes, moved as one
// word that overlaps the lane's own previous word -- the same bytes written
// twice, never a neighbour's; strings shorter than 8 bytes move bytewise.  So
// no byte outside data[0, data_len) is read and none outside the j's own out
// range is written, whatever the alignment of either buffer, and a j that
// fails a check touches nothing.  The lanes of a wave write neighbouring out
// ranges: with keys of 8-24 bytes a wave's stores fall into a few consecutive
// lines.  A string of thousands of bytes keeps one lane busy while its wave
// waits: a wave-cooperative path for long strings is not built.
#pragma once

#include "dpg_common.h"
#include "dpg_keydict.h"
#include "dpg_strkey.h"

namespace dpg {

__device__ __forceinline__ void str_store8(uint8_t *p, uint64_t w) {
    __builtin_memcpy(p, &w, 8);
}

// Offsets of record r of an n-record column, checked: false reads nothing
// past the two offsets.
__device__ __forceinline__ bool str_record(const int64_t *offsets, int64_t data_len, int64_t n,
                                           int64_t r, int64_t &start, int64_t &end) {
    if (r < 0 || r >= n) return false;
    start = offsets[r];
    end = offsets[r + 1];
    return str_range_ok(start, end, data_len);
}

__global__ __launch_bounds__(kKdThreads) void k_string_lengths(const int64_t *offsets,
                                                               int64_t data_len, int64_t n,
                                                               const int64_t *records, uint32_t m,
                                                               int64_t *out_len,
                                                               unsigned long long *info) {
    uint32_t invalid = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    // j stays below m + stride < 2^32: m < 2^31 and the grid has fewer threads
    for (uint32_t j = blockIdx.x * kKdThreads + threadIdx.x; j < m; j += stride) {
        int64_t start, end;
        if (!str_record(offsets, data_len, n, records[j], start, end)) {
            ++invalid;
            out_len[j] = 0;
            continue;
        }
        out_len[j] = end - start;
    }
    kd_wave_add(info, invalid);
}

__global__ __launch_bounds__(kKdThreads) void k_string_pack(
    const int64_t *offsets, const uint8_t *data, int64_t data_len, int64_t n,
    const int64_t *records, uint32_t m, const int64_t *out_offsets, uint8_t *out_data,
    int64_t out_total, unsigned long long *info) {
    uint32_t invalid = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t j = blockIdx.x * kKdThreads + threadIdx.x; j < m; j += stride) {
        int64_t start, end;
        const int64_t o0 = out_offsets[j], o1 = out_offsets[j + 1];
        if (!str_record(offsets, data_len, n, records[j], start, end) ||
            !str_range_ok(o0, o1, out_total) || o1 - o0 != end - start) {
            ++invalid;
            continue;
        }
        const uint64_t len = (uint64_t)(end - start);
        const uint8_t *src = data + start;
        uint8_t *dst = out_data + o0;
        if (len < 8) {
            for (uint32_t b = 0; b < (uint32_t)len; ++b) dst[b] = src[b];
            continue;
        }
        const uint64_t words = len >> 3;
        for (uint64_t w = 0; w < words; ++w) str_store8(dst + 8 * w, str_load8(src + 8 * w));
        if (len & 7u) str_store8(dst + len - 8, str_load8(src + len - 8));
    }
    kd_wave_add(info, invalid);
}

__global__ __launch_bounds__(kKdThreads) void k_string_verify_runs(
    const uint64_t *keys, const uint32_t *order, const int64_t *offsets, const uint8_t *data,
    int64_t data_len, int64_t n_strings, uint32_t m, uint8_t *head, unsigned long long *info) {
    uint32_t differ = 0, invalid = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t j = blockIdx.x * kKdThreads + threadIdx.x; j < m; j += stride) {
        const bool first = j == 0 || keys[j] != keys[j - 1];
        head[j] = first ? 1 : 0;
        if (first) continue;
        const int64_t a = order ? (int64_t)order[j] : (int64_t)j;
        const int64_t b = order ? (int64_t)order[j - 1] : (int64_t)j - 1;
        int64_t as, ae, bs, be;
        if (!str_record(offsets, data_len, n_strings, a, as, ae) ||
            !str_record(offsets, data_len, n_strings, b, bs, be)) {
            ++differ;
            ++invalid;
            continue;
        }
        if (ae - as != be - bs || !str_equal(data + as, data + bs, (uint64_t)(ae - as))) ++differ;
    }
    kd_wave_add(info, differ);
    kd_wave_add(info + 1, invalid);
}

}  // namespace dpg
