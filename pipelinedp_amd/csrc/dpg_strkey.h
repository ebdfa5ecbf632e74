// dpg_strkey.h -- string columns to 64-bit keys, and the check that no two
// different strings share one (gfx950).
//
// A string column is Arrow's variable-width layout: record i is the bytes
// data[offsets[i], offsets[i + 1]).  Three kernels reduce it to what the key
// dictionary (dpg_keydict.h) takes:
//
//   k_string_hash        record -> 64-bit key (the definition is in dpg.h)
//   k_keydict_reps       slot -> the smallest record index that landed in it
//   k_string_verify      record's bytes == its slot's representative's bytes?
//
// The table only sees the keys, so two different strings with one key would
// share a slot and a partition.  After the verify pass every record of a slot
// is byte-equal to one record of that slot, hence to every other: equal slot
// <=> equal string, whatever the hash did.  A mismatch is counted and the
// caller raises; nothing is repaired here.
//
// Shape: one lane per string, a loop over its 8-byte words.  Keys of 8-24
// bytes are one to three loads per lane; the lanes of a wave read neighbouring
// strings, so a wave's loads fall into a few consecutive cache lines.  Strings
// start at any byte, so a word is read with an unaligned 8-byte load (gfx950
// global loads take any address).  No load leaves the string it belongs to:
// whole words lie inside it by construction, and the tail of a string of 8 or
// more bytes is the LAST 8 bytes of the string shifted down (they overlap the
// previous word, never the neighbour); only strings shorter than 8 bytes are
// read bytewise.  So nothing outside data[0, data_len) is touched once the
// offsets have passed 0 <= start <= end <= data_len, and a record that fails
// this reads nothing at all.  A string of thousands of bytes keeps one lane
// busy while its wave waits: a wave-cooperative path for long strings is not
// built.
//
// rep[] only falls (atomicMin), so k_keydict_reps reads it with a plain load
// first: a stale line -- a CU's L1 is not refreshed by other CUs' stores and
// the XCDs' L2s are not coherent -- can only show a LARGER value than the true
// one, never a smaller.  A lane that sees a value <= its index is done without
// an atomic (every record of a hot key but the first few per CU); any other
// goes to the device-scope atomicMin, which is decided at the true value.  The
// same argument as the table's plain-load-first probe.
#pragma once

#include "dpg_common.h"
#include "dpg_keydict.h"

namespace dpg {

constexpr uint64_t kStrLenMul = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t str_load8(const uint8_t *p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

// The last, partial word of a string of `len` bytes at p (rem = len & 7 > 0),
// little-endian, zero above its rem bytes.
__device__ __forceinline__ uint64_t str_tail(const uint8_t *p, uint64_t len, uint32_t rem) {
    if (len >= 8) return str_load8(p + len - 8) >> (8u * (8u - rem));
    uint64_t w = 0;
    for (uint32_t b = 0; b < rem; ++b) w |= (uint64_t)p[b] << (8u * b);
    return w;
}

__device__ __forceinline__ bool str_range_ok(int64_t start, int64_t end, int64_t data_len) {
    return start >= 0 && start <= end && end <= data_len;
}

__global__ __launch_bounds__(kKdThreads) void k_string_hash(const int64_t *offsets,
                                                            const uint8_t *data, int64_t data_len,
                                                            uint32_t n, uint64_t seed,
                                                            uint64_t *out_keys,
                                                            unsigned long long *info) {
    uint32_t invalid = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    // i stays below n + stride < 2^32: n < 2^31 and the grid has fewer threads
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const int64_t start = offsets[i], end = offsets[i + 1];
        if (!str_range_ok(start, end, data_len)) {
            ++invalid;
            out_keys[i] = 0;
            continue;
        }
        const uint64_t len = (uint64_t)(end - start);
        const uint8_t *p = data + start;
        uint64_t h = fmix64(seed ^ (len * kStrLenMul));
        const uint64_t words = len >> 3;
        for (uint64_t w = 0; w < words; ++w) h = fmix64(h ^ str_load8(p + 8 * w));
        const uint32_t rem = (uint32_t)len & 7u;
        if (rem) h = fmix64(h ^ str_tail(p, len, rem));
        out_keys[i] = h == kKdEmpty ? (kKdEmpty ^ 1ull) : h;
    }
    kd_wave_add(info, invalid);
}

__global__ __launch_bounds__(kKdThreads) void k_keydict_reps(const uint32_t *rec_slots,
                                                             uint32_t n, uint32_t mask,
                                                             uint32_t *rep) {
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint32_t s = rec_slots[i];
        if (s > mask) continue;  // kKdNoSlot, or anything else that is not a slot
        if (rep[s] > i) atomicMin(rep + s, i);
    }
}

// True if the strings [a, a + len) and [b, b + len) hold the same bytes.
__device__ __forceinline__ bool str_equal(const uint8_t *a, const uint8_t *b, uint64_t len) {
    const uint64_t words = len >> 3;
    for (uint64_t w = 0; w < words; ++w)
        if (str_load8(a + 8 * w) != str_load8(b + 8 * w)) return false;
    const uint32_t rem = (uint32_t)len & 7u;
    return !rem || str_tail(a, len, rem) == str_tail(b, len, rem);
}

__global__ __launch_bounds__(kKdThreads) void k_string_verify(
    const int64_t *offsets, const uint8_t *data, int64_t data_len, uint32_t n,
    const uint32_t *rec_slots, const uint32_t *rep, unsigned long long *n_mismatch) {
    uint32_t bad = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint32_t s = rec_slots[i];
        if (s == kKdNoSlot) continue;
        const int64_t start = offsets[i], end = offsets[i + 1];
        if (!str_range_ok(start, end, data_len)) {
            ++bad;
            continue;
        }
        const uint32_t r = rep[s];
        if (r == i) continue;
        if (r >= n) {  // no representative: rep was not built from these slots
            ++bad;
            continue;
        }
        const int64_t rstart = offsets[r], rend = offsets[r + 1];
        if (!str_range_ok(rstart, rend, data_len) || rend - rstart != end - start ||
            !str_equal(data + start, data + rstart, (uint64_t)(end - start)))
            ++bad;
    }
    kd_wave_add(n_mismatch, bad);
}

}  // namespace dpg
