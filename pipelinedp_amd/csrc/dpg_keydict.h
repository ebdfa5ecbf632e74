// dpg_keydict.h -- write-once hash dictionary of sparse int64 partition keys
// (gfx950).
//
// Several ranks need one global dense id per partition key
// (distributed.build_key_dictionary).  Each rank first reduces its records to
// their distinct keys: one probe per record into an open-addressing table
// that the caller allocates and fills with kKdEmpty, instead of the full sorts
// of the record column that a unique-with-inverse costs.  The same table then
// carries the ids back: the owners' ids are stored beside the keys
// (dpg_keydict_assign) and every record reads its own (dpg_keydict_lookup).
//
//   h     = fmix64(key)                 murmur3's 64-bit finaliser
//   home  = h & (capacity - 1)          linear probing, wrapping around
//   owner = ((h >> 32) * R) >> 32       the high half: independent of the slot
//                                       bits (host side: distributed.key_owner)
//
// A slot is write-once: kKdEmpty -> key by one 64-bit compare-and-swap, never
// anything else afterwards.  So the probe reads the slot with a plain load
// first.  A cache line that is out of date -- a CU's L1 is not refreshed by
// other CUs' stores and the XCDs' L2s are not coherent -- can only still show
// kKdEmpty, never a key that is not there: a lane that reads its own key is
// done without an atomic (every record of a hot key but the first few), a lane
// that reads another key moves on, and a lane that reads kKdEmpty goes to the
// device-scope CAS, whose return value is the slot's true content.  The key
// INT64_MIN has the bit pattern of kKdEmpty: it is reserved, counted and never
// stored.
//
// Wide privacy ids (distributed.encode_privacy_ids) use the same table
// rank-locally and probe it once: dpg_keydict_insert_slots remembers the slot
// every record found -- final, since a key never moves -- and
// dpg_keydict_gather_ids reads slot_ids there.
//
// Every probe loop runs at most `capacity` steps, so a full table ends the
// call (insert counts the record in info[1]); nothing spins.  The other three
// kernels run behind the inserts in stream order and only read the slots.
#pragma once

#include "dpg_common.h"

namespace dpg {

constexpr uint64_t kKdEmpty = 0x8000000000000000ull;
constexpr uint32_t kKdThreads = 256;
constexpr uint32_t kKdNoSlot = 0xFFFFFFFFu;  // capacity <= 2^31: never a slot

// Adds the wave's sum of x to *dst with one atomic (all lanes active).
__device__ __forceinline__ void kd_wave_add(unsigned long long *dst, uint32_t x) {
    uint32_t total;
    wave_excl_scan(x, total);
    if ((threadIdx.x & 63u) == 0 && total) atomicAdd(dst, (unsigned long long)total);
}

// Slot of `key` (not kKdEmpty) in a table no kernel is writing, or capacity:
// the chain ends at the first empty slot or after `capacity` steps.
__device__ __forceinline__ uint32_t kd_find(const uint64_t *slots, uint32_t mask, uint64_t key) {
    uint32_t s = (uint32_t)fmix64(key) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {
        const uint64_t cur = slots[s];
        if (cur == key) return s;
        if (cur == kKdEmpty) break;
        s = (s + 1u) & mask;
    }
    return mask + 1u;
}

// One record per lane and trip; consecutive lanes load consecutive keys.
__global__ __launch_bounds__(kKdThreads) void k_keydict_insert(const uint64_t *keys, uint32_t n,
                                                               uint64_t *slots, uint32_t mask,
                                                               unsigned long long *info) {
    uint32_t reserved = 0, lost = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    // i stays below n + stride < 2^32: n < 2^31 and the grid has fewer threads
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        if (key == kKdEmpty) {
            ++reserved;
            continue;
        }
        uint32_t s = (uint32_t)fmix64(key) & mask;
        bool placed = false;
        for (uint32_t step = 0; step <= mask; ++step) {
            uint64_t cur = slots[s];
            if (cur == kKdEmpty)
                cur = atomicCAS(reinterpret_cast<unsigned long long *>(slots + s),
                                (unsigned long long)kKdEmpty, (unsigned long long)key);
            if (cur == key || cur == kKdEmpty) {
                placed = true;
                break;
            }
            s = (s + 1u) & mask;
        }
        lost += placed ? 0u : 1u;
    }
    kd_wave_add(info, reserved);
    kd_wave_add(info + 1, lost);
}

// k_keydict_insert that also remembers where every record ended up.  A slot is
// write-once and a key never moves, so the slot a record finds here is final:
// out_slots[i] stands for the key from now on, and k_keydict_gather_ids turns
// it into an id without reading the key column or walking a chain again.  A
// reserved or lost record stores kKdNoSlot.
__global__ __launch_bounds__(kKdThreads) void k_keydict_insert_slots(
    const uint64_t *keys, uint32_t n, uint64_t *slots, uint32_t mask, uint32_t *out_slots,
    unsigned long long *info) {
    uint32_t reserved = 0, lost = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    // i stays below n + stride < 2^32: n < 2^31 and the grid has fewer threads
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        if (key == kKdEmpty) {
            ++reserved;
            out_slots[i] = kKdNoSlot;
            continue;
        }
        uint32_t s = (uint32_t)fmix64(key) & mask;
        bool placed = false;
        for (uint32_t step = 0; step <= mask; ++step) {
            uint64_t cur = slots[s];
            if (cur == kKdEmpty)
                cur = atomicCAS(reinterpret_cast<unsigned long long *>(slots + s),
                                (unsigned long long)kKdEmpty, (unsigned long long)key);
            if (cur == key || cur == kKdEmpty) {
                placed = true;
                break;
            }
            s = (s + 1u) & mask;
        }
        out_slots[i] = placed ? s : kKdNoSlot;
        lost += placed ? 0u : 1u;
    }
    kd_wave_add(info, reserved);
    kd_wave_add(info + 1, lost);
}

// out_ids[i] = slot_ids[out_slots[i]]: 4 bytes in, 8 out and one 4-byte gather
// per record.  Four records per lane and trip, their gathers in flight
// together; anything that is not a slot (kKdNoSlot) gives -1 and is counted.
constexpr uint32_t kKdGather = 4;
__global__ __launch_bounds__(kKdThreads) void k_keydict_gather_ids(
    const uint32_t *out_slots, uint32_t n, const uint32_t *slot_ids, uint32_t mask,
    int64_t *out_ids, unsigned long long *n_missing) {
    uint32_t missing = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    // i0 + 3 * stride stays below n + 7 * stride < 2^32: n < 2^31, stride < 2^27
    for (uint32_t i0 = blockIdx.x * kKdThreads + threadIdx.x; i0 < n; i0 += kKdGather * stride) {
        uint32_t s[kKdGather], id[kKdGather];
#pragma unroll
        for (uint32_t k = 0; k < kKdGather; ++k)
            s[k] = i0 + k * stride < n ? out_slots[i0 + k * stride] : kKdNoSlot;
#pragma unroll
        for (uint32_t k = 0; k < kKdGather; ++k) id[k] = s[k] <= mask ? slot_ids[s[k]] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kKdGather; ++k) {
            if (i0 + k * stride >= n) continue;
            out_ids[i0 + k * stride] = s[k] <= mask ? (int64_t)id[k] : -1;
            missing += s[k] <= mask ? 0u : 1u;
        }
    }
    kd_wave_add(n_missing, missing);
}

// Compaction of the occupied slots: a wave reserves one run of out_keys for
// its occupied slots (one atomic per wave and trip), so the order depends on
// the arrival of the waves.
__global__ __launch_bounds__(kKdThreads) void k_keydict_keys(const uint64_t *slots,
                                                             uint32_t capacity,
                                                             uint64_t *out_keys,
                                                             unsigned long long *n_keys) {
    const uint32_t stride = gridDim.x * kKdThreads;
    // capacity is a multiple of 64: a wave's lanes enter and leave together
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < capacity; i += stride) {
        const uint64_t cur = slots[i];
        const uint32_t occ = cur != kKdEmpty ? 1u : 0u;
        uint32_t total;
        const uint32_t ex = wave_excl_scan(occ, total);
        unsigned long long base = 0;
        if ((threadIdx.x & 63u) == 0 && total) base = atomicAdd(n_keys, (unsigned long long)total);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        if (occ) out_keys[lo + ex] = cur;  // lo + ex < occupied slots <= capacity < 2^32
    }
}

__global__ __launch_bounds__(kKdThreads) void k_keydict_assign(const uint64_t *keys,
                                                               const int64_t *ids, uint32_t n,
                                                               const uint64_t *slots,
                                                               uint32_t *slot_ids, uint32_t mask,
                                                               unsigned long long *n_missing) {
    uint32_t missing = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        const uint32_t s = key == kKdEmpty ? mask + 1u : kd_find(slots, mask, key);
        if (s <= mask)
            slot_ids[s] = (uint32_t)ids[i];
        else
            ++missing;
    }
    kd_wave_add(n_missing, missing);
}

__global__ __launch_bounds__(kKdThreads) void k_keydict_lookup(const uint64_t *keys, uint32_t n,
                                                               const uint64_t *slots,
                                                               const uint32_t *slot_ids,
                                                               uint32_t mask, int64_t *out_ids,
                                                               unsigned long long *n_missing) {
    uint32_t missing = 0;
    const uint32_t stride = gridDim.x * kKdThreads;
    for (uint32_t i = blockIdx.x * kKdThreads + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        const uint32_t s = key == kKdEmpty ? mask + 1u : kd_find(slots, mask, key);
        out_ids[i] = s <= mask ? (int64_t)slot_ids[s] : -1;
        missing += s <= mask ? 0u : 1u;
    }
    kd_wave_add(n_missing, missing);
}

}  // namespace dpg
