// The partition sampler's hash of an integer key: the big-endian first 8
// bytes of SHA-1 (FIPS 180-4) over the ASCII decimal repr of the signed key
// ("-" for negatives, no leading zeros; at most 20 characters, so the padded
// message is always one 64-byte block).  hashlib.sha1(repr(k).encode()) is
// the definition; int(hexdigest()[:16], 16) is the value returned here.
//
// Self-contained (no project includes): the device sampler (dpg_sample.h)
// and a stand-alone host program (tests/test_sampler_host.py) compile the
// same function.  Everything is straight-line code over named scalars and a
// 16-word schedule indexed by literals only, so the device keeps it all in
// registers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPG_SHA1_HD __host__ __device__ inline
#else
#define DPG_SHA1_HD inline
#endif

namespace dpg {

DPG_SHA1_HD uint32_t sha1_rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// Words 0 .. 5 of the padded message of `key`: the characters, the 0x80
// terminator right behind them, zeros.  *len: the character count.
DPG_SHA1_HD void sha1_decimal_block(int64_t key, uint32_t m[6], uint32_t *len) {
    const bool neg = key < 0;
    const uint64_t u = neg ? 0ull - (uint64_t)key : (uint64_t)key;
    // three chunks of 8, 8 and 4 decimal digits: one 64-bit division, the
    // digits then come from 32-bit values
    const uint64_t hi = u / 100000000ull;
    uint32_t c0 = (uint32_t)(u - hi * 100000000ull);
    uint32_t c1 = (uint32_t)(hi % 100000000ull);
    uint32_t c2 = (uint32_t)(hi / 100000000ull);
    uint32_t nd = 1;  // decimal digits of u
    uint64_t p = 10;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 1; k < 20; ++k) {
        nd += u >= p;
        p *= 10;  // the product after the last comparison (10^20) wraps, unused
    }
    // the text right-aligned in 24 bytes b[0 .. 23]: the terminator is byte
    // 23, digit i (from the right) byte 22 - i, the sign byte 22 - nd.  Word
    // j holds bytes 4j .. 4j + 3, big-endian.
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0x80u;
#define DPG_SHA1_CHAR(i, chunk, word, shift)                                        \
    {                                                                               \
        const uint32_t d_ = chunk % 10u;                                            \
        chunk /= 10u;                                                               \
        const uint32_t ch_ = (uint32_t)(i) < nd ? 0x30u + d_                        \
                                                : (((uint32_t)(i) == nd && neg) ? 0x2Du : 0u); \
        word |= ch_ << (shift);                                                     \
    }
    DPG_SHA1_CHAR(0, c0, b5, 8)
    DPG_SHA1_CHAR(1, c0, b5, 16)
    DPG_SHA1_CHAR(2, c0, b5, 24)
    DPG_SHA1_CHAR(3, c0, b4, 0)
    DPG_SHA1_CHAR(4, c0, b4, 8)
    DPG_SHA1_CHAR(5, c0, b4, 16)
    DPG_SHA1_CHAR(6, c0, b4, 24)
    DPG_SHA1_CHAR(7, c0, b3, 0)
    DPG_SHA1_CHAR(8, c1, b3, 8)
    DPG_SHA1_CHAR(9, c1, b3, 16)
    DPG_SHA1_CHAR(10, c1, b3, 24)
    DPG_SHA1_CHAR(11, c1, b2, 0)
    DPG_SHA1_CHAR(12, c1, b2, 8)
    DPG_SHA1_CHAR(13, c1, b2, 16)
    DPG_SHA1_CHAR(14, c1, b2, 24)
    DPG_SHA1_CHAR(15, c1, b1, 0)
    DPG_SHA1_CHAR(16, c2, b1, 8)
    DPG_SHA1_CHAR(17, c2, b1, 16)
    DPG_SHA1_CHAR(18, c2, b1, 24)
    DPG_SHA1_CHAR(19, c2, b0, 0)
    // (position 20, a sign in front of 20 digits, cannot occur: |key| <= 2^63
    // has 19 digits)
#undef DPG_SHA1_CHAR
    const uint32_t n = nd + (neg ? 1u : 0u);
    *len = n;
    // left-align: shift the 24 bytes left by 23 - n bytes (3 .. 22), whole
    // words by conditional moves, the rest by a funnel shift
    const uint32_t sh = 23u - n;
    if (sh & 16u) { b0 = b4; b1 = b5; b2 = 0; b3 = 0; b4 = 0; b5 = 0; }
    if (sh & 8u) { b0 = b2; b1 = b3; b2 = b4; b3 = b5; b4 = 0; b5 = 0; }
    if (sh & 4u) { b0 = b1; b1 = b2; b2 = b3; b3 = b4; b4 = b5; b5 = 0; }
    const uint32_t bs = (sh & 3u) * 8u;
    m[0] = (uint32_t)(((((uint64_t)b0) << 32) | b1) << bs >> 32);
    m[1] = (uint32_t)(((((uint64_t)b1) << 32) | b2) << bs >> 32);
    m[2] = (uint32_t)(((((uint64_t)b2) << 32) | b3) << bs >> 32);
    m[3] = (uint32_t)(((((uint64_t)b3) << 32) | b4) << bs >> 32);
    m[4] = (uint32_t)(((((uint64_t)b4) << 32) | b5) << bs >> 32);
    m[5] = (uint32_t)((((uint64_t)b5) << 32) << bs >> 32);
}

// H(key): see the head of this file.
DPG_SHA1_HD uint64_t sha1_key_hash(int64_t key) {
    uint32_t m[6], len;
    sha1_decimal_block(key, m, &len);
    uint32_t w[16] = {m[0], m[1], m[2], m[3], m[4], m[5], 0, 0, 0, 0, 0, 0, 0, 0, 0, len * 8u};
    uint32_t a = 0x67452301u, b = 0xEFCDAB89u, c = 0x98BADCFEu, d = 0x10325476u, e = 0xC3D2E1F0u;
// the schedule in place: word t lives in w[t & 15]
#define DPG_SHA1_W(t)                                                                \
    (w[(t) & 15] = sha1_rol(w[((t) + 13) & 15] ^ w[((t) + 8) & 15] ^ w[((t) + 2) & 15] ^ \
                                w[(t) & 15], 1))
// one round; the caller rotates the roles of a .. e instead of moving them
#define DPG_SHA1_R(v, x, y, z, u, f, k, wt) \
    u += sha1_rol(v, 5) + (f) + (k) + (wt);  \
    x = sha1_rol(x, 30);
#define DPG_SHA1_F0(x, y, z) (((x) & ((y) ^ (z))) ^ (z))
#define DPG_SHA1_F1(x, y, z) ((x) ^ (y) ^ (z))
#define DPG_SHA1_F2(x, y, z) ((((x) | (y)) & (z)) | ((x) & (y)))
#define DPG_SHA1_R0(v, x, y, z, u, t) DPG_SHA1_R(v, x, y, z, u, DPG_SHA1_F0(x, y, z), 0x5A827999u, w[t])
#define DPG_SHA1_R1(v, x, y, z, u, t) DPG_SHA1_R(v, x, y, z, u, DPG_SHA1_F0(x, y, z), 0x5A827999u, DPG_SHA1_W(t))
#define DPG_SHA1_R2(v, x, y, z, u, t) DPG_SHA1_R(v, x, y, z, u, DPG_SHA1_F1(x, y, z), 0x6ED9EBA1u, DPG_SHA1_W(t))
#define DPG_SHA1_R3(v, x, y, z, u, t) DPG_SHA1_R(v, x, y, z, u, DPG_SHA1_F2(x, y, z), 0x8F1BBCDCu, DPG_SHA1_W(t))
#define DPG_SHA1_R4(v, x, y, z, u, t) DPG_SHA1_R(v, x, y, z, u, DPG_SHA1_F1(x, y, z), 0xCA62C1D6u, DPG_SHA1_W(t))
// five rounds bring the roles back to (a, b, c, d, e)
#define DPG_SHA1_5(R, t)      \
    R(a, b, c, d, e, (t))     \
    R(e, a, b, c, d, (t) + 1) \
    R(d, e, a, b, c, (t) + 2) \
    R(c, d, e, a, b, (t) + 3) \
    R(b, c, d, e, a, (t) + 4)
    DPG_SHA1_5(DPG_SHA1_R0, 0)
    DPG_SHA1_5(DPG_SHA1_R0, 5)
    DPG_SHA1_5(DPG_SHA1_R0, 10)
    DPG_SHA1_R0(a, b, c, d, e, 15)
    DPG_SHA1_R1(e, a, b, c, d, 16)
    DPG_SHA1_R1(d, e, a, b, c, 17)
    DPG_SHA1_R1(c, d, e, a, b, 18)
    DPG_SHA1_R1(b, c, d, e, a, 19)
    DPG_SHA1_5(DPG_SHA1_R2, 20)
    DPG_SHA1_5(DPG_SHA1_R2, 25)
    DPG_SHA1_5(DPG_SHA1_R2, 30)
    DPG_SHA1_5(DPG_SHA1_R2, 35)
    DPG_SHA1_5(DPG_SHA1_R3, 40)
    DPG_SHA1_5(DPG_SHA1_R3, 45)
    DPG_SHA1_5(DPG_SHA1_R3, 50)
    DPG_SHA1_5(DPG_SHA1_R3, 55)
    DPG_SHA1_5(DPG_SHA1_R4, 60)
    DPG_SHA1_5(DPG_SHA1_R4, 65)
    DPG_SHA1_5(DPG_SHA1_R4, 70)
    DPG_SHA1_5(DPG_SHA1_R4, 75)
#undef DPG_SHA1_5
#undef DPG_SHA1_R4
#undef DPG_SHA1_R3
#undef DPG_SHA1_R2
#undef DPG_SHA1_R1
#undef DPG_SHA1_R0
#undef DPG_SHA1_F2
#undef DPG_SHA1_F1
#undef DPG_SHA1_F0
#undef DPG_SHA1_R
#undef DPG_SHA1_W
    // the digest's first two words only
    (void)c;
    (void)d;
    (void)e;
    return ((uint64_t)(0x67452301u + a) << 32) | (uint64_t)(0xEFCDAB89u + b);
}

}  // namespace dpg
