// crc32_combine.hpp — GF(2)[x]/P arithmetic on finished CRC-32 values (zlib's
// crc32_combine semantics), shared by the host fold (wtp_host.cpp) and the device fold
// (wtp_concat.hip).  Generated from the polynomial; nothing is copied from the reference.
//
// A 32-bit word is a polynomial in the reflected order of the CRC register: bit 31 is
// x^0, bit 0 is x^31, so 1 = 0x80000000 and x = 0x40000000.  For finished CRCs (init and
// xorout ~0) the affine parts cancel and
//   crc32(A || B) = crc32(A) * x^(8|B|) mod P  ^  crc32(B).
// x has multiplicative order dividing 2^32 - 1 (x^(8(2^32-1)) = 1, checked in
// tests/test_concat_model.py), so byte counts may be carried mod 2^32 - 1.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define WTP_HD __host__ __device__
#else
#define WTP_HD
#endif

namespace wtp {
namespace gf {

constexpr uint32_t kP = 0xEDB88320u;     // reflected 0x04C11DB7
constexpr uint32_t kOne = 0x80000000u;   // x^0
constexpr uint32_t kOrder = 0xFFFFFFFFu; // x^(8 * kOrder) = 1

// a * b mod P.  With a wave-uniform b the b-chain runs on the scalar unit and a step costs
// three vector instructions.
WTP_HD constexpr uint32_t mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & kP);
    }
    return p;
}

// kPow8[k] = x^(8 * 2^k), k = 0 .. 31
struct Pow8 {
    uint32_t v[32];
    constexpr Pow8() : v{} {
        uint32_t g = kOne >> 8;  // x^8
        for (int k = 0; k < 32; ++k) {
            v[k] = g;
            g = mul(g, g);
        }
    }
};

WTP_HD constexpr uint32_t reduce(uint64_t nbytes) { return uint32_t(nbytes % kOrder); }

// x^(8 * nbytes): square and multiply over the reduced byte count
WTP_HD constexpr uint32_t xpow8(uint64_t nbytes) {
    constexpr Pow8 kPow8{};
    uint32_t e = reduce(nbytes), r = kOne;
    for (int k = 0; e; ++k, e >>= 1)
        if (e & 1u) r = mul(r, kPow8.v[k]);
    return r;
}

WTP_HD constexpr uint32_t combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return mul(crc_a, xpow8(len_b)) ^ crc_b;
}

static_assert(combine(0xE8B7BE43u /* "a" */, 0x71BEEFF9u /* "b" */, 1) == 0x9E83486Du /* "ab" */, "combine");
static_assert(xpow8(kOrder) == kOne && xpow8(0) == kOne && mul(0x12345678u, kOne) == 0x12345678u, "order of x");

}  // namespace gf
}  // namespace wtp
