// wtp_crc_dev.hpp — what the DATA builders (wtp_tx.hip, wtp_buildvar.hip, wtp_txvar.hip, wtp_tx_flows.hip) share
// on the device: the slice-by-4 table's type and the byte helpers around a 16-B vector.  Each
// unit defines its own table object and keeps its kernel bodies.  Internal.
#pragma once
#include "crc32_math.hpp"
#include "wtp_common.hpp"

namespace wtp {
namespace dev {

// Slice-by-4 tables built at compile time for the device: t[0] is the byte table of
// crc32_math.hpp's Sarwate, t[k][b] = the register after byte b and k zero bytes.
struct SliceTable {
    uint32_t t[4][256];
    constexpr SliceTable() : t{} {
        for (uint32_t b = 0; b < 256; ++b) {
            uint32_t c = b;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : (c >> 1);
            t[0][b] = c;
        }
        for (int k = 1; k < 4; ++k)
            for (uint32_t b = 0; b < 256; ++b) t[k][b] = (t[k - 1][b] >> 8) ^ t[0][t[k - 1][b] & 0xFFu];
    }
};

// tab: a SliceTable's 1024 words (in LDS)
__device__ __forceinline__ uint32_t crc_word(const uint32_t *tab, uint32_t c, uint32_t w) {
    c ^= w;
    return tab[768 + (c & 0xFFu)] ^ tab[512 + ((c >> 8) & 0xFFu)] ^ tab[256 + ((c >> 16) & 0xFFu)] ^ tab[c >> 24];
}

// The register after bytes [0, nb) of v (little-endian byte order, nb <= 16) from c.
__device__ __forceinline__ uint32_t crc_vec(const uint32_t *tab, uint32_t c, u32x4 v, uint32_t nb) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        if (nb >= 4 * r + 4) {
            c = crc_word(tab, c, w[r]);
        } else if (nb > 4 * r) {
#pragma unroll
            for (uint32_t q = 0; q < 3; ++q)
                if (4 * r + q < nb) c = tab[(c ^ (w[r] >> (8 * q))) & 0xFFu] ^ (c >> 8);
        }
    }
    return c;
}

// Bytes [from, nb) of v to d, one by one.
__device__ __forceinline__ void store_bytes(uint8_t *d, u32x4 v, uint32_t from, uint32_t nb) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b >= from && b < nb) d[b] = uint8_t(w[b / 4] >> (8 * (b % 4)));
}

// Bytes [0, nb) of v to d, nb <= 16.  vec: d is 16-B aligned.
__device__ __forceinline__ void store_vec(uint8_t *d, u32x4 v, uint32_t nb, bool vec) {
    if (vec && nb == 16) {
        *reinterpret_cast<u32x4 *>(d) = v;
    } else if (vec) {
        uint32_t *dw = reinterpret_cast<uint32_t *>(d);
        if (nb >= 4) dw[0] = v.x;
        if (nb >= 8) dw[1] = v.y;
        if (nb >= 12) dw[2] = v.z;
        store_bytes(d, v, nb & ~3u, nb);
    } else {
        store_bytes(d, v, 0, nb);
    }
}

// Payload bytes [src, src + nb), nb <= 16, as a vector, loaded one by one.
__device__ __forceinline__ u32x4 load_bytes(const uint8_t *src, uint32_t nb) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b < nb) w[b / 4] |= uint32_t(src[b]) << (8 * (b % 4));
    u32x4 v;
    v.x = w[0];
    v.y = w[1];
    v.z = w[2];
    v.w = w[3];
    return v;
}

}  // namespace dev
}  // namespace wtp
