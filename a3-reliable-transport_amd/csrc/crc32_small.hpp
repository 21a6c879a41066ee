// crc32_small.hpp — the small kernels: k_wire_copy and k_wire_header (the DATA builder's
// three-step path) and k_synth (synthetic payload fill).  A part of the one translation
// unit crc32_kernels.hip; not a header for other units.
#pragma once

namespace wtp {
namespace dev {

// ------------------------------------------------------------------------------------
// 3. fused DATA packet builder
// ------------------------------------------------------------------------------------
// Stage A: copy chunk i into its wire slot after a 16-B header hole; CRC computed on
// the payload with the general kernel, then stage B writes the big-endian header.
__global__ void k_wire_copy(const uint8_t *__restrict__ src, uint64_t total, uint8_t *__restrict__ wire,
                            uint64_t wstride, uint64_t nchunks) {
    const uint64_t per = WTP_MAX_PAYLOAD;
    for (uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;; t += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t i = t / (per / 4 + 1);  // 364 dwords + 1 header slot per chunk
        if (i >= nchunks) break;
        const uint64_t w = t % (per / 4 + 1);
        if (w == per / 4) continue;
        const uint64_t so = i * per + w * 4;
        uint8_t *dst = wire + i * wstride + 16 + w * 4;
        if (so + 4 <= total) {
            uint32_t v;
            memcpy(&v, src + so, 4);
            memcpy(dst, &v, 4);
        } else {
            for (uint64_t b = so; b < total && b < so + 4; ++b) dst[b - so] = src[b];
        }
    }
}
// crc and wlen may be the same buffer (the CRCs are staged in d_wire_len, then become the
// lengths): neither is __restrict__, so each thread's crc[i] load stays ahead of its
// wlen[i] store.
__global__ void k_wire_header(const uint32_t *crc, uint64_t total, uint32_t seq0, uint8_t *__restrict__ wire,
                              uint64_t wstride, uint32_t *wlen, uint64_t nchunks) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nchunks;
         i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t rem = total - i * WTP_MAX_PAYLOAD;
        const uint32_t len = uint32_t(rem < WTP_MAX_PAYLOAD ? rem : WTP_MAX_PAYLOAD);
        const uint32_t hdr[4] = {bswap32(WTP_TYPE_DATA), bswap32(seq0 + uint32_t(i)), bswap32(len), bswap32(crc[i])};
        memcpy(wire + i * wstride, hdr, 16);
        if (wlen) wlen[i] = 16 + len;
    }
}

// ------------------------------------------------------------------------------------
// 4. synthetic payload fill
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ void k_synth(uint8_t *__restrict__ out, uint64_t start, uint64_t nbytes, uint64_t seed) {
    const uint64_t w0 = start >> 3, w1 = (start + nbytes + 7) >> 3;
    for (uint64_t w = w0 + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; w < w1;
         w += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t z = mix64(seed + (w + 1) * 0x9E3779B97F4A7C15ull);
        const uint64_t g0 = w << 3;
        if (g0 >= start && g0 + 8 <= start + nbytes && ((reinterpret_cast<uintptr_t>(out + (g0 - start)) & 7u) == 0)) {
            *reinterpret_cast<uint64_t *>(out + (g0 - start)) = z;
        } else {
            for (uint32_t b = 0; b < 8; ++b) {
                const uint64_t g = g0 + b;
                if (g >= start && g < start + nbytes) out[g - start] = uint8_t(z >> (8 * b));
            }
        }
    }
}

}  // namespace dev
}  // namespace wtp
