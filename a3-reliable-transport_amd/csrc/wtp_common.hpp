// wtp_common.hpp — what the protocol translation units (wtp_accept.hip, wtp_concat.hip,
// wtp_tx.hip, wtp_txvar.hip, wtp_ack.hip, wtp_buildvar.hip, wtp_deliver.hip, wtp_advance.hip, wtp_flows.hip, wtp_flows_flush.hip) share: error plumbing and argument checks on the host, and on
// the device the header's wire format and the wave reductions.
// Internal: the C-ABI is include/wtp_crc32.h.
//
// Each protocol call is a separate translation unit: k_fixed_braid and everything it
// inlines stay as they are (tests/test_bench.py pins the headline kernel's machine code),
// so crc32_kernels.hip does not include this header and nothing here is shared with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "wtp_crc32.h"

// Defined in crc32_kernels.hip: the per-thread state behind wtp_last_error() / wtp_last_kernel().
extern "C" int wtp_set_error_(int code, const char *msg);
extern "C" void wtp_set_kernel_(const char *name);

namespace wtp {

inline int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return wtp_set_error_(code, buf);
}

inline int launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WTP_EHIP, "launch %s: %s", what, hipGetErrorString(e));
    return WTP_OK;
}

// A caller's d_work may be 1-B aligned: its words start at the first 4-B boundary, and a
// layout asks for kWorkSlack bytes more than it holds.
constexpr size_t kWorkSlack = 4;
inline uint8_t *align4(void *d_work) {
    return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(d_work) + 3) & ~uintptr_t(3));
}

// The checks of a datagram ring's arguments.  Each is its own call because the entry points
// interleave them with their own checks, and which message two bad arguments give is part
// of the C-ABI.
inline int check_batch(size_t n) {  // a claim is 0x80000000 | index
    return n >= (size_t(1) << 31) ? fail(WTP_EINVAL, "n %zu >= 2^31", n) : WTP_OK;
}
inline int check_mode(uint32_t mode) {
    return mode != WTP_ACK_SELECTIVE && mode != WTP_ACK_CUMULATIVE ? fail(WTP_EINVAL, "unknown mode %u", mode) : WTP_OK;
}
inline int check_stride(size_t stride) {
    return stride < WTP_HEADER_BYTES ? fail(WTP_EINVAL, "stride %zu < 16", stride) : WTP_OK;
}
// n > 0: the ring, its lengths and verdicts are there (other_null: a further pointer the call
// cannot do without is not), and a slot holds a header
inline int check_ring(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, const uint8_t *d_ok,
                      bool other_null = false) {
    if (!d_dgrams || !d_recv_len || !d_ok || other_null) return fail(WTP_EINVAL, "null pointer");
    return check_stride(stride);
}

namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t be32(const uint8_t *p) {
    return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, uint32_t(__shfl_xor(v, d, 64)));
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, uint32_t(__shfl_xor(v, d, 64)));
    return v;
}

// ---- the 16-byte header: htonl{type, seqNum, length, checksum} ---------------------------

struct Header {
    uint32_t type, seq, len, sum;
};

// The header at h.  A 4-B aligned slot takes dword loads, any other alignment bytes (no
// access wider than the slot's alignment); a field the caller does not use is not loaded.
__device__ __forceinline__ Header load_header(const uint8_t *h) {
    if ((reinterpret_cast<uintptr_t>(h) & 3u) == 0) {
        const uint32_t *hw = reinterpret_cast<const uint32_t *>(h);
        return {__builtin_bswap32(hw[0]), __builtin_bswap32(hw[1]), __builtin_bswap32(hw[2]), __builtin_bswap32(hw[3])};
    }
    return {be32(h), be32(h + 4), be32(h + 8), be32(h + 12)};
}

// The header as one 16-B store's worth of big-endian fields.
__device__ __forceinline__ u32x4 header_be(uint32_t type, uint32_t seq, uint32_t len, uint32_t sum) {
    u32x4 hv;
    hv.x = __builtin_bswap32(type);
    hv.y = __builtin_bswap32(seq);
    hv.z = __builtin_bswap32(len);
    hv.w = __builtin_bswap32(sum);
    return hv;
}

// The ordered compaction of k_tx_count / k_tx_select and k_ack_mark / k_ack_emit is not
// here: as functions of this header its two halves did not leave those kernels' register
// use and timing within the parent's, so each keeps its own body.

}  // namespace dev
}  // namespace wtp
