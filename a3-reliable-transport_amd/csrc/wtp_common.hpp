// wtp_common.hpp — what the protocol translation units (PROTO in the Makefile) share: on the
// host the error plumbing, the launch helper, the argument checks and the d_work layout, and
// on the device the header's wire format, the wave reductions, a few one-line helpers, the
// receive window's claim, ACK and slot copy, and the flush kernels' owner searches.
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
#include <type_traits>

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

// Every launch of the protocol units: launches, records `name` for wtp_last_kernel() and
// returns launch_check(name), so after a launch that itself fails the name is that launch's.
// The arguments convert to the kernel's parameter types as they do at a direct call.  Always
// inlined: left to itself the compiler emits one out-of-line copy per kernel signature.
template <class... P>
__attribute__((always_inline)) inline int launch(const char *name, void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st,
                  std::type_identity_t<P>... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
    wtp_set_kernel_(name);
    return launch_check(name);
}

// The layout of a call's d_work: consecutive arrays from the first `align`-byte boundary (4,
// or 16 where a kernel reads 16-B vectors).  A caller's d_work may be 1-B aligned, so a layout
// asks for `align` bytes more than it holds.  With a NULL d_work only bytes() means anything.
// The order of the arrays is the layout's: each must start at a multiple of its element size.
struct Work {
    uintptr_t base;
    size_t align, end = 0;
    Work(void *d_work, size_t a) : base((reinterpret_cast<uintptr_t>(d_work) + a - 1) & ~uintptr_t(a - 1)), align(a) {}
    template <class T>
    T *take(size_t count) {
        T *p = reinterpret_cast<T *>(base + end);
        end += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return align + end; }
};

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

inline int check_work_bytes(size_t work_bytes, size_t need) {
    return work_bytes < need ? fail(WTP_EINVAL, "work_bytes %zu < %zu", work_bytes, need) : WTP_OK;
}
inline int null_arg(const char *name) { return fail(WTP_EINVAL, "null pointer: %s", name); }
// the multi-connection state: flow f owns global slots [f * window, (f + 1) * window)
inline int check_flows(uint32_t nflows, uint32_t window) {
    if (nflows > WTP_RX_MAX_FLOWS) return fail(WTP_EINVAL, "nflows %u > %u", nflows, WTP_RX_MAX_FLOWS);
    if (window > WTP_RX_MAX_WINDOW) return fail(WTP_EINVAL, "window %u > %u", window, WTP_RX_MAX_WINDOW);
    if (uint64_t(nflows) * window > WTP_RX_MAX_FLOW_SLOTS)
        return fail(WTP_EINVAL, "nflows %u * window %u > %u slots", nflows, window, WTP_RX_MAX_FLOW_SLOTS);
    return WTP_OK;
}
// the multi-connection sender state: the same split of one d_acked / d_sent_ms among the flows
inline int check_tx_flows(uint32_t nflows, uint32_t window) {
    if (nflows > WTP_TX_MAX_FLOWS) return fail(WTP_EINVAL, "nflows %u > %u", nflows, WTP_TX_MAX_FLOWS);
    if (window > WTP_TX_MAX_INFLIGHT) return fail(WTP_EINVAL, "window %u > %u", window, WTP_TX_MAX_INFLIGHT);
    if (uint64_t(nflows) * window > WTP_TX_MAX_FLOW_SLOTS)
        return fail(WTP_EINVAL, "nflows %u * window %u > %u slots", nflows, window, WTP_TX_MAX_FLOW_SLOTS);
    return WTP_OK;
}
// [p, p + bytes) and [q, q + bytes) share a byte (bytes > 0)
inline bool overlap(const void *p, const void *q, uint64_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(p), y = reinterpret_cast<uintptr_t>(q);
    return x < y ? y - x < bytes : x - y < bytes;
}

namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // a 16-B load of dword alignment

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

// Orders a wave's LDS stores before its later LDS loads of other lanes' data (and the
// reverse); a wave's DS instructions execute in order, so this binds only the compiler.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Bytes [0, n) of a 16-byte vector as masks of its low and high half.
__device__ __forceinline__ uint64_t below_lo(uint32_t n) { return n >= 8 ? ~uint64_t(0) : (uint64_t(1) << (8 * n)) - 1; }
__device__ __forceinline__ uint64_t below_hi(uint32_t n) {
    return n <= 8 ? 0 : n >= 16 ? ~uint64_t(0) : (uint64_t(1) << (8 * (n - 8))) - 1;
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

// An ACK datagram at slot: htonl{type = 3, seqNum, length = 0, checksum = crc32("") = 0}.
__device__ __forceinline__ void store_ack(uint8_t *slot, uint32_t seq) {
    if ((reinterpret_cast<uintptr_t>(slot) & 15u) == 0) {  // one 16-B store
        *reinterpret_cast<u32x4 *>(slot) = header_be(WTP_TYPE_ACK, seq, 0u, 0u);
    } else {
        // any other alignment: bytes (no access wider than the slot's alignment)
        // the loop stays rolled, or the compiler merges the sixteen stores into one
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (uint32_t b = 0; b < WTP_HEADER_BYTES; ++b) {
            const uint32_t word = b < 4 ? uint32_t(WTP_TYPE_ACK) : b < 8 ? seq : 0u;
            slot[b] = uint8_t(word >> (8 * (3 - b % 4)));
        }
    }
}

// ---- the receive window: slot_len claims, the cumulative ACK, the slot copy ---------------

constexpr uint32_t kClaim = 0x80000000u;  // claim of datagram i = kClaim | i (n < 2^31)
constexpr uint32_t kGroup = 16;           // lanes per slot (or datagram) in the place and advance kernels
constexpr uint32_t kSlotVecs = (WTP_MAX_PAYLOAD / 16 + kGroup - 1) / kGroup;  // a full slot: 91 vectors -> 6 per lane
static_assert(WTP_MAX_PAYLOAD % 16 == 0, "every slot of a 16-B aligned image is 16-B aligned");

// The ACK is kept as seq0 + (lowest EMPTY slot seen so far); "lower" is taken on the slot
// index, i.e. after subtracting seq0, so a window that wraps 2^32 orders correctly.
__device__ __forceinline__ void ack_lower(uint32_t *ack, uint32_t seq0, uint32_t s) {
    uint32_t cur = __hip_atomic_load(ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (s < cur - seq0) {
        const uint32_t seen = atomicCAS(ack, cur, seq0 + s);
        if (seen == cur) break;
        cur = seen;
    }
}

// Lane g of a 16-lane group copies its share of the len <= 1456 payload bytes of one slot.
// vec (both ends 16-B aligned): floor(len / 16) vectors and a tail of one byte per lane.  A
// full slot is 91 vectors, rows 0 .. 4 whole and row 5 lanes 0 .. 10, six per lane with all
// of a lane's loads in flight before its first store; a shorter one (a Zipf record is a
// vector or two per lane) a loop.  Any other alignment: bytes (exact; no access wider than
// the buffers' alignment).  LNT / SNT: the 16-B loads / stores stream (nt).
template <bool LNT, bool SNT>
__device__ __forceinline__ void copy_slot16(const uint8_t *src, uint8_t *dst, uint32_t len, uint32_t g, bool vec) {
    auto ld16 = [](const u32x4 *p) { return LNT ? __builtin_nontemporal_load(p) : *p; };
    auto st16 = [](u32x4 *p, u32x4 v) {
        if (SNT)
            __builtin_nontemporal_store(v, p);
        else
            *p = v;
    };
    if (vec) {
        const u32x4 *vs = reinterpret_cast<const u32x4 *>(src);
        u32x4 *vd = reinterpret_cast<u32x4 *>(dst);
        const uint32_t nvec = len / 16;
        if (len == WTP_MAX_PAYLOAD) {
            u32x4 w[kSlotVecs];
#pragma unroll
            for (uint32_t k = 0; k + 1 < kSlotVecs; ++k) w[k] = ld16(vs + g + k * kGroup);
            const bool last = g + (kSlotVecs - 1) * kGroup < WTP_MAX_PAYLOAD / 16;
            if (last) w[kSlotVecs - 1] = ld16(vs + g + (kSlotVecs - 1) * kGroup);
#pragma unroll
            for (uint32_t k = 0; k + 1 < kSlotVecs; ++k) st16(vd + g + k * kGroup, w[k]);
            if (last) st16(vd + g + (kSlotVecs - 1) * kGroup, w[kSlotVecs - 1]);
        } else {
#pragma clang loop unroll_count(2)
            for (uint32_t v = g; v < nvec; v += kGroup) st16(vd + v, ld16(vs + v));
        }
        const uint32_t b = nvec * 16 + g;  // byte-exact tail: at most 15 bytes, one per lane
        if (b < len) dst[b] = src[b];
    } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
        for (uint32_t b = g; b < len; b += kGroup) dst[b] = src[b];
    }
}

// ---- the flush kernels' search in a monotone prefix-sum array -------------------------------

// The last index in [lo, hi] whose p is <= b (p(lo) <= b is the caller's).
template <class Get>
__device__ __forceinline__ uint32_t owner(Get p, uint32_t lo, uint32_t hi, uint32_t b) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (p(mid) <= b)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// The same over P[0 .. k] by a half-wave at a time: lanes 0 .. 31 look for one byte, lanes 32 ..
// 63 for another, 32 probes per step, so 2^20 entries take four dependent loads and 2^24 five,
// not twenty and more.  All 64 lanes call it; returns the half's answer in each of its lanes.
template <class T>
__device__ __forceinline__ uint32_t owner_wave(const T *__restrict__ P, uint32_t k, T b, uint32_t lane) {
    uint32_t lo = 0, hi = k;
    while (__ballot(lo < hi) != 0) {
        const uint32_t step = max((hi - lo + 31) / 32, 1u);
        const uint32_t idx = lo + ((lane & 31u) + 1) * step;  // <= 2^24 + 2^24 + 32
        const bool le = idx <= hi && P[idx] <= b;             // P is monotone: true in a prefix of the half
        const uint64_t bal = __ballot(le);
        const uint32_t c = __popc(lane < 32 ? uint32_t(bal) : uint32_t(bal >> 32));
        lo += c * step;
        hi = min(hi, lo + step - 1);
    }
    return lo;
}

// The ordered compaction of k_tx_count / k_tx_select and k_ack_mark / k_ack_emit is not
// here: as functions of this header its two halves did not leave those kernels' register
// use and timing within the parent's, so each keeps its own body.  By the same
// rule k_rx_advance and k_rx_advance_flows keep their copies of copy_slot16's text.

}  // namespace dev
}  // namespace wtp
