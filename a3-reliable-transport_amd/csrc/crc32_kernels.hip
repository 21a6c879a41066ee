// crc32_kernels.hip — CDNA4 (gfx950) kernels for WTP's per-packet CRC-32.
//
// Reference path being replaced (mmheyer/a3-reliable-transport):
//   crc32()  cpp/src/common/Crc32.hpp:91-102 — byte-at-a-time Sarwate loop, one call
//            per DATA payload (Packet.cpp:13 sender build, Receiver.cpp:204 verify).
//
// Two kernel families, both HBM-read-bound integer work (no MFMA):
//
// 1. k_fixed_braid<ROWS> — equal-length payloads whose ends are 16-B aligned (the
//    1456-B DATA chunk case, the receiver's 1472-B ring, the fused packet builder).
//    16 lanes per packet, 4 packets per wave.  Each lane owns 4 interleaved "braids"
//    (CRC streams over every 64th dword of the packet's frame), so the 16 lanes of a
//    packet read 256 contiguous bytes per row with buffer_load_dwordx4 (coalesced, no
//    LDS staging) and every lane carries 4 independent dependency chains.  Per lookup:
//    one v_perm_b32 builds the LDS address and one ds_read_b32 fetches the table word
//    from staggered 8-copy tables (conflict-free whatever the data).  A lane folds its
//    braids in-lane (x^-32 Horner); every 8 rounds a flush combines each packet's 16
//    columns by Horner's rule through an LDS transposition slot.
//
// 2. k_pieces<Prov, Epi> — anything else (mixed lengths, odd strides, unaligned
//    buffers, datagrams that are not full ring slots).  Each packet is cut into pieces of
//    S = 64 bytes counted back from its end (the head piece is shorter); pieces of
//    consecutive packets are packed densely into the 64 lanes of a wave ("wavefront-
//    packed tails"), each lane runs a slice-by-4 chain over its piece, and a segmented
//    inclusive scan with uniform x^(8*64*d) shifts combines the pieces of each packet.
//    Waves get equal piece counts, and rotate their issue priority.
//
// All algebra (tables, operators) is generated on the host in crc32_math.hpp.
//
// This file is one translation unit (tools/kbench.hip and tools/pprobe.hip include it
// whole): the build switches, then the bodies from internal headers in this order, then
// the C-ABI entry points.
//   crc32_dev.hpp     table and LDS layout, shared device helpers
//   crc32_pieces.hpp  k_pieces and the braided verify's fix-up phase
//   crc32_braid.hpp   k_fixed_braid and its epilogues
//   crc32_stream.hpp  k_stream
//   crc32_small.hpp   k_wire_copy, k_wire_header, k_synth
//   crc32_launch.hpp  per-device host state, launchers, metadata providers
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <string>
#include <vector>

#include "crc32_math.hpp"
#include "wtp_crc32.h"

// ------------------------------------------------------------------------------------
// Build switches.  These are instruments, not variants: the product takes each at the
// value below, and only tools/build_ab.sh and tools/Makefile (kbench, pprobe) define
// WTP_AB_BUILD to build with another.  A misconfigured product build is a compile error,
// not a library that runs wrong.  (The A/B switches whose question is settled are gone;
// DESIGN.md names the last commit that has each variant's code.)
// ------------------------------------------------------------------------------------
#ifndef WTP_PROBE  // 1: per-wave phase timestamps (PC_PROBE) for tools/pprobe.hip
#define WTP_PROBE 0
#endif
#ifndef WTP_BR_PROLOGUE_DIAG  // k_fixed_braid, probe builds only: 1 = no table loads, 2 = no table fill at all
#define WTP_BR_PROLOGUE_DIAG 0
#endif
#ifndef WTP_BUILD_DIAG  // DIAG of the fused builder's k_fixed_braid (ablation builds only: wrong CRCs)
#define WTP_BUILD_DIAG 0
#endif
#ifndef WTP_PC_TAILCLAMP  // k_pieces: clamp the last span prefetches (see pieces_loop)
#define WTP_PC_TAILCLAMP 0  // measured and not shipped: -12.1 MB of reads, +1.5 us
#endif
#ifndef WTP_AB_BUILD
static_assert(WTP_PROBE == 0 && WTP_BR_PROLOGUE_DIAG == 0 && WTP_BUILD_DIAG == 0,
              "product build: no probe, prologue ablation or builder ablation");
static_assert(WTP_PC_TAILCLAMP == 0, "product build: the piece kernel's tail clamp is off");
#endif

#include "crc32_dev.hpp"
#include "crc32_pieces.hpp"
#include "crc32_braid.hpp"
#include "crc32_stream.hpp"
#include "crc32_small.hpp"
#include "crc32_launch.hpp"

// ======================================================================================
// C ABI
// ======================================================================================
using namespace wtp;

extern "C" {

const char *wtp_version(void) { return "wtp-crc32-mi355x 0.1 (gfx950)"; }

const char *wtp_last_error(void) { return g_err.c_str(); }
const char *wtp_last_kernel(void) { return g_kernel.c_str(); }

int wtp_set_error_(int code, const char *msg) {
    g_err = msg ? msg : "";
    return code;
}

// wtp_last_kernel() for launchers in other translation units (wtp_accept.hip)
void wtp_set_kernel_(const char *name) { g_kernel = name ? name : ""; }

int wtp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int wtp_init(int device) { return init_device(device); }

int wtp_reserve_cus(int device, int ncus) {
    int rc = init_device(device);
    if (rc) return rc;
    DevState &s = g_dev[device];
    if (ncus < 0 || ncus >= s.cus) return fail(WTP_EINVAL, "ncus %d outside [0, %d)", ncus, s.cus);
    s.reserve.store(ncus, std::memory_order_relaxed);
    return WTP_OK;
}

int wtp_device_status(int device, uint32_t *flags, int clear) {
    if (!flags) return fail(WTP_EINVAL, "flags is null");
    int rc = init_device(device);
    if (rc) return rc;
    int prev = 0;
    WTP_HIP(hipGetDevice(&prev));
    WTP_HIP(hipSetDevice(device));
    auto body = [&]() -> int {
        WTP_HIP(hipDeviceSynchronize());
        WTP_HIP(hipMemcpy(flags, g_dev[device].status, 4, hipMemcpyDeviceToHost));
        if (clear) WTP_HIP(hipMemset(g_dev[device].status, 0, 4));
        return WTP_OK;
    };
    rc = body();
    (void)hipSetDevice(prev);  // restored on failure too
    return rc;
}

uint32_t wtp_crc32(const void *buf, size_t size) {
    return raw_update(0xFFFFFFFFu, static_cast<const uint8_t *>(buf), size) ^ 0xFFFFFFFFu;
}

int wtp_crc32_batch_fixed(const void *d_payloads, size_t stride, size_t len, size_t n, uint32_t *d_out,
                          void *stream) {
    if (n == 0) return WTP_OK;
    if (!d_out || (!d_payloads && len > 0)) return fail(WTP_EINVAL, "null pointer");
    if (len > kMaxVarLen) return fail(WTP_EINVAL, "len %zu > %u", len, kMaxVarLen);
    DevState *s = nullptr;
    int rc = current(s);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *b = static_cast<const uint8_t *>(d_payloads);
    // braided fast path (stride <= 16 KiB: the range the parity tests cover)
    const bool fast = len >= 16 && len <= 1536 && len % 16 == 0 && stride % 16 == 0 && stride <= 16384 &&
                      reinterpret_cast<uintptr_t>(b) % 16 == 0;
    if (fast) return launch_fixed_braid(*s, b, stride, uint32_t(len), n, dev::CrcBEpi{d_out, 0}, st);
    // general kernel, in sub-batches whose byte span stays < 2 GiB
    const uint64_t per = std::min<uint64_t>(kSubBatch, stride ? std::max<uint64_t>(1, ((1ull << 30) - 4096) / stride) : n);
    for (uint64_t p = 0; p < n; p += per) {
        const uint64_t cnt = std::min<uint64_t>(per, n - p);
        const uint8_t *sb = b + p * stride;
        const uint64_t lead = reinterpret_cast<uintptr_t>(sb) & 15u;
        const uint64_t span = (cnt - 1) * stride + len;
        rc = launch_pieces(*s, sb, span, dev::FixedProvL{stride, lead, uint32_t(len)}, cnt,
                           dev::CrcEpi{d_out + p, uint32_t(cnt)}, st);
        if (rc) return rc;
    }
    return WTP_OK;
}

int wtp_crc32_batch_var(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                        const uint32_t *d_lengths, size_t n, uint32_t *d_out, void *stream) {
    if (n == 0) return WTP_OK;
    if (!d_base || !d_offsets || !d_lengths || !d_out) return fail(WTP_EINVAL, "null pointer");
    DevState *s = nullptr;
    int rc = current(s);
    if (rc) return rc;
    const uint8_t *b = static_cast<const uint8_t *>(d_base);
    const uint64_t lead = reinterpret_cast<uintptr_t>(b) & 15u;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The general kernel addresses a view of < 2 GiB (32-bit buffer offsets).  Larger
    // buffers take launch_packed_ranges: device-cut < 2 GiB sub-launches of the same
    // kernel when the offsets are packed (the common layout even through this entry),
    // else the gated stream kernel (64-bit offsets, exact for any layout) redoes the batch.
    if (((lead + base_bytes + 15) & ~uint64_t(15)) >= (1ull << 31))
        return launch_packed_ranges(*s, b, base_bytes, d_offsets, d_lengths, n, d_out, st);
    for (uint64_t p = 0; p < n; p += kSubBatch) {
        const uint64_t cnt = std::min<uint64_t>(kSubBatch, n - p);
        rc = launch_pieces(*s, b, base_bytes, dev::ArrayProvL{d_offsets + p, d_lengths + p, lead, uint32_t(cnt)}, cnt,
                           dev::CrcEpi{d_out + p, uint32_t(cnt)}, st);
        if (rc) break;
    }
    return rc;
}

int wtp_crc32_batch_packed(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                           const uint32_t *d_lengths, size_t n, uint32_t *d_out, void *stream) {
    if (n == 0) return WTP_OK;
    if (!d_base || !d_offsets || !d_lengths || !d_out) return fail(WTP_EINVAL, "null pointer");
    // The piece-stream kernel is the faster one on every distribution measured (C5 Zipf
    // 1.1: 45.6 vs 57.0 us), so below 2 GiB a packed batch takes the same route as
    // wtp_crc32_batch_var, and from 2 GiB on it runs the same kernel in < 2 GiB
    // sub-launches cut on the device (launch_packed_ranges).  WTP_STREAM_KERNEL=1 in the
    // environment forces the stream kernel (tests, measurements).
    const char *force = getenv("WTP_STREAM_KERNEL");
    const bool stream_kernel = force && force[0] == '1';
    const uint64_t lead = reinterpret_cast<uintptr_t>(d_base) & 15u;
    const bool big = ((lead + base_bytes + 15) & ~uint64_t(15)) >= (1ull << 31);
    if (!stream_kernel && !big) return wtp_crc32_batch_var(d_base, base_bytes, d_offsets, d_lengths, n, d_out, stream);
    DevState *s = nullptr;
    int rc = current(s);
    if (rc) return rc;
    if (!stream_kernel)
        return launch_packed_ranges(*s, static_cast<const uint8_t *>(d_base), base_bytes, d_offsets, d_lengths, n,
                                    d_out, static_cast<hipStream_t>(stream));
    return launch_stream(*s, static_cast<const uint8_t *>(d_base), base_bytes, d_offsets, d_lengths, n, d_out,
                         static_cast<hipStream_t>(stream));
}

int wtp_crc32_verify_batch(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                           uint8_t *d_ok, uint32_t *d_crc_out, void *stream) {
    if (n == 0) return WTP_OK;
    if (!d_dgrams || !d_recv_len || !d_ok) return fail(WTP_EINVAL, "null pointer");
    if (stride < 16) return fail(WTP_EINVAL, "stride %zu < 16", stride);
    DevState *s = nullptr;
    int rc = current(s);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *b = static_cast<const uint8_t *>(d_dgrams);
    // Braided fast path for a 16-B aligned ring: one launch per sub-batch decides every
    // datagram of the ring's full WTP length 16 + min(stride - 16, 1456) (1472 B in
    // wReceiver's 1504-B slots or in a packed 1472-B ring); each workgroup then finishes
    // the rest of its own datagrams (short, empty, 1473-1500 B, malformed) in its fix-up
    // phase (verify_fixup).  No memory outside the caller's buffers, so captures, graph
    // replays and concurrent calls on any streams need nothing from the host.  The
    // sub-batches keep each launch's ring view below 2 GiB (32-bit buffer offsets).
    if (stride % 16 == 0 && stride >= 32 && stride <= 16384 && reinterpret_cast<uintptr_t>(b) % 16 == 0) {
        const uint32_t flen = uint32_t(std::min<size_t>(stride - 16, WTP_MAX_PAYLOAD));
        const uint64_t per = std::min<uint64_t>(kSubBatch, ((1ull << 31) - 4096) / stride);
        for (uint64_t p = 0; p < n && !rc; p += per) {
            const uint64_t cnt = std::min<uint64_t>(per, n - p);
            const uint8_t *sb = b + p * stride;
            rc = launch_fixed_braid(*s, sb + 16, stride, flen, cnt,
                                    dev::VerifyBEpi{d_recv_len + p, sb, stride, d_ok + p,
                                                    d_crc_out ? d_crc_out + p : nullptr, s->status, 0, cnt, 16u + flen},
                                    st);
        }
        return rc;
    }
    const uint64_t per = std::min<uint64_t>(kSubBatch, std::max<uint64_t>(1, (1ull << 30) / stride));
    for (uint64_t p = 0; p < n; p += per) {
        const uint64_t cnt = std::min<uint64_t>(per, n - p);
        const uint8_t *sb = b + p * stride;
        const uint64_t lead = reinterpret_cast<uintptr_t>(sb) & 15u;
        rc = launch_pieces(*s, sb, cnt * stride, dev::DgramProvL{stride, lead, d_recv_len + p}, cnt,
                           dev::VerifyEpi{d_ok + p, d_crc_out ? d_crc_out + p : nullptr, uint32_t(cnt)}, st);
        if (rc) return rc;
    }
    return WTP_OK;
}

int wtp_synth_fill(void *d_out, uint64_t start_byte, size_t nbytes, uint64_t seed, void *stream) {
    if (nbytes == 0) return WTP_OK;
    if (!d_out) return fail(WTP_EINVAL, "null pointer");
    const uint64_t words = (nbytes + 16) / 8;
    uint64_t blocks = (words + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(dev::k_synth, dim3(unsigned(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint8_t *>(d_out), start_byte, uint64_t(nbytes), seed);
    return launch_check("k_synth");
}

int wtp_build_data_packets(const void *d_payloads, size_t total_bytes, uint32_t seq0, void *d_wire,
                           size_t wire_stride, uint32_t *d_wire_len, void *stream) {
    if (total_bytes == 0) return WTP_OK;
    if (!d_payloads || !d_wire) return fail(WTP_EINVAL, "null pointer");
    if (wire_stride < 16 + WTP_MAX_PAYLOAD) return fail(WTP_EINVAL, "wire_stride %zu < 1472", wire_stride);
    DevState *s = nullptr;
    int rc = current(s);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t nch = (total_bytes + WTP_MAX_PAYLOAD - 1) / WTP_MAX_PAYLOAD;
    const uint64_t full = total_bytes / WTP_MAX_PAYLOAD;
    const uint8_t *pay = static_cast<const uint8_t *>(d_payloads);
    uint8_t *wire = static_cast<uint8_t *>(d_wire);
    // Fused path: the braided kernel reads each full chunk once, copies it into its wire
    // slot and writes the header (16-B aligned buffers and slots).
    const bool fused = reinterpret_cast<uintptr_t>(pay) % 16 == 0 && reinterpret_cast<uintptr_t>(wire) % 16 == 0 &&
                       wire_stride % 16 == 0 && wire_stride <= 16384;
    const uint64_t first = fused ? full : 0;  // chunks [first, nch) take the three-step path
    if (fused && full &&
        (rc = launch_fixed_braid(*s, pay, WTP_MAX_PAYLOAD, WTP_MAX_PAYLOAD, full,
                                 dev::BuildBEpi{wire, wire_stride, seq0, WTP_MAX_PAYLOAD, d_wire_len, 0}, st)))
        return rc;
    const uint64_t nslow = nch - first;
    if (!nslow) return WTP_OK;
    // Three-step path (unaligned buffers, and the short last chunk): copy into the slots,
    // CRC over the slots, then the headers.  CRCs land in d_wire_len first (then become
    // the lengths), else in stream-ordered scratch.
    const uint8_t *spay = pay + first * WTP_MAX_PAYLOAD;
    uint8_t *swire = wire + first * wire_stride;
    const uint64_t stotal = total_bytes - first * WTP_MAX_PAYLOAD;
    uint32_t *crc = d_wire_len ? d_wire_len + first : nullptr;
    uint32_t *tmp = nullptr;
    if (!crc) {
        WTP_HIP(hipMallocFromPoolAsync(reinterpret_cast<void **>(&tmp), nslow * 4, s->pool, st));
        crc = tmp;
    }
    {
        const uint64_t work = nslow * (WTP_MAX_PAYLOAD / 4 + 1);
        uint64_t blocks = (work + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL(dev::k_wire_copy, dim3(unsigned(blocks)), dim3(256), 0, st, spay, stotal, swire,
                           uint64_t(wire_stride), nslow);
        rc = launch_check("k_wire_copy");
    }
    const uint64_t sfull = stotal / WTP_MAX_PAYLOAD;
    const uint64_t tail = stotal - sfull * WTP_MAX_PAYLOAD;
    if (!rc && sfull) rc = wtp_crc32_batch_fixed(swire + 16, wire_stride, WTP_MAX_PAYLOAD, sfull, crc, stream);
    if (!rc && tail) rc = wtp_crc32_batch_fixed(swire + sfull * wire_stride + 16, 0, tail, 1, crc + sfull, stream);
    if (!rc) {
        uint64_t blocks = (nslow + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL(dev::k_wire_header, dim3(unsigned(blocks)), dim3(256), 0, st, crc, stotal,
                           seq0 + uint32_t(first), swire, uint64_t(wire_stride), crc == tmp ? nullptr : crc, nslow);
        rc = launch_check("k_wire_header");
    }
    if (tmp) {
        const hipError_t fe = hipFreeAsync(tmp, st);
        if (!rc && fe != hipSuccess) rc = fail(WTP_EHIP, "hipFreeAsync: %s", hipGetErrorString(fe));
    }
    if (rc) return rc;
    return WTP_OK;
}

}  // extern "C"
