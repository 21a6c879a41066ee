// wtp_accept.hip — device-side receive (include/wtp_crc32.h: wtp_accept_data_packets).
//
// The inverse of the fused builder: a batch of received datagrams in a device ring is
// verified, window-checked, de-duplicated and its payloads are copied to their place in
// the file image, with the cumulative ACK, in three stream-ordered launches and no host
// synchronisation.  Semantics: the sequential arrival-order loop of the reference's
// receiver (cpp/src/base/Receiver.cpp:25-35 memcpy into Packet1::data, :208-237 window
// check, buffering, next_seq) and of wReceiver.cpp's pending.emplace (first arrival wins).
//
//   1. verify        wtp_crc32_verify_batch (the braided kernel on an aligned ring) -> ok[]
//   2. k_accept_claim one lane per datagram: an intact in-window DATA datagram claims its
//                    slot with atomicMin(&slot_len[s], 0x80000000 | i).  EMPTY (0xFFFFFFFF)
//                    > any claim > any stored length (<= 1456), so a filled slot stays
//                    filled and the lowest index wins; the window state itself is the
//                    only scratch.
//   3. k_accept_place 16 lanes per datagram: the owner (slot_len[s] == 0x80000000 | i)
//                    copies its payload (wtp_common.hpp: copy_slot16), then publishes
//                    slot_len[s] = len and place[i];
//                    every lane also scans its share of slot_len for the first EMPTY slot
//                    (the cumulative ACK).
//
// The copy is not fused into the CRC rounds (as BuildBEpi::kCopy is on the send side): it
// would store payload bytes before the verdict, so a corrupt or duplicate datagram could
// overwrite good data and tear a slot.  Only the owner of a slot ever writes it.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

#ifndef WTP_ACCEPT_NT
#define WTP_ACCEPT_NT 1  // the place kernel's 16-B payload stores stream (nt); A/B builds: 0
#endif
#ifndef WTP_ACCEPT_LNT
#define WTP_ACCEPT_LNT 1  // the same for its 16-B ring loads
#endif

namespace wtp {
namespace dev {

// Slot of datagram i if it may be placed (intact, DATA, payload <= 1456 B, inside the
// window), else WTP_NOT_PLACED.  ok[i] != 0 already says 16 <= recv_len <= stride.
__device__ __forceinline__ uint32_t accept_slot(const uint8_t *__restrict__ ring, uint64_t stride,
                                                const uint32_t *__restrict__ recv_len, const uint8_t *__restrict__ ok,
                                                uint64_t i, uint32_t seq0, uint32_t window, uint32_t &len) {
    const uint8_t good = ok[i];
    const uint32_t rl = recv_len[i];
    if (!good) return WTP_NOT_PLACED;  // the header is read only where verify saw >= 16 bytes
    const uint8_t *h = ring + i * stride;
    const uint32_t type = be32(h), seq = be32(h + 4);  // the compiler merges these into one 8-B load
    len = rl - WTP_HEADER_BYTES;
    const uint32_t s = seq - seq0;  // unsigned: wrap is well defined
    return len <= WTP_MAX_PAYLOAD && type == WTP_TYPE_DATA && s < window ? s : WTP_NOT_PLACED;
}

__global__ void __launch_bounds__(256)
k_accept_claim(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
               const uint8_t *__restrict__ ok, uint64_t n, uint32_t seq0, uint32_t window, uint32_t *slot_len,
               uint32_t *ack) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i == 0 && ack) *ack = seq0 + window;  // "no EMPTY slot": k_accept_place lowers it
    if (i >= n) return;
    uint32_t len = 0;
    const uint32_t s = accept_slot(ring, stride, recv_len, ok, i, seq0, window, len);
    if (s != WTP_NOT_PLACED) atomicMin(&slot_len[s], kClaim | uint32_t(i));
}

__global__ void __launch_bounds__(256)
k_accept_place(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
               const uint8_t *__restrict__ ok, uint64_t n, uint32_t seq0, uint32_t window, uint8_t *__restrict__ out,
               uint32_t *slot_len, uint32_t *__restrict__ place, uint32_t *ack) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    // Cumulative ACK: the first EMPTY slot.  Every claim made by k_accept_claim is placed
    // below, so a claimed slot counts as filled whether or not its length is published
    // yet.  A lane walks its slots in rising order and stops at its first EMPTY one.
    if (ack) {
        const uint64_t step = uint64_t(gridDim.x) * blockDim.x;
        for (uint64_t s = t; s < window; s += step)
            if (__hip_atomic_load(&slot_len[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == WTP_SLOT_EMPTY) {
                ack_lower(ack, seq0, uint32_t(s));
                break;
            }
    }
    const uint64_t i = t / kGroup;
    const uint32_t g = uint32_t(t % kGroup);
    if (i >= n) return;
    uint32_t len = 0;
    uint32_t s = accept_slot(ring, stride, recv_len, ok, i, seq0, window, len);
    // the owner's claim is still in the slot: only this group publishes over it, and it
    // does so after this load (the 16 lanes of a group share a wave)
    if (s != WTP_NOT_PLACED && slot_len[s] != (kClaim | uint32_t(i))) s = WTP_NOT_PLACED;
    if (s == WTP_NOT_PLACED) {
        if (place && g == 0) place[i] = WTP_NOT_PLACED;
        return;
    }
    const uint8_t *src = ring + i * stride + WTP_HEADER_BYTES;
    uint8_t *dst = out + uint64_t(s) * WTP_MAX_PAYLOAD;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    copy_slot16<WTP_ACCEPT_LNT, WTP_ACCEPT_NT>(src, dst, len, g, vec);
    if (g == 0) {
        slot_len[s] = len;
        if (place) place[i] = s;
    }
}

}  // namespace dev
}  // namespace wtp

extern "C" int wtp_accept_data_packets(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                                       uint32_t seq0, uint32_t window, void *d_out, uint32_t *d_slot_len,
                                       uint8_t *d_ok, uint32_t *d_place, uint32_t *d_ack, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if (n > 0) {
        if ((rc = check_ring(d_dgrams, stride, d_recv_len, d_ok, !d_out || !d_slot_len))) return rc;
    } else {
        if (!d_ack) return WTP_OK;  // nothing to place, nothing to report
        if (window > 0 && !d_slot_len) return fail(WTP_EINVAL, "null pointer");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *ring = static_cast<const uint8_t *>(d_dgrams);
    rc = wtp_crc32_verify_batch(d_dgrams, stride, d_recv_len, n, d_ok, nullptr, stream);
    if (rc) return rc;
    {
        const uint64_t blocks = std::max<uint64_t>(1, (uint64_t(n) + 255) / 256);
        rc = launch("k_accept_claim", dev::k_accept_claim, dim3(unsigned(blocks)), dim3(256), st, ring, uint64_t(stride),
                    d_recv_len, d_ok, uint64_t(n), seq0, window, d_slot_len, d_ack);
        if (rc) return rc;
    }
    // one 16-lane group per datagram; at least enough lanes to scan a small window at once
    const uint64_t scan = d_ack ? std::min<uint64_t>((uint64_t(window) + 255) / 256, 1024) : 0;
    const uint64_t blocks = std::max<uint64_t>({1, (uint64_t(n) * dev::kGroup + 255) / 256, scan});
    return launch("k_accept_place", dev::k_accept_place, dim3(unsigned(blocks)), dim3(256), st, ring, uint64_t(stride),
                  d_recv_len, d_ok, uint64_t(n), seq0, window, static_cast<uint8_t *>(d_out), d_slot_len, d_place, d_ack);
}
