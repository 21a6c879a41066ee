// wtp_advance.hip — slide both windows on the device (include/wtp_crc32.h: wtp_rx_advance,
// wtp_tx_advance), the calls that close a protocol round: the receiver's follows
// wtp_rx_deliver and moves accept's window state down by the number of slots delivered, the
// sender's follows wtp_tx_ingest_acks and moves d_acked / d_sent_ms down by the leading
// ACKed run.  Both read the advance from device memory when the kernel runs (deliver's and
// ingest's d_counts as they are), so a round needs no host read before it and one captured
// graph serves every round.
//
// Both write a second copy of the state: an in-place slide makes every destination slot the
// source of another one, and workgroups run in no defined order.
//
//   k_rx_advance  one launch.  A wave takes 64 consecutive destination slots per round
//                 (grid-stride over rounds, the grid capped): lane l loads d_slot_len[s0 + l
//                 + a] (EMPTY behind the window's end) and stores d_slot_len_next[s0 + l],
//                 one coalesced 256-B read and write.  Then the wave walks the ballot of the
//                 lanes with 1 <= v <= 1456, four slots per step, one per 16-lane group: a
//                 group copies its slot's floor(v / 16) vectors (k_accept_place's shape: a
//                 full slot is six vectors per lane, all loads issued before the first
//                 store, so a full window keeps 4 x 1456 B in flight per wave and step; a
//                 shorter one a loop of a vector or two per lane), and the v % 16 tail one
//                 byte per lane.  Cost follows the filled bytes: a slot that holds
//                 nothing costs its 4 + 4 bytes of d_slot_len and no branch of its own.
//                 Images that are not both 16-B aligned move byte by byte.
//   k_tx_advance  one lane per entry of both arrays.
// No LDS, no atomics, no scratch, no library table; *d_adv is one uniform load.
// k_rx_advance keeps its own copy of the slot copy's text (wtp_common.hpp: copy_slot16): on the
// helper its machine code changed and the timing rule did not let it move.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

#ifndef WTP_ADVANCE_NT
#define WTP_ADVANCE_NT 0  // k_rx_advance's 16-B image stores are plain; A/B builds: 1 = streaming (nt), slower here
#endif

namespace wtp {
namespace dev {

constexpr uint32_t kAdvBlock = 256;  // four waves, each on its own rounds
constexpr uint32_t kAdvWaves = kAdvBlock / 64;
constexpr uint32_t kAdvMaxBlocks = 2048;  // the capped grid: eight workgroups per CU, 2^19 slots per pass
static_assert(uint64_t(WTP_RX_MAX_WINDOW) * 2 < (uint64_t(1) << 32), "s + a fits 32 bits");

__device__ __forceinline__ void adv_store(u32x4 *p, u32x4 v) {
    if (WTP_ADVANCE_NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// eight waves per SIMD: left to itself the register allocator spreads the six vectors of a
// full slot over 90 VGPRs (five waves); bound, it takes 49 and spills nothing
__global__ void __launch_bounds__(kAdvBlock, 8)
k_rx_advance(const uint8_t *__restrict__ img, const uint32_t *__restrict__ slot_len, uint32_t window,
             const uint64_t *__restrict__ adv, uint8_t *__restrict__ img_next, uint32_t *__restrict__ slot_len_next,
             uint32_t vec) {
    const uint64_t by = *adv;
    const uint32_t a = by < window ? uint32_t(by) : window;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x / 64, g = lane % kGroup, q = lane / kGroup;
    const uint32_t rounds = (window + 63) / 64, step = gridDim.x * kAdvWaves;
    for (uint32_t r = blockIdx.x * kAdvWaves + wv; r < rounds; r += step) {
        const uint32_t s = r * 64 + lane;
        uint32_t v = WTP_SLOT_EMPTY;
        if (s < window) {
            const uint32_t t = s + a;
            if (t < window) v = slot_len[t];
            slot_len_next[s] = v;  // every value as it is
        }
        // the slots with bytes to move (a lane past the window holds EMPTY), four per step
        uint64_t todo = __ballot(img != nullptr && v - 1u < WTP_MAX_PAYLOAD);
        while (todo) {
            uint32_t pick = 64;
#pragma unroll
            for (uint32_t j = 0; j < 64 / kGroup; ++j) {
                const uint32_t b = todo ? uint32_t(__builtin_ctzll(todo)) : 64u;
                todo &= todo - 1;
                if (q == j) pick = b;
            }
            const uint32_t len = __shfl(v, pick & 63u, 64);  // by every lane of the wave
            if (pick == 64) continue;
            const uint32_t sd = r * 64 + pick;
            const uint8_t *src = img + uint64_t(sd + a) * WTP_MAX_PAYLOAD;
            uint8_t *dst = img_next + uint64_t(sd) * WTP_MAX_PAYLOAD;
            if (vec) {
                const u32x4 *vs = reinterpret_cast<const u32x4 *>(src);
                u32x4 *vd = reinterpret_cast<u32x4 *>(dst);
                const uint32_t nvec = len / 16;
                if (len == WTP_MAX_PAYLOAD) {
                    // a full slot, 91 vectors: rows 0 .. 4 whole, row 5 lanes 0 .. 10; all of a
                    // lane's loads are in flight before its first store
                    u32x4 w[kSlotVecs];
#pragma unroll
                    for (uint32_t k = 0; k + 1 < kSlotVecs; ++k) w[k] = vs[g + k * kGroup];
                    const bool last = g + (kSlotVecs - 1) * kGroup < WTP_MAX_PAYLOAD / 16;
                    if (last) w[kSlotVecs - 1] = vs[g + (kSlotVecs - 1) * kGroup];
#pragma unroll
                    for (uint32_t k = 0; k + 1 < kSlotVecs; ++k) adv_store(vd + g + k * kGroup, w[k]);
                    if (last) adv_store(vd + g + (kSlotVecs - 1) * kGroup, w[kSlotVecs - 1]);
                } else {
                    // a shorter one: a Zipf record is a vector or two per lane
#pragma clang loop unroll_count(2)
                    for (uint32_t x = g; x < nvec; x += kGroup) adv_store(vd + x, vs[x]);
                }
                const uint32_t b = nvec * 16 + g;  // byte-exact tail: at most 15 bytes, one per lane
                if (b < len) dst[b] = src[b];
            } else {
                // any other alignment: bytes (exact; no access wider than the images' alignment)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
                for (uint32_t b = g; b < len; b += kGroup) dst[b] = src[b];
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_tx_advance(const uint32_t *__restrict__ acked, const uint32_t *__restrict__ sent_ms, uint32_t slots,
             const uint32_t *__restrict__ adv, uint32_t fill_ms, uint32_t *__restrict__ acked_next,
             uint32_t *__restrict__ sent_ms_next) {
    const uint32_t a = min(*adv, slots);
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    const uint32_t t = s + a;  // <= 2^21
    acked_next[s] = t < slots ? acked[t] : 0u;
    sent_ms_next[s] = t < slots ? sent_ms[t] : fill_ms;
}

}  // namespace dev
}  // namespace wtp

extern "C" int wtp_rx_advance(const void *d_img, const uint32_t *d_slot_len, uint32_t window, const uint64_t *d_adv,
                              void *d_img_next, uint32_t *d_slot_len_next, void *stream) {
    using namespace wtp;
    if (window > WTP_RX_MAX_WINDOW) return fail(WTP_EINVAL, "window %u > %u", window, WTP_RX_MAX_WINDOW);
    if (!d_img != !d_img_next)
        return fail(WTP_EINVAL, "null pointer: %s without %s", d_img ? "d_img_next" : "d_img", d_img ? "d_img" : "d_img_next");
    if (window == 0) return WTP_OK;
    if (!d_adv) return fail(WTP_EINVAL, "null pointer: d_adv with window %u", window);
    if (!d_slot_len) return fail(WTP_EINVAL, "null pointer: d_slot_len with window %u", window);
    if (!d_slot_len_next) return fail(WTP_EINVAL, "null pointer: d_slot_len_next with window %u", window);
    if (overlap(d_slot_len, d_slot_len_next, uint64_t(window) * 4))
        return fail(WTP_EINVAL, "d_slot_len_next overlaps d_slot_len (window %u)", window);
    if (d_img && overlap(d_img, d_img_next, uint64_t(window) * WTP_MAX_PAYLOAD))
        return fail(WTP_EINVAL, "d_img_next overlaps d_img (window %u)", window);
    // the grid from the window, never from *d_adv
    const uint32_t groups = ((window + 63) / 64 + dev::kAdvWaves - 1) / dev::kAdvWaves;
    const unsigned blocks = std::min(groups, dev::kAdvMaxBlocks);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(d_img) | reinterpret_cast<uintptr_t>(d_img_next)) & 15u) == 0;
    return launch("k_rx_advance", dev::k_rx_advance, dim3(blocks), dim3(dev::kAdvBlock), static_cast<hipStream_t>(stream),
                  static_cast<const uint8_t *>(d_img), d_slot_len, window, d_adv, static_cast<uint8_t *>(d_img_next),
                  d_slot_len_next, vec);
}

extern "C" int wtp_tx_advance(const uint32_t *d_acked, const uint32_t *d_sent_ms, uint32_t slots, const uint32_t *d_adv,
                              uint32_t fill_ms, uint32_t *d_acked_next, uint32_t *d_sent_ms_next, void *stream) {
    using namespace wtp;
    if (slots > WTP_TX_MAX_INFLIGHT) return fail(WTP_EINVAL, "slots %u > %u", slots, WTP_TX_MAX_INFLIGHT);
    if (slots == 0) return WTP_OK;
    if (!d_adv) return fail(WTP_EINVAL, "null pointer: d_adv with slots %u", slots);
    if (!d_acked) return fail(WTP_EINVAL, "null pointer: d_acked with slots %u", slots);
    if (!d_sent_ms) return fail(WTP_EINVAL, "null pointer: d_sent_ms with slots %u", slots);
    if (!d_acked_next) return fail(WTP_EINVAL, "null pointer: d_acked_next with slots %u", slots);
    if (!d_sent_ms_next) return fail(WTP_EINVAL, "null pointer: d_sent_ms_next with slots %u", slots);
    // an output over either input: another workgroup may still read what this one writes
    const void *in[2] = {d_acked, d_sent_ms}, *out[2] = {d_acked_next, d_sent_ms_next};
    const char *in_name[2] = {"d_acked", "d_sent_ms"}, *out_name[2] = {"d_acked_next", "d_sent_ms_next"};
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 2; ++i)
            if (overlap(in[i], out[o], uint64_t(slots) * 4))
                return fail(WTP_EINVAL, "%s overlaps %s (slots %u)", out_name[o], in_name[i], slots);
    if (overlap(d_acked_next, d_sent_ms_next, uint64_t(slots) * 4))
        return fail(WTP_EINVAL, "d_sent_ms_next overlaps d_acked_next (slots %u)", slots);
    return launch("k_tx_advance", dev::k_tx_advance, dim3((slots + 255) / 256), dim3(256), static_cast<hipStream_t>(stream),
                  d_acked, d_sent_ms, slots, d_adv, fill_ms, d_acked_next, d_sent_ms_next);
}
