// wtp_deliver.hip — in-order flush of the receive window as a packed stream (include/
// wtp_crc32.h: wtp_rx_deliver), the receiver's sixth call: it follows
// wtp_accept_data_packets and wtp_rx_build_acks and turns the leading run of filled slots
// back into the byte stream that wtp_build_data_packets_var started from
// (cpp/src/base/Receiver.cpp:208-237, the std::map loop of wReceiver.cpp).
//
// The mirror image of k_build_var: there the source sits at arbitrary byte addresses and
// the destination is 16-B aligned; here the source slots are 16-B aligned (1456 = 91 * 16)
// and the destination is one contiguous stream at an arbitrary byte phase.
//
// Stream-ordered launches, scratch in the caller's d_work (hdr[4], bsum[ceil(window /
// 1024)], bend[the same], P[window + 1]):
//   k_deliver_bsum  per 1024-slot block: the sum of the valid lengths and the index of the
//                   first slot whose length ends the run (> WTP_MAX_PAYLOAD), else ~0
//   k_deliver_scan  every block reduces the block entries (<= 1024, one per lane): the
//                   bytes before it and the run; scans its own 1024 slots: P[s] = the
//                   exclusive prefix sum, P[window] = the total.  "Delivered" is a monotone
//                   predicate per slot (s < run, s < max_slots, P[s] + len <= stream_bytes -
//                   stream_off), so the one slot where it turns false is k: that lane
//                   writes d_counts[0], [2] and hdr = {k, P[k]}, the lane at s == run writes
//                   d_counts[1], [3]; a delivered slot's lane writes d_offsets_out /
//                   d_lengths_out.  No atomics, no host read.
//   k_deliver_copy  one lane per 16-B destination vector: lane v covers stream bytes [A +
//                   16 v, + 16), A = the 16-B boundary at or below d_stream + stream_off, so
//                   the stores are fully coalesced and lanes are busy in proportion to
//                   bytes whatever the mix of lengths.  A wave takes 4 KiB of the stream
//                   per round (four vectors per lane, all loads issued before the first
//                   store).  Lanes 0 .. 31 find the owner of the round's first byte and lanes
//                   32 .. 63 of its last byte in P[0 .. k], 32 probes per step (four dependent
//                   loads for 2^20 slots, once per 4 KiB); the prefix sums between the two
//                   owners go to LDS (up to 256; a round of more records reads them from
//                   memory), and a lane finds the owner of its vector's first byte there.  A
//                   vector inside one record is loaded from the slot as the four dwords from
//                   the 4-B aligned address below the source byte plus the dword that
//                   follows, shifted by v_alignbyte_b32 (address & 3), and stored once.  A
//                   vector that spans records (any number: 1-byte and empty records) is
//                   merged from one such widened load per record, masked to the record's
//                   bytes; a widened load that would cross either end of the image, and
//                   every load of an image that is not 4-B aligned, is replaced by the
//                   record's own bytes one by one.  The first and last vector of the
//                   delivered range is stored byte by byte over exactly the delivered
//                   bytes, every other one whole.
// Every word of d_work that a kernel reads was written by an earlier launch of the same
// call; the call keeps no state and reads no library table.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

#ifndef WTP_DELIVER_NT
#define WTP_DELIVER_NT 1  // the copy kernel's 16-B stream stores stream (nt); A/B builds: 0
#endif
#ifndef WTP_DELIVER_LNT
#define WTP_DELIVER_LNT 0  // its 16-B image loads do not; A/B builds: 1
#endif

namespace wtp {
namespace dev {

constexpr uint32_t kDlBlock = 1024;  // slots per block of the two scan kernels
constexpr uint32_t kDlWaves = kDlBlock / 64;
static_assert(WTP_RX_MAX_WINDOW <= kDlBlock * kDlBlock, "one block entry per lane of k_deliver_scan");
static_assert(uint64_t(WTP_RX_MAX_WINDOW) * WTP_MAX_PAYLOAD < (uint64_t(1) << 31), "P fits 32 bits");
constexpr uint32_t kDlNone = 0xFFFFFFFFu;  // bend: no slot of the block ends the run

constexpr uint32_t kDlCopyBlock = 256;  // four waves, each on its own rounds
constexpr uint32_t kDlVecs = 4;         // 16-B vectors per lane and round
constexpr uint32_t kDlRound = 64 * kDlVecs;  // vectors per wave and round (4 KiB)
constexpr uint32_t kDlMaxBlocks = 2048;  // the capped grid: eight workgroups per CU (62 VGPRs), 32 MiB of the stream per pass
constexpr uint32_t kDlStage = 256;      // prefix sums a wave keeps in LDS per round

__global__ void __launch_bounds__(kDlBlock)
k_deliver_bsum(const uint32_t *__restrict__ slot_len, uint32_t window, uint32_t *__restrict__ bsum,
               uint32_t *__restrict__ bend) {
    __shared__ uint32_t psum[kDlWaves], pend[kDlWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kDlBlock + t;
    const uint32_t len = s < window ? slot_len[s] : 0u;
    const bool bad = len > WTP_MAX_PAYLOAD;
    const uint32_t sum = wave_sum(bad ? 0u : len), end = wave_min(bad ? s : kDlNone);
    if ((t & 63u) == 0) {
        psum[t / 64] = sum;
        pend[t / 64] = end;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t a = 0, e = kDlNone;
        for (uint32_t w = 0; w < kDlWaves; ++w) {
            a += psum[w];
            e = min(e, pend[w]);
        }
        bsum[blockIdx.x] = a;
        bend[blockIdx.x] = e;
    }
}

__global__ void __launch_bounds__(kDlBlock)
k_deliver_scan(const uint32_t *__restrict__ slot_len, uint32_t window, uint32_t max_slots, uint64_t stream_off,
               uint64_t room, const uint32_t *__restrict__ bsum, const uint32_t *__restrict__ bend,
               uint32_t nblk, uint32_t *__restrict__ P, uint32_t *__restrict__ hdr, uint64_t *__restrict__ offs_out,
               uint32_t *__restrict__ lens_out, uint64_t *__restrict__ counts) {
    __shared__ uint32_t before[kDlWaves], ends[kDlWaves], wave_top[kDlWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kDlBlock + t, w = t / 64, lane = t & 63u;
    if (window == 0) {  // one block: nothing to scan
        if (t == 0) {
            P[0] = 0;
            hdr[0] = hdr[1] = 0;
            counts[0] = counts[1] = counts[2] = counts[3] = 0;
        }
        return;
    }
    // the bytes of the blocks before this one and the run over all blocks (nblk <= 1024)
    const uint32_t part = wave_sum(t < blockIdx.x ? bsum[t] : 0u);
    const uint32_t pe = wave_min(t < nblk ? bend[t] : kDlNone);
    const uint32_t len = s < window ? slot_len[s] : 0u;
    const uint32_t v = len > WTP_MAX_PAYLOAD ? 0u : len;
    uint32_t inc = v;  // inclusive prefix sum over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 0) {
        before[w] = part;
        ends[w] = pe;
    }
    if (lane == 63) wave_top[w] = inc;
    __syncthreads();
    uint32_t pre = 0, run = kDlNone;
    for (uint32_t k = 0; k < kDlWaves; ++k) {
        pre += before[k] + (k < w ? wave_top[k] : 0u);
        run = min(run, ends[k]);
    }
    run = min(run, window);
    const uint32_t ex = pre + inc - v;  // P_s (for s >= run: a defined value nobody uses)
    if (s > window) return;
    P[s] = ex;  // s == window: the total
    if (s == window) return;
    // delivered(s), and delivered(s - 1) from this lane's own values: P_(s-1) + len_(s-1) = P_s
    const bool fits_before = ex <= room;  // room = stream_bytes - stream_off
    const bool mine = s < run && s < max_slots && uint64_t(ex) + v <= room;
    const bool prev = s == 0 || (s - 1 < run && s - 1 < max_slots && fits_before);
    if (mine) {
        if (offs_out) offs_out[s] = stream_off + ex;
        if (lens_out) lens_out[s] = v;
    }
    // the predicate is monotone: exactly one of these two holds for exactly one slot
    if (!mine && prev) {
        counts[0] = s;
        counts[2] = ex;
        hdr[0] = s;
        hdr[1] = ex;
    } else if (mine && s + 1 == window) {
        counts[0] = window;
        counts[2] = ex + v;
        hdr[0] = window;
        hdr[1] = ex + v;
    }
    if (s == run) {
        counts[1] = run;
        counts[3] = ex;
    } else if (run == window && s + 1 == window) {
        counts[1] = window;
        counts[3] = ex + v;
    }
}

// Delivered bytes [b0, b1), b1 - b0 <= 16, as bytes [skip, skip + b1 - b0) of a vector, piece
// by piece: a piece is what one record gives to the vector.  Each piece comes from one
// widened load of the 16 source bytes that put it at its place in the vector (the bytes
// around it belong to the slot's tail or a neighbouring slot and are masked off); where that
// load would leave the image, or the image is not 4-B aligned, from its own bytes one by
// one.  o owns b0; p(i) = P[i].
template <class Get>
__device__ __forceinline__ u32x4 dl_merge(const uint8_t *__restrict__ img, uint32_t img_bytes, uint32_t vec, Get p,
                                          uint32_t o, uint32_t b0, uint32_t b1, uint32_t skip) {
    uint64_t lo = 0, hi = 0;
    uint32_t cur = p(o), nxt = p(o + 1);
    uint32_t j = b0;
    while (j < b1) {
        while (j >= nxt) {  // the next record with a byte: j < P[k], so o + 1 <= k
            ++o;
            cur = nxt;
            nxt = p(o + 1);
        }
        const uint32_t end = min(nxt, b1), pos = skip + (j - b0), nb = end - j;  // bytes [pos, pos + nb) of the vector
        const uint32_t x = o * WTP_MAX_PAYLOAD + (j - cur);                      // the image byte of j
        const uint32_t s = x - pos, sh = s & 3u, a = s - sh;
        uint64_t vlo = 0, vhi = 0;
        if (vec && x >= pos && a + (sh ? 20u : 16u) <= img_bytes) {
            const u32x4 d = *reinterpret_cast<const u32x4_a4 *>(img + a);
            const uint32_t e = *reinterpret_cast<const uint32_t *>(img + a + (sh ? 16 : 12));
            vlo = (uint64_t(__builtin_amdgcn_alignbyte(d.z, d.y, sh)) << 32) | __builtin_amdgcn_alignbyte(d.y, d.x, sh);
            vhi = (uint64_t(__builtin_amdgcn_alignbyte(e, d.w, sh)) << 32) | __builtin_amdgcn_alignbyte(d.w, d.z, sh);
        } else {
#pragma clang loop unroll(disable)
            for (uint32_t q = 0; q < nb; ++q) {
                const uint64_t byte = img[x + q];
                if (pos + q < 8)
                    vlo |= byte << (8 * (pos + q));
                else
                    vhi |= byte << (8 * (pos + q - 8));
            }
        }
        lo |= vlo & below_lo(pos + nb) & ~below_lo(pos);
        hi |= vhi & below_hi(pos + nb) & ~below_hi(pos);
        j = end;
    }
    u32x4 r;
    r.x = uint32_t(lo);
    r.y = uint32_t(lo >> 32);
    r.z = uint32_t(hi);
    r.w = uint32_t(hi >> 32);
    return r;
}

__device__ __forceinline__ void dl_store(u32x4 *p, u32x4 v) {
    if (WTP_DELIVER_NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

__global__ void __launch_bounds__(kDlCopyBlock)
k_deliver_copy(const uint8_t *__restrict__ img, uint32_t img_bytes, uint32_t vec, const uint32_t *__restrict__ P,
               const uint32_t *__restrict__ hdr, uint8_t *__restrict__ dst, uint32_t ph) {
    __shared__ uint32_t s_P[kDlCopyBlock / 64][kDlStage];
    // dst = A, the 16-B boundary at or below the first delivered byte, which is dst[ph]
    const uint32_t k = hdr[0], total = hdr[1];
    if (total == 0) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x / 64;
    const uint32_t nvec = (ph + total + 15) / 16;  // total < 2^31
    const uint32_t rounds = (nvec + kDlRound - 1) / kDlRound, step_r = gridDim.x * (kDlCopyBlock / 64);
    for (uint32_t r = blockIdx.x * (kDlCopyBlock / 64) + wv; r < rounds; r += step_r) {
        const uint32_t v0 = r * kDlRound;
        // the records this round's bytes come from: between the owners of its first and last byte
        const uint32_t fb = 16 * v0 > ph ? 16 * v0 - ph : 0u;
        const uint32_t lb = min(16 * (v0 + kDlRound) - ph, total) - 1;  // 16 * (v0 + 256) <= 2^31 + 4 KiB
        const uint32_t edge = owner_wave(P, k, lane < 32 ? fb : lb, lane);
        const uint32_t olo = __shfl(edge, 0, 64), ohi = __shfl(edge, 63, 64);
        // their prefix sums P[olo .. ohi + 1] in LDS, if they fit (a round of 4 KiB holds 30 Zipf records)
        const uint32_t cnt = ohi - olo + 2;
        const bool staged = cnt <= kDlStage;
        if (staged)
            for (uint32_t i = lane; i < cnt; i += 64) s_P[wv][i] = P[olo + i];
        wave_sync();
        // the round over p(i) = P[i]: from LDS, or from memory (two bodies: one pointer, one address space each)
        auto body = [&](auto p) {
        uint32_t b0[kDlVecs], b1[kDlVecs], own[kDlVecs], sh[kDlVecs], soff[kDlVecs];
        bool fast[kDlVecs];
#pragma unroll
        for (uint32_t u = 0; u < kDlVecs; ++u) {
            const uint32_t v = v0 + 64 * u + lane;
            b0[u] = 16 * v > ph ? 16 * v - ph : 0u;
            b1[u] = v < nvec ? min(16 * v + 16 - ph, total) : 0u;
            own[u] = 0;
            sh[u] = 0;
            soff[u] = 0;
            fast[u] = false;
            if (b0[u] < b1[u]) {
                own[u] = owner(p, olo, ohi, b0[u]);
                const uint32_t x = own[u] * WTP_MAX_PAYLOAD + (b0[u] - p(own[u]));
                sh[u] = x & 3u;
                soff[u] = x - sh[u];
                // whole, inside one record, and the widened load inside the image
                fast[u] = vec && b1[u] - b0[u] == 16 && b0[u] + 16 <= p(own[u] + 1) &&
                          soff[u] + (sh[u] ? 20u : 16u) <= img_bytes;
            }
        }
        u32x4 d[kDlVecs] = {};
        uint32_t e[kDlVecs] = {};
#pragma unroll
        for (uint32_t u = 0; u < kDlVecs; ++u)
            if (fast[u]) {
                const uint8_t *q = img + soff[u];  // the dword that holds the first byte
                const u32x4_a4 *q4 = reinterpret_cast<const u32x4_a4 *>(q);
                d[u] = WTP_DELIVER_LNT ? __builtin_nontemporal_load(q4) : *q4;
                e[u] = *reinterpret_cast<const uint32_t *>(q + (sh[u] ? 16 : 12));  // sh == 0: d.w again, unused
            }
        uint32_t slow = 0;  // the vectors that are not one whole load: one after the other, in one body
#pragma unroll
        for (uint32_t u = 0; u < kDlVecs; ++u) {
            if (fast[u]) {
                u32x4 val;
                val.x = __builtin_amdgcn_alignbyte(d[u].y, d[u].x, sh[u]);
                val.y = __builtin_amdgcn_alignbyte(d[u].z, d[u].y, sh[u]);
                val.z = __builtin_amdgcn_alignbyte(d[u].w, d[u].z, sh[u]);
                val.w = __builtin_amdgcn_alignbyte(e[u], d[u].w, sh[u]);
                dl_store(reinterpret_cast<u32x4 *>(dst + 16 * uint64_t(v0 + 64 * u + lane)), val);
            } else if (b0[u] < b1[u]) {
                slow |= 1u << u;
            }
        }
        static_assert(kDlVecs == 4, "the selects below");
        while (slow) {
            const uint32_t u = __builtin_ctz(slow);
            slow &= slow - 1;
            const uint32_t c0 = u == 0 ? b0[0] : u == 1 ? b0[1] : u == 2 ? b0[2] : b0[3];
            const uint32_t c1 = u == 0 ? b1[0] : u == 1 ? b1[1] : u == 2 ? b1[2] : b1[3];
            const uint32_t o = u == 0 ? own[0] : u == 1 ? own[1] : u == 2 ? own[2] : own[3];
            const uint32_t v = v0 + 64 * u + lane;
            uint8_t *at = dst + 16 * uint64_t(v);
            // the vector's first delivered byte is byte `skip` of it (> 0 only in the stream's first vector)
            const uint32_t skip = c0 + ph - 16 * v;
            const u32x4 val = dl_merge(img, img_bytes, vec, p, o, c0, c1, skip);
            if (c1 - c0 == 16) {
                dl_store(reinterpret_cast<u32x4 *>(at), val);
            } else {
                // the first or last vector: exactly the delivered bytes
                // the loop stays rolled, or the compiler may merge the stores
                const uint64_t lo = (uint64_t(val.y) << 32) | val.x, hi = (uint64_t(val.w) << 32) | val.z;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
                for (uint32_t b = skip; b < skip + (c1 - c0); ++b)
                    at[b] = uint8_t(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
            }
        }
        };
        const uint32_t *sp = s_P[wv];
        if (staged)
            body([&](uint32_t i) { return sp[i - olo]; });
        else
            body([&](uint32_t i) { return P[i]; });
        wave_sync();  // the next round's s_P stores follow these loads
    }
}

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_rx_deliver: hdr[4] = {k, P[k], -, -}, bsum[nblk], bend[nblk], P[window + 1].
struct DeliverWork {
    uint32_t nblk;
    uint32_t *hdr, *bsum, *bend, *P;
    size_t bytes;
};

DeliverWork deliver_layout(void *d_work, uint32_t window) {
    DeliverWork w;
    wtp::Work l(d_work, 4);
    w.nblk = (window + wtp::dev::kDlBlock - 1) / wtp::dev::kDlBlock;
    w.hdr = l.take<uint32_t>(4);
    w.bsum = l.take<uint32_t>(w.nblk);
    w.bend = l.take<uint32_t>(w.nblk);
    w.P = l.take<uint32_t>(size_t(window) + 1);
    w.bytes = l.bytes();
    return w;
}

}  // namespace

extern "C" size_t wtp_rx_deliver_work_bytes(uint32_t window) {
    return deliver_layout(nullptr, std::min<uint32_t>(window, WTP_RX_MAX_WINDOW)).bytes;
}

extern "C" int wtp_rx_deliver(const void *d_img, const uint32_t *d_slot_len, uint32_t window, uint32_t max_slots,
                              void *d_stream, size_t stream_bytes, uint64_t stream_off, uint64_t *d_offsets_out,
                              uint32_t *d_lengths_out, uint64_t *d_counts, void *d_work, size_t work_bytes,
                              void *stream) {
    using namespace wtp;
    if (window > WTP_RX_MAX_WINDOW) return fail(WTP_EINVAL, "window %u > %u", window, WTP_RX_MAX_WINDOW);
    if (stream_off > stream_bytes)
        return fail(WTP_EINVAL, "stream_off %llu > stream_bytes %zu", static_cast<unsigned long long>(stream_off), stream_bytes);
    const DeliverWork w = deliver_layout(d_work, window);
    int rc = check_work_bytes(work_bytes, w.bytes);
    if (rc) return rc;
    if (!d_counts) return null_arg("d_counts");
    if (!d_work) return null_arg("d_work");
    if (window > 0) {
        if (!d_img) return fail(WTP_EINVAL, "null pointer: d_img with window %u", window);
        if (!d_slot_len) return fail(WTP_EINVAL, "null pointer: d_slot_len with window %u", window);
        if (max_slots > 0 && !d_stream)
            return fail(WTP_EINVAL, "null pointer: d_stream with window %u and max_slots %u", window, max_slots);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (window > 0) {
        if ((rc = launch("k_deliver_bsum", dev::k_deliver_bsum, dim3(w.nblk), dim3(dev::kDlBlock), st, d_slot_len, window,
                         w.bsum, w.bend)))
            return rc;
    }
    // window == 0: one block, which only writes d_counts = {0, 0, 0, 0}
    rc = launch("k_deliver_scan", dev::k_deliver_scan, dim3(window / dev::kDlBlock + 1), dim3(dev::kDlBlock), st, d_slot_len,
                window, max_slots, stream_off, uint64_t(stream_bytes) - stream_off, w.bsum, w.bend, w.nblk, w.P, w.hdr,
                d_offsets_out, d_lengths_out, d_counts);
    if (rc || window == 0 || max_slots == 0) return rc;
    // the grid from what the arguments allow, never from d_counts: min(window, max_slots)
    // full slots, capped; a workgroup leaves at once when the scan delivered fewer bytes
    const uintptr_t first = reinterpret_cast<uintptr_t>(d_stream) + stream_off;
    const uint32_t ph = uint32_t(first & 15u);
    const uint64_t most = uint64_t(std::min(window, max_slots)) * WTP_MAX_PAYLOAD + ph;
    const uint64_t groups = (most + 16 * dev::kDlRound * (dev::kDlCopyBlock / 64) - 1) / (16 * dev::kDlRound * (dev::kDlCopyBlock / 64));
    const unsigned blocks = unsigned(std::min<uint64_t>(groups, dev::kDlMaxBlocks));
    const uint32_t vec = (reinterpret_cast<uintptr_t>(d_img) & 3u) == 0;
    return launch("k_deliver_copy", dev::k_deliver_copy, dim3(blocks), dim3(dev::kDlCopyBlock), st,
                  static_cast<const uint8_t *>(d_img), window * WTP_MAX_PAYLOAD, vec, w.P, w.hdr,
                  reinterpret_cast<uint8_t *>(first - ph), ph);
}
