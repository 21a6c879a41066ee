// wtp_flows_flush.hip — multi-connection flush and slide (include/wtp_crc32.h:
// wtp_rx_deliver_flows, wtp_rx_advance_flows), the second half of the multi-flow receive
// round of wtp_flows.hip: the leading run of every flow's sub-window goes to one packed
// stream, flow 0's records first, and every flow's window and base move by what was
// delivered for it, all flows in one stream-ordered pass.
//
// Per-flow semantics are those of wtp_deliver.hip and wtp_advance.hip; the state layout is
// that of wtp_flows.hip (flow f owns global slots [f*window, (f+1)*window)).  Nothing is
// done serially per flow: every kernel below spreads the nflows*window global slots (or the
// delivered bytes) over its grid, so 2^20 flows of 16 slots and one flow of 2^20 slots are
// the same work.
//
// deliver, scratch in the caller's d_work (DflowsWork below):
//   k_dflows_init  one lane per flow: run[f] = window ("no slot ends the run")
//   k_dflows_run   one lane per global slot: a wave finds with one ballot the first slot of
//                  every flow it covers whose length ends the run (> WTP_MAX_PAYLOAD), and
//                  only those lanes lower run[f] (k_flows_place's scheme, one atomicMin per
//                  flow and wave at the most)
//   k_dflows_bsum  per 1024-slot block: the number and bytes of the candidates (s <
//                  min(run_f, max_slots)) and of the run slots (s < run_f)
//   k_dflows_mid   one block: the exclusive scan of the <= 16384 block sums, 16 consecutive
//                  entries per lane (1024 * 16 * 1024 = 2^24 slots), bytes in 64 bits; the
//                  totals give d_counts[1], [3] and, when every candidate fits, [0], [2]
//   k_dflows_scan  every block scans its 1024 slots: a candidate gets its rank r and Q_r.
//                  "Delivered" (stream_off + Q_r + len <= stream_bytes) is monotone in r, so
//                  the one candidate with Q_r <= room < Q_r + len is rank K: that lane
//                  writes d_counts[0], [2].  A delivered candidate writes map[r] = its
//                  global slot, Q[r] and its entry of the record arrays; the lane of slot 0
//                  of a flow writes the flow's first rank and Q.  No atomics, no host read.
//   k_dflows_out   one lane per flow: k_f, R_f, B_f and bytes_f from K, the flow's first
//                  rank and Q[]
//   k_dflows_copy  k_deliver_copy's design over the records by rank: one lane per 16-B
//                  destination vector, 4 KiB of the stream per wave and round, the
//                  half-wave owner search in Q[0 .. K] once per round, the round's prefix
//                  sums (relative to its first record's, so 32 bits) and slot numbers in
//                  LDS, widened dword loads shifted by v_alignbyte, spanning vectors merged
//                  in a rolled loop, the first and last vector and the image's edges
//                  bytewise, nt stores.  The source of record r is slot map[r], so a vector
//                  may span records of different flows with empty flows in between.
// advance:
//   k_rx_advance_flows  k_rx_advance's shape over the global slots: a wave takes 64
//                  consecutive destination slots per round, each lane looks up its own
//                  flow's advance, then the ballot walk (four slots per step, 16 lanes per
//                  slot, six vectors per lane for a full slot).  The lane of slot 0 of a
//                  flow writes the flow's next base.
// Every word of d_work that a kernel reads was written by an earlier launch of the same
// call; the calls keep no state and read no library table.
//
// From wtp_common.hpp, with wtp_deliver.hip: the two owner searches (owner, owner_wave).  The
// kernels keep their own bodies, k_rx_advance_flows its copy of copy_slot16's text: on the
// helper its machine code changed and the timing rule did not let it move.
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kFfBlock = 1024;  // slots per block of the scan kernels
constexpr uint32_t kFfWaves = kFfBlock / 64;
constexpr uint32_t kFfPer = 16;      // block sums per lane of k_dflows_mid
static_assert(uint64_t(WTP_RX_MAX_FLOW_SLOTS) <= uint64_t(kFfBlock) * kFfPer * kFfBlock, "k_dflows_mid covers every block");
static_assert(uint64_t(kFfBlock) * WTP_MAX_PAYLOAD < (uint64_t(1) << 32), "a block's bytes fit 32 bits");

constexpr uint32_t kFfCopyBlock = 256;  // four waves, each on its own rounds
constexpr uint32_t kFfCopyWaves = kFfCopyBlock / 64;
constexpr uint32_t kFfVecs = 4;         // 16-B vectors per lane and round
constexpr uint32_t kFfRound = 64 * kFfVecs;  // vectors per wave and round (4 KiB)
constexpr uint32_t kFfMaxBlocks = 2048;  // the capped grid of the copy and of the advance
constexpr uint32_t kFfStage = 256;       // records a wave keeps in LDS per round

static_assert(uint64_t(WTP_RX_MAX_FLOW_SLOTS) + WTP_RX_MAX_WINDOW < (uint64_t(1) << 32), "a source slot fits 32 bits");

__device__ __forceinline__ uint64_t ff_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint64_t ff_shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_up(uint32_t(v), d, 64), hi = __shfl_up(uint32_t(v >> 32), d, 64);
    return (uint64_t(hi) << 32) | lo;
}

// Global slot g: its flow and slot, whether it is in its flow's run and a candidate, and its
// length (0 outside the run, so never a value above WTP_MAX_PAYLOAD).
struct FfSlot {
    uint32_t f, s, len;
    bool inrun, cand;
};
__device__ __forceinline__ FfSlot ff_slot(const uint32_t *__restrict__ slot_len, const uint32_t *__restrict__ run, uint32_t g,
                                          uint32_t slots, uint32_t window, uint32_t max_slots) {
    FfSlot x = {0, 0, 0, false, false};
    if (g >= slots) return x;
    x.f = g / window;
    x.s = g - x.f * window;
    x.inrun = x.s < run[x.f];
    x.cand = x.inrun && x.s < max_slots;
    x.len = x.inrun ? slot_len[g] : 0u;
    return x;
}

__global__ void __launch_bounds__(256)
k_dflows_init(uint32_t nflows, uint32_t window, uint32_t *__restrict__ run, uint32_t *__restrict__ first,
              uint64_t *__restrict__ flow_q) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    run[f] = window;  // k_dflows_run lowers it
    first[f] = 0;     // window == 0: no k_dflows_scan writes them
    flow_q[f] = 0;
}

__global__ void __launch_bounds__(256)
k_dflows_run(const uint32_t *__restrict__ slot_len, uint32_t slots, uint32_t window, uint32_t *run) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool bad = g < slots && slot_len[g] > WTP_MAX_PAYLOAD;
    const uint64_t m = __ballot(bad);
    if (!bad) return;
    // the lanes of this lane's flow in the wave start at lane - min(s, lane): report only if
    // none of them below this one ends the run too
    const uint32_t f = g / window, s = g - f * window;
    const uint32_t from = lane - min(s, lane);
    const uint64_t mine = (m >> from) << from;
    if ((mine & ((uint64_t(1) << lane) - 1)) == 0) atomicMin(&run[f], s);
}

__global__ void __launch_bounds__(kFfBlock)
k_dflows_bsum(const uint32_t *__restrict__ slot_len, const uint32_t *__restrict__ run, uint32_t slots, uint32_t window,
              uint32_t max_slots, u32x4 *__restrict__ bsum) {
    __shared__ uint32_t part[kFfWaves][4];
    const uint32_t t = threadIdx.x;
    const FfSlot x = ff_slot(slot_len, run, blockIdx.x * kFfBlock + t, slots, window, max_slots);
    const uint32_t c = uint32_t(__popcll(__ballot(x.cand))), r = uint32_t(__popcll(__ballot(x.inrun)));
    const uint32_t cb = wave_sum(x.cand ? x.len : 0u), rb = wave_sum(x.len);
    if ((t & 63u) == 0) {
        part[t / 64][0] = c;
        part[t / 64][1] = cb;
        part[t / 64][2] = r;
        part[t / 64][3] = rb;
    }
    __syncthreads();
    if (t == 0) {
        u32x4 a = {0, 0, 0, 0};
        for (uint32_t w = 0; w < kFfWaves; ++w) {
            a.x += part[w][0];
            a.y += part[w][1];
            a.z += part[w][2];
            a.w += part[w][3];
        }
        bsum[blockIdx.x] = a;
    }
}

__global__ void __launch_bounds__(kFfBlock)
k_dflows_mid(const u32x4 *__restrict__ bsum, uint32_t nblk, uint64_t room, uint32_t *__restrict__ bpre_c,
             uint64_t *__restrict__ bpre_q, uint64_t *__restrict__ Q, uint64_t *__restrict__ hdr,
             uint64_t *__restrict__ counts) {
    __shared__ uint32_t w_c[kFfWaves];
    __shared__ uint64_t w_q[kFfWaves], w_rc[kFfWaves], w_rq[kFfWaves];
    const uint32_t t = threadIdx.x, w = t / 64, lane = t & 63u;
    uint32_t c = 0;
    uint64_t q = 0, rc = 0, rq = 0;
    for (uint32_t k = 0; k < kFfPer; ++k) {
        const uint32_t b = t * kFfPer + k;
        if (b < nblk) {
            const u32x4 e = bsum[b];
            c += e.x;
            q += e.y;
            rc += e.z;
            rq += e.w;
        }
    }
    uint32_t inc_c = c;
    uint64_t inc_q = q;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t uc = __shfl_up(inc_c, d, 64);
        const uint64_t uq = ff_shfl_up64(inc_q, d);
        if (lane >= d) {
            inc_c += uc;
            inc_q += uq;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {  // the run totals need no prefix
        rc += (uint64_t(uint32_t(__shfl_xor(uint32_t(rc >> 32), d, 64))) << 32) | uint32_t(__shfl_xor(uint32_t(rc), d, 64));
        rq += (uint64_t(uint32_t(__shfl_xor(uint32_t(rq >> 32), d, 64))) << 32) | uint32_t(__shfl_xor(uint32_t(rq), d, 64));
    }
    if (lane == 63) {
        w_c[w] = inc_c;
        w_q[w] = inc_q;
        w_rc[w] = rc;
        w_rq[w] = rq;
    }
    __syncthreads();
    uint32_t pre_c = 0, all_c = 0;
    uint64_t pre_q = 0, all_q = 0, all_rc = 0, all_rq = 0;
    for (uint32_t k = 0; k < kFfWaves; ++k) {
        if (k < w) {
            pre_c += w_c[k];
            pre_q += w_q[k];
        }
        all_c += w_c[k];
        all_q += w_q[k];
        all_rc += w_rc[k];
        all_rq += w_rq[k];
    }
    uint32_t at_c = pre_c + inc_c - c;  // exclusive: before this lane's first block
    uint64_t at_q = pre_q + inc_q - q;
    for (uint32_t k = 0; k < kFfPer; ++k) {
        const uint32_t b = t * kFfPer + k;
        if (b < nblk) {
            const u32x4 e = bsum[b];
            bpre_c[b] = at_c;
            bpre_q[b] = at_q;
            at_c += e.x;
            at_q += e.y;
        }
    }
    if (t == 0) {
        counts[1] = all_rc;
        counts[3] = all_rq;
        Q[all_c] = all_q;  // the end of the last candidate
        if (all_q <= room) {  // every candidate fits; otherwise the lane of rank K in k_dflows_scan writes these
            counts[0] = all_c;
            counts[2] = all_q;
            hdr[0] = all_c;
            hdr[1] = all_q;
        }
    }
}

__global__ void __launch_bounds__(kFfBlock)
k_dflows_scan(const uint32_t *__restrict__ slot_len, const uint32_t *__restrict__ run, uint32_t slots, uint32_t window,
              uint32_t max_slots, uint64_t stream_off, uint64_t room, const uint32_t *__restrict__ bpre_c,
              const uint64_t *__restrict__ bpre_q, uint32_t *__restrict__ map, uint64_t *__restrict__ Q,
              uint32_t *__restrict__ first, uint64_t *__restrict__ flow_q, uint64_t *__restrict__ hdr,
              uint64_t *__restrict__ offs_out, uint32_t *__restrict__ lens_out, uint64_t *__restrict__ counts) {
    __shared__ uint32_t w_c[kFfWaves], w_b[kFfWaves];
    const uint32_t t = threadIdx.x, g = blockIdx.x * kFfBlock + t, w = t / 64, lane = t & 63u;
    const FfSlot x = ff_slot(slot_len, run, g, slots, window, max_slots);
    const uint64_t bal = __ballot(x.cand);
    const uint32_t v = x.cand ? x.len : 0u;
    uint32_t inc = v;  // inclusive prefix sum over the wave
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) {
        w_c[w] = uint32_t(__popcll(bal));
        w_b[w] = inc;
    }
    __syncthreads();
    uint32_t r = bpre_c[blockIdx.x], pb = 0;
    for (uint32_t k = 0; k < w; ++k) {
        r += w_c[k];
        pb += w_b[k];
    }
    r += __builtin_amdgcn_mbcnt_hi(uint32_t(bal >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bal), 0u));
    const uint64_t q = bpre_q[blockIdx.x] + pb + (inc - v);  // the candidates before this slot: their number r, their bytes q
    if (g >= slots) return;
    if (x.s == 0) {
        first[x.f] = r;
        flow_q[x.f] = q;
    }
    if (!x.cand) return;
    if (q + x.len <= room) {  // room = stream_bytes - stream_off
        map[r] = g;
        Q[r] = q;
        if (offs_out) offs_out[r] = stream_off + q;
        if (lens_out) lens_out[r] = x.len;
    } else if (q <= room) {
        // the predicate is monotone in r: the candidate before this one fits (or there is none), so this is rank K
        Q[r] = q;
        counts[0] = r;
        counts[2] = q;
        hdr[0] = r;
        hdr[1] = q;
    }
}

__global__ void __launch_bounds__(256)
k_dflows_out(uint32_t nflows, uint32_t max_slots, uint64_t stream_off, const uint32_t *__restrict__ run,
             const uint32_t *__restrict__ first, const uint64_t *__restrict__ flow_q, const uint64_t *__restrict__ Q,
             const uint64_t *__restrict__ hdr, uint64_t *__restrict__ adv, uint64_t *__restrict__ info) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    const uint64_t K = hdr[0], QK = hdr[1];
    const uint32_t rn = run[f], cf = min(rn, max_slots), fr = first[f];
    // ranks [R, end) are the flow's delivered records.  No difference under a condition here: the compiler
    // took `fr < K ? K - fr : 0` as a promise that K >= fr and dropped the min below
    const uint64_t R = ff_min64(fr, K), end = ff_min64(uint64_t(fr) + cf, K);  // end >= R
    const uint64_t kf = end > R ? end - R : 0;
    adv[f] = kf;
    if (!info) return;
    info[4 * uint64_t(f) + 0] = rn;
    info[4 * uint64_t(f) + 1] = R;
    // the flows before it delivered all of theirs (R == fr: Q of its first candidate), or the cut is before it
    const uint64_t at = R == fr ? flow_q[f] : QK;
    info[4 * uint64_t(f) + 2] = stream_off + at;
    info[4 * uint64_t(f) + 3] = Q[end > R ? end : R] - Q[R];
}

// Delivered bytes [b0, b1) of the round (relative to its first record's Q), b1 - b0 <= 16, as
// bytes [skip, skip + b1 - b0) of a vector, piece by piece: a piece is what one record gives to
// the vector, from one widened load of the 16 source bytes that put it at its place (the bytes
// around it are masked off); where that load would leave the image, or the image is not 4-B
// aligned, from its own bytes one by one.  o owns b0; p(i) = Q[i] relative, m(i) = map[i].
template <class Get, class Map>
__device__ __forceinline__ u32x4 ff_merge(const uint8_t *__restrict__ img, uint64_t img_bytes, uint32_t vec, Get p, Map m,
                                          uint32_t o, uint32_t b0, uint32_t b1, uint32_t skip) {
    uint64_t lo = 0, hi = 0;
    uint32_t cur = p(o), nxt = p(o + 1);
    uint32_t j = b0;
    while (j < b1) {
        while (j >= nxt) {  // the next record with a byte: j < Q[K], so o + 1 <= K
            ++o;
            cur = nxt;
            nxt = p(o + 1);
        }
        const uint32_t end = min(nxt, b1), pos = skip + (j - b0), nb = end - j;  // bytes [pos, pos + nb) of the vector
        const uint64_t x = uint64_t(m(o)) * WTP_MAX_PAYLOAD + (j - cur);          // the image byte of j
        const uint64_t s = x - pos;
        const uint32_t sh = uint32_t(s) & 3u;
        const uint64_t a = s - sh;
        uint64_t vlo = 0, vhi = 0;
        if (vec && x >= pos && a + (sh ? 20u : 16u) <= img_bytes) {
            const u32x4 d = *reinterpret_cast<const u32x4_a4 *>(img + a);
            const uint32_t e = *reinterpret_cast<const uint32_t *>(img + a + (sh ? 16 : 12));
            vlo = (uint64_t(__builtin_amdgcn_alignbyte(d.z, d.y, sh)) << 32) | __builtin_amdgcn_alignbyte(d.y, d.x, sh);
            vhi = (uint64_t(__builtin_amdgcn_alignbyte(e, d.w, sh)) << 32) | __builtin_amdgcn_alignbyte(d.w, d.z, sh);
        } else {
#pragma clang loop unroll(disable)
            for (uint32_t k = 0; k < nb; ++k) {
                const uint64_t byte = img[x + k];
                if (pos + k < 8)
                    vlo |= byte << (8 * (pos + k));
                else
                    vhi |= byte << (8 * (pos + k - 8));
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

__global__ void __launch_bounds__(kFfCopyBlock)
k_dflows_copy(const uint8_t *__restrict__ img, uint64_t img_bytes, uint32_t vec, const uint64_t *__restrict__ Q,
              const uint32_t *__restrict__ map, const uint64_t *__restrict__ hdr, uint8_t *__restrict__ dst, uint32_t ph) {
    __shared__ uint32_t s_P[kFfCopyWaves][kFfStage], s_M[kFfCopyWaves][kFfStage];
    // dst = A, the 16-B boundary at or below the first delivered byte, which is dst[ph]
    const uint32_t K = uint32_t(hdr[0]);
    const uint64_t total = hdr[1];
    if (total == 0) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x / 64;
    const uint32_t nvec = uint32_t((ph + total + 15) / 16);  // total <= 2^24 * 1456
    const uint32_t rounds = (nvec + kFfRound - 1) / kFfRound, step_r = gridDim.x * kFfCopyWaves;
    for (uint32_t r = blockIdx.x * kFfCopyWaves + wv; r < rounds; r += step_r) {
        const uint32_t v0 = r * kFfRound;
        // the records this round's bytes come from: between the owners of its first and last byte
        const uint64_t fb = 16 * uint64_t(v0) > ph ? 16 * uint64_t(v0) - ph : 0u;
        const uint64_t lb = ff_min64(16 * (uint64_t(v0) + kFfRound) - ph, total) - 1;
        const uint32_t edge = owner_wave(Q, K, lane < 32 ? fb : lb, lane);
        const uint32_t olo = __shfl(edge, 0, 64), ohi = __shfl(edge, 63, 64);
        // everything below is relative to the first record's Q: the round's bytes and the
        // records' ends are within 4 KiB + 1456 of it
        const uint64_t base = Q[olo];
        const uint32_t cnt = ohi - olo + 2;
        const bool staged = cnt <= kFfStage;
        if (staged)
            for (uint32_t i = lane; i < cnt; i += 64) {
                s_P[wv][i] = uint32_t(Q[olo + i] - base);
                if (i + 1 < cnt) s_M[wv][i] = map[olo + i];
            }
        wave_sync();
        // the round over p(i) and m(i): from LDS, or from memory (two bodies: one address space each)
        auto body = [&](auto p, auto m) {
        uint32_t b0[kFfVecs], b1[kFfVecs], own[kFfVecs], sh[kFfVecs];
        uint64_t soff[kFfVecs];
        bool fast[kFfVecs];
#pragma unroll
        for (uint32_t u = 0; u < kFfVecs; ++u) {
            const uint64_t v = uint64_t(v0) + 64 * u + lane;
            const uint64_t a0 = 16 * v > ph ? 16 * v - ph : 0u;
            const uint64_t a1 = v < nvec ? ff_min64(16 * v + 16 - ph, total) : 0u;
            const bool any = a0 < a1;  // a0 >= fb >= base
            b0[u] = any ? uint32_t(a0 - base) : 0u;
            b1[u] = any ? uint32_t(a1 - base) : 0u;
            own[u] = 0;
            sh[u] = 0;
            soff[u] = 0;
            fast[u] = false;
            if (any) {
                own[u] = owner(p, olo, ohi, b0[u]);
                const uint64_t x = uint64_t(m(own[u])) * WTP_MAX_PAYLOAD + (b0[u] - p(own[u]));
                sh[u] = uint32_t(x) & 3u;
                soff[u] = x - sh[u];
                // whole, inside one record, and the widened load inside the image
                fast[u] = vec && b1[u] - b0[u] == 16 && b0[u] + 16 <= p(own[u] + 1) &&
                          soff[u] + (sh[u] ? 20u : 16u) <= img_bytes;
            }
        }
        u32x4 d[kFfVecs] = {};
        uint32_t e[kFfVecs] = {};
#pragma unroll
        for (uint32_t u = 0; u < kFfVecs; ++u)
            if (fast[u]) {
                const uint8_t *q = img + soff[u];  // the dword that holds the first byte
                d[u] = *reinterpret_cast<const u32x4_a4 *>(q);
                e[u] = *reinterpret_cast<const uint32_t *>(q + (sh[u] ? 16 : 12));  // sh == 0: d.w again, unused
            }
        uint32_t slow = 0;  // the vectors that are not one whole load: one after the other, in one body
#pragma unroll
        for (uint32_t u = 0; u < kFfVecs; ++u) {
            if (fast[u]) {
                u32x4 val;
                val.x = __builtin_amdgcn_alignbyte(d[u].y, d[u].x, sh[u]);
                val.y = __builtin_amdgcn_alignbyte(d[u].z, d[u].y, sh[u]);
                val.z = __builtin_amdgcn_alignbyte(d[u].w, d[u].z, sh[u]);
                val.w = __builtin_amdgcn_alignbyte(e[u], d[u].w, sh[u]);
                __builtin_nontemporal_store(val, reinterpret_cast<u32x4 *>(dst + 16 * (uint64_t(v0) + 64 * u + lane)));
            } else if (b0[u] < b1[u]) {
                slow |= 1u << u;
            }
        }
        static_assert(kFfVecs == 4, "the selects below");
        while (slow) {
            const uint32_t u = __builtin_ctz(slow);
            slow &= slow - 1;
            const uint32_t c0 = u == 0 ? b0[0] : u == 1 ? b0[1] : u == 2 ? b0[2] : b0[3];
            const uint32_t c1 = u == 0 ? b1[0] : u == 1 ? b1[1] : u == 2 ? b1[2] : b1[3];
            const uint32_t o = u == 0 ? own[0] : u == 1 ? own[1] : u == 2 ? own[2] : own[3];
            const uint64_t v = uint64_t(v0) + 64 * u + lane;
            uint8_t *at = dst + 16 * v;
            // the vector's first delivered byte is byte `skip` of it (> 0 only in the stream's first vector)
            const uint32_t skip = uint32_t(base + c0 + ph - 16 * v);
            const u32x4 val = ff_merge(img, img_bytes, vec, p, m, o, c0, c1, skip);
            if (c1 - c0 == 16) {
                __builtin_nontemporal_store(val, reinterpret_cast<u32x4 *>(at));
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
        const uint32_t *sp = s_P[wv], *sm = s_M[wv];
        if (staged)
            body([&](uint32_t i) { return sp[i - olo]; }, [&](uint32_t i) { return sm[i - olo]; });
        else
            body([&](uint32_t i) { return uint32_t(Q[i] - base); }, [&](uint32_t i) { return map[i]; });
        wave_sync();  // the next round's LDS stores follow these loads
    }
}

// eight waves per SIMD, as k_rx_advance: bound, the six vectors of a full slot do not spread
__global__ void __launch_bounds__(256, 8)
k_rx_advance_flows(const uint8_t *__restrict__ img, const uint32_t *__restrict__ slot_len, uint32_t slots, uint32_t window,
                   const uint64_t *__restrict__ flow_adv, const uint32_t *__restrict__ seq0, uint8_t *__restrict__ img_next,
                   uint32_t *__restrict__ slot_len_next, uint32_t *__restrict__ seq0_next, uint32_t vec) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x / 64, g = lane % kGroup, q = lane / kGroup;
    const uint32_t rounds = (slots + 63) / 64, step = gridDim.x * 4;
    for (uint32_t r = blockIdx.x * 4 + wv; r < rounds; r += step) {
        const uint32_t gs = r * 64 + lane;
        uint32_t v = WTP_SLOT_EMPTY, a = 0;
        if (gs < slots) {
            const uint32_t f = gs / window, s = gs - f * window;
            const uint64_t by = flow_adv[f];
            a = by < window ? uint32_t(by) : window;
            if (s + a < window) v = slot_len[gs + a];
            slot_len_next[gs] = v;  // every value as it is
            if (s == 0 && seq0) seq0_next[f] = seq0[f] + a;
        }
        // the slots with bytes to move (a lane past the state holds EMPTY), four per step
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
            const uint32_t by = __shfl(a, pick & 63u, 64);
            if (pick == 64) continue;
            const uint32_t sd = r * 64 + pick;
            const uint8_t *src = img + uint64_t(sd + by) * WTP_MAX_PAYLOAD;
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
                    for (uint32_t k = 0; k + 1 < kSlotVecs; ++k) vd[g + k * kGroup] = w[k];
                    if (last) vd[g + (kSlotVecs - 1) * kGroup] = w[kSlotVecs - 1];
                } else {
                    // a shorter one: a Zipf record is a vector or two per lane
#pragma clang loop unroll_count(2)
                    for (uint32_t x = g; x < nvec; x += kGroup) vd[x] = vs[x];
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

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_rx_deliver_flows, from the first 16-B boundary on: hdr[2] = {K, Q_K} (u64),
// bsum[nblk] (4 x u32), Q[slots + 1] (u64), bpre_q[nblk] (u64), flow_q[nflows] (u64),
// map[slots], bpre_c[nblk], run[nflows], first[nflows] (u32).
struct DflowsWork {
    uint32_t nblk;
    uint64_t *hdr, *Q, *bpre_q, *flow_q;
    wtp::dev::u32x4 *bsum;
    uint32_t *map, *bpre_c, *run, *first;
    size_t bytes;
};

DflowsWork dflows_layout(void *d_work, uint32_t nflows, uint32_t slots) {
    DflowsWork w;
    wtp::Work l(d_work, 16);
    w.nblk = (slots + wtp::dev::kFfBlock - 1) / wtp::dev::kFfBlock;
    w.hdr = l.take<uint64_t>(2);
    w.bsum = l.take<wtp::dev::u32x4>(w.nblk);
    w.Q = l.take<uint64_t>(size_t(slots) + 1);
    w.bpre_q = l.take<uint64_t>(w.nblk);
    w.flow_q = l.take<uint64_t>(nflows);
    w.map = l.take<uint32_t>(slots);
    w.bpre_c = l.take<uint32_t>(w.nblk);
    w.run = l.take<uint32_t>(nflows);
    w.first = l.take<uint32_t>(nflows);
    w.bytes = l.bytes();
    return w;
}

}  // namespace

extern "C" size_t wtp_rx_deliver_flows_work_bytes(uint32_t nflows, uint32_t window) {
    const uint32_t f = std::min<uint32_t>(nflows, WTP_RX_MAX_FLOWS), w = std::min<uint32_t>(window, WTP_RX_MAX_WINDOW);
    return dflows_layout(nullptr, f, uint32_t(std::min<uint64_t>(uint64_t(f) * w, WTP_RX_MAX_FLOW_SLOTS))).bytes;
}

extern "C" int wtp_rx_deliver_flows(const void *d_img, const uint32_t *d_slot_len, uint32_t nflows, uint32_t window,
                                    uint32_t max_slots, void *d_stream, size_t stream_bytes, uint64_t stream_off,
                                    uint64_t *d_offsets_out, uint32_t *d_lengths_out, uint64_t *d_flow_adv,
                                    uint64_t *d_flow_info, uint64_t *d_counts, void *d_work, size_t work_bytes,
                                    void *stream) {
    using namespace wtp;
    int rc = check_flows(nflows, window);
    if (rc) return rc;
    if (stream_off > stream_bytes)
        return fail(WTP_EINVAL, "stream_off %llu > stream_bytes %zu", static_cast<unsigned long long>(stream_off), stream_bytes);
    const uint32_t slots = nflows * window;
    const DflowsWork w = dflows_layout(d_work, nflows, slots);
    if ((rc = check_work_bytes(work_bytes, w.bytes))) return rc;
    if (!d_counts) return null_arg("d_counts");
    if (!d_work) return null_arg("d_work");
    if (nflows > 0 && !d_flow_adv) return fail(WTP_EINVAL, "null pointer: d_flow_adv with nflows %u", nflows);
    if (slots > 0) {
        if (!d_img) return fail(WTP_EINVAL, "null pointer: d_img with %u slots", slots);
        if (!d_slot_len) return fail(WTP_EINVAL, "null pointer: d_slot_len with %u slots", slots);
        if (max_slots > 0 && !d_stream)
            return fail(WTP_EINVAL, "null pointer: d_stream with %u slots and max_slots %u", slots, max_slots);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t room = uint64_t(stream_bytes) - stream_off;
    const unsigned fblocks = (nflows + 255) / 256;
    if (nflows > 0) {
        rc = launch("k_dflows_init", dev::k_dflows_init, dim3(fblocks), dim3(256), st, nflows, window, w.run, w.first, w.flow_q);
        if (rc) return rc;
    }
    if (slots > 0) {
        rc = launch("k_dflows_run", dev::k_dflows_run, dim3((slots + 255) / 256), dim3(256), st, d_slot_len, slots, window, w.run);
        if (rc) return rc;
        rc = launch("k_dflows_bsum", dev::k_dflows_bsum, dim3(w.nblk), dim3(dev::kFfBlock), st, d_slot_len, w.run, slots, window,
                    max_slots, w.bsum);
        if (rc) return rc;
    }
    // no slots: the one block only writes d_counts = {0, 0, 0, 0}
    rc = launch("k_dflows_mid", dev::k_dflows_mid, dim3(1), dim3(dev::kFfBlock), st, w.bsum, w.nblk, room, w.bpre_c, w.bpre_q,
                w.Q, w.hdr, d_counts);
    if (rc) return rc;
    if (slots > 0) {
        rc = launch("k_dflows_scan", dev::k_dflows_scan, dim3(w.nblk), dim3(dev::kFfBlock), st, d_slot_len, w.run, slots, window,
                    max_slots, stream_off, room, w.bpre_c, w.bpre_q, w.map, w.Q, w.first, w.flow_q, w.hdr, d_offsets_out,
                    d_lengths_out, d_counts);
        if (rc) return rc;
    }
    if (nflows > 0) {
        rc = launch("k_dflows_out", dev::k_dflows_out, dim3(fblocks), dim3(256), st, nflows, max_slots, stream_off, w.run,
                    w.first, w.flow_q, w.Q, w.hdr, d_flow_adv, d_flow_info);
        if (rc) return rc;
    }
    if (slots == 0 || max_slots == 0) return WTP_OK;
    // the grid from what the arguments allow, never from d_counts: min(window, max_slots) full
    // slots per flow, capped; a workgroup leaves at once when the scan delivered fewer bytes
    const uintptr_t dst0 = reinterpret_cast<uintptr_t>(d_stream) + stream_off;
    const uint32_t ph = uint32_t(dst0 & 15u);
    const uint64_t most = uint64_t(nflows) * std::min(window, max_slots) * WTP_MAX_PAYLOAD + ph;
    const uint64_t per = 16 * dev::kFfRound * dev::kFfCopyWaves;
    const unsigned blocks = unsigned(std::min<uint64_t>((most + per - 1) / per, dev::kFfMaxBlocks));
    const uint32_t vec = (reinterpret_cast<uintptr_t>(d_img) & 3u) == 0;
    return launch("k_dflows_copy", dev::k_dflows_copy, dim3(blocks), dim3(dev::kFfCopyBlock), st,
                  static_cast<const uint8_t *>(d_img), uint64_t(slots) * WTP_MAX_PAYLOAD, vec, w.Q, w.map, w.hdr,
                  reinterpret_cast<uint8_t *>(dst0 - ph), ph);
}

extern "C" int wtp_rx_advance_flows(const void *d_img, const uint32_t *d_slot_len, uint32_t nflows, uint32_t window,
                                    const uint64_t *d_flow_adv, const uint32_t *d_seq0, void *d_img_next,
                                    uint32_t *d_slot_len_next, uint32_t *d_seq0_next, void *stream) {
    using namespace wtp;
    int rc = check_flows(nflows, window);
    if (rc) return rc;
    if (!d_img != !d_img_next)
        return fail(WTP_EINVAL, "null pointer: %s without %s", d_img ? "d_img_next" : "d_img", d_img ? "d_img" : "d_img_next");
    if (!d_seq0 != !d_seq0_next)
        return fail(WTP_EINVAL, "null pointer: %s without %s", d_seq0 ? "d_seq0_next" : "d_seq0",
                    d_seq0 ? "d_seq0" : "d_seq0_next");
    const uint32_t slots = nflows * window;
    if (slots == 0) return WTP_OK;
    if (!d_flow_adv) return fail(WTP_EINVAL, "null pointer: d_flow_adv with %u slots", slots);
    if (!d_slot_len) return fail(WTP_EINVAL, "null pointer: d_slot_len with %u slots", slots);
    if (!d_slot_len_next) return fail(WTP_EINVAL, "null pointer: d_slot_len_next with %u slots", slots);
    if (overlap(d_slot_len, d_slot_len_next, uint64_t(slots) * 4))
        return fail(WTP_EINVAL, "d_slot_len_next overlaps d_slot_len (%u slots)", slots);
    if (d_img && overlap(d_img, d_img_next, uint64_t(slots) * WTP_MAX_PAYLOAD))
        return fail(WTP_EINVAL, "d_img_next overlaps d_img (%u slots)", slots);
    if (d_seq0 && overlap(d_seq0, d_seq0_next, uint64_t(nflows) * 4))
        return fail(WTP_EINVAL, "d_seq0_next overlaps d_seq0 (nflows %u)", nflows);
    // the grid from the state's size, never from d_flow_adv
    const uint32_t groups = ((slots + 63) / 64 + 3) / 4;
    const unsigned blocks = std::min(groups, dev::kFfMaxBlocks);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(d_img) | reinterpret_cast<uintptr_t>(d_img_next)) & 15u) == 0;
    return launch("k_rx_advance_flows", dev::k_rx_advance_flows, dim3(blocks), dim3(256), static_cast<hipStream_t>(stream),
                  static_cast<const uint8_t *>(d_img), d_slot_len, slots, window, d_flow_adv, d_seq0,
                  static_cast<uint8_t *>(d_img_next), d_slot_len_next, d_seq0_next, vec);
}
