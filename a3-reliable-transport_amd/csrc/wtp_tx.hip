// wtp_tx.hip — device-side sender window (include/wtp_crc32.h: wtp_tx_ingest_acks,
// wtp_tx_build_retransmit, wtp_tx_build_retransmit_var), the mirror of wtp_accept.hip.
//
// The window state (d_acked[inflight], d_sent_ms[inflight]) is the caller's and persists
// across calls.  Semantics: the reference's selective-repeat sender, cpp/src/opt/
// Sender.cpp:130-139 (one ACK marks one packet, Window.cpp:45-54; the window advances over
// the leading ACKed packets, Window.cpp:66-75) and :121-127 (on a timeout resend what is
// un-ACKed and older than the timeout, Packet.cpp:52-56), and the go-back-N sender,
// cpp/src/base/Sender.cpp:101-109 (an ACK names the next expected packet; a timeout
// resends the whole window).
//
// wtp_tx_ingest_acks, stream-ordered, no scratch (d_counts is the only accumulator):
//   memset          d_counts <- {0, 0}
//   k_tx_ingest     one lane per datagram: ok (a 16-byte ACK is decided inline, its payload
//                   is empty and crc32("") = 0; a longer one is hashed by its lane), type
//                   and window check, d_hit.  Selective: atomicCAS(&acked[s], 0, 1), the
//                   old value makes the 0 -> 1 count exact under duplicates (d_counts[1]);
//                   lane 0 sets d_counts[0] = inflight ("no un-ACKed slot").
//                   Cumulative: atomicMax(&d_counts[1], a).
//   k_tx_lead       selective mode, after all marks, as accept's place pass follows its
//                   claim pass: every lane walks its share of d_acked in rising order up
//                   to its first un-ACKed slot; one atomicMin per wave lowers d_counts[0].
//   k_tx_window     cumulative mode, one workgroup: fill of slots [0, max a) with its
//                   0 -> 1 count, then the leading-run scan, which stops at the first
//                   un-ACKed slot.  d_counts holds three quantities over such a call (max
//                   a, the 0 -> 1 count, the run), so the pass that trades one for another
//                   is a single workgroup: it reads max a, synchronises, and only then
//                   overwrites it.
//
// wtp_tx_build_retransmit, stream-ordered, scratch in the caller's d_work:
//   k_tx_count      the due predicate per slot, wave64 ballot + popcount -> a count per
//                   1024-slot block
//   k_tx_select     every block sums the counts before it (<= 1024 of them), recomputes its
//                   predicate and ranks its due slots: an ordered compaction.  Rank k <
//                   max_sel: sel[k] (in d_work, and in d_sel), timer reset; d_counts.
//   k_tx_emit       16 lanes per datagram, fused CRC and copy: a lane loads its 96
//                   contiguous payload bytes once (six 16-B vectors), stores them into the
//                   wire slot and hashes them from registers (slice-by-4, tables in LDS);
//                   the 16 partial CRCs combine as crc_g * x^(8 * bytes after segment g)
//                   (crc32_combine.hpp), the multipliers of a full chunk being constants.
//                   A first version ran wtp_crc32_batch_var over the selection and then a
//                   copy pass: the general kernel, which gives every wave 64 payloads, took
//                   0.14 ms for 658 payloads and 65 - 93 % of the call (DESIGN.md 3.6,
//                   profiles/retx/retx_bench_twopass.json).
//                   A chunk shorter than 1456 B (at most the window's last) and buffers
//                   that are not 16-B aligned go bytewise, same segments, same result.
// wtp_tx_build_retransmit_var, the same window over records of mixed length (base, offsets,
// lengths: wtp_build_data_packets_var's layout), the same d_work:
//   k_tx_count, k_tx_select   as above, unchanged: the selection does not look at the records
//   k_tx_emit_var   wtp_txvar.hip, its own translation unit so that the kernels here keep
//                   their machine code: the builder's move-and-hash body behind the
//                   selection, launched through tx_emit_var_launch.
// The selection is ordered because the reference walks its deque front to back, and a
// ring shorter than the due set must hold the oldest packets; it is counted on the device
// because the host never reads d_counts[0]: grids are sized from max_sel.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_crc_dev.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kTxBlock = 1024;  // slots per block of the count / select passes
constexpr uint32_t kTxWaves = kTxBlock / 64;
constexpr uint32_t kTxGroup = 16;    // lanes per datagram in k_tx_emit
constexpr uint32_t kTxVecs = (WTP_MAX_PAYLOAD / 16 + kTxGroup - 1) / kTxGroup;  // 91 vectors -> 6 per lane
constexpr uint32_t kTxSeg = kTxVecs * 16;  // a lane's contiguous segment: 96 B (lane 15: 16 B)
static_assert(kTxSeg * (kTxGroup - 1) < WTP_MAX_PAYLOAD && kTxSeg * kTxGroup >= WTP_MAX_PAYLOAD, "segments");
constexpr uint32_t kTxScan = 16;     // slots per lane and round of k_tx_window's scan

__device__ const SliceTable g_tx_table{};  // this unit's own object of the shared type (wtp_crc_dev.hpp)

// x^(8 * bytes after segment g) of a full 1456-B chunk
struct TxTail {
    uint32_t v[kTxGroup];
    constexpr TxTail() : v{} {
        for (uint32_t g = 0; g < kTxGroup; ++g) {
            const uint32_t end = kTxSeg * (g + 1) < WTP_MAX_PAYLOAD ? kTxSeg * (g + 1) : WTP_MAX_PAYLOAD;
            v[g] = gf::xpow8(WTP_MAX_PAYLOAD - end);
        }
    }
};
__device__ const TxTail g_tx_tail{};

// ---- ACK ingest ----------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_tx_ingest(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len, uint64_t n,
            uint32_t mode, uint32_t seq0, uint32_t inflight, uint32_t *acked, uint8_t *__restrict__ ok,
            uint32_t *__restrict__ hit, uint32_t *counts) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    uint32_t fresh = 0, amax = 0;
    if (i == 0 && mode == WTP_ACK_SELECTIVE) counts[0] = inflight;  // k_tx_lead lowers it
    if (i < n) {
        const uint32_t rl = recv_len[i];
        const uint8_t *h = ring + i * stride;
        bool good = rl >= WTP_HEADER_BYTES && rl <= stride && rl - WTP_HEADER_BYTES <= WTP_MAX_KERNEL_LEN;
        Header hd{};
        if (good) {
            hd = load_header(h);  // type, seq, sum
            uint32_t c = 0;  // the CRC of the empty payload: a plain ACK is decided here
            if (rl > WTP_HEADER_BYTES) {
                c = 0xFFFFFFFFu;
                for (uint32_t b = WTP_HEADER_BYTES; b < rl; ++b) c = g_tx_table.t[0][(c ^ h[b]) & 0xFFu] ^ (c >> 8);
                c ^= 0xFFFFFFFFu;
            }
            good = hd.sum == c;
        }
        ok[i] = good ? 1 : 0;
        uint32_t where = WTP_NOT_PLACED;
        if (good && hd.type == WTP_TYPE_ACK) {
            const uint32_t d = hd.seq - seq0;  // unsigned: a wrapping window is well defined
            if (mode == WTP_ACK_SELECTIVE) {
                if (d < inflight) {
                    where = d;
                    fresh = atomicCAS(&acked[d], 0u, 1u) == 0u;
                }
            } else if (d > 0 && d <= inflight) {
                where = d;
                amax = d;
            }
        }
        if (hit) hit[i] = where;
    }
    // one atomic per wave
    if (mode == WTP_ACK_SELECTIVE) {
        const uint32_t sum = wave_sum(fresh);
        if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&counts[1], sum);
    } else {
        const uint32_t m = wave_max(amax);
        if ((threadIdx.x & 63u) == 0 && m) atomicMax(&counts[1], m);
    }
}

// Selective mode: counts[0] (= inflight on entry) becomes the first un-ACKed slot.  A lane
// stops at its first un-ACKed slot, or once it is past a lower one already published.
__global__ void __launch_bounds__(256)
k_tx_lead(uint32_t inflight, const uint32_t *__restrict__ acked, uint32_t *counts) {
    const uint32_t step = gridDim.x * blockDim.x;
    uint32_t mine = inflight;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < inflight; s += step) {
        if (s >= __hip_atomic_load(&counts[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        if (acked[s] == 0) {
            mine = s;
            break;
        }
    }
    mine = wave_min(mine);
    if ((threadIdx.x & 63u) == 0 && mine < __hip_atomic_load(&counts[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&counts[0], mine);
}

// One workgroup, cumulative mode (exact in selective mode too): counts[1] holds max a on
// entry; slots [0, max a) are filled and counts[1] becomes the 0 -> 1 count; counts[0] = the
// leading run.
__global__ void __launch_bounds__(kTxBlock)
k_tx_window(uint32_t mode, uint32_t inflight, uint32_t *acked, uint32_t *counts) {
    __shared__ uint32_t part[kTxWaves];
    __shared__ uint32_t first;
    const uint32_t t = threadIdx.x;
    uint32_t start = 0;
    if (mode == WTP_ACK_CUMULATIVE) {
        const uint32_t top = min(counts[1], inflight);  // <= inflight by construction
        uint32_t fresh = 0;
        for (uint32_t s = t; s < top; s += kTxBlock)
            if (acked[s] == 0) {
                acked[s] = 1;
                ++fresh;
            }
        fresh = wave_sum(fresh);
        if ((t & 63u) == 0) part[t / 64] = fresh;
        __syncthreads();  // every lane has read counts[1] and stored its slots
        if (t == 0) {
            uint32_t sum = 0;
            for (uint32_t w = 0; w < kTxWaves; ++w) sum += part[w];
            counts[1] = sum;
        }
        start = top;  // slots below are ACKed now
    }
    // leading run: rounds of kTxScan * kTxBlock slots from `start`, until a round holds an
    // un-ACKed slot; a lane's loads of one round are independent
    for (uint32_t base = start;; base += kTxScan * kTxBlock) {
        if (t == 0) first = inflight;
        __syncthreads();
        uint32_t mine = inflight;
#pragma unroll
        for (uint32_t k = kTxScan; k-- > 0;) {
            const uint64_t s = uint64_t(base) + k * kTxBlock + t;
            if (s < inflight && acked[s] == 0) mine = uint32_t(s);
        }
        if (mine < inflight) atomicMin(&first, mine);
        __syncthreads();
        const uint32_t f = first;
        __syncthreads();  // `first` is reset at the top of the next round
        if (f < inflight || uint64_t(base) + kTxScan * kTxBlock >= inflight) {
            if (t == 0) counts[0] = f;
            return;
        }
    }
}

// ---- retransmit selection --------------------------------------------------------------

__device__ __forceinline__ bool tx_due(const uint32_t *acked, const uint32_t *sent, uint32_t s, uint32_t inflight,
                                       uint32_t now, uint32_t timeout, uint32_t flags) {
    if (s >= inflight || acked[s] != 0) return false;
    return (flags & WTP_RETX_ALL) || uint32_t(now - sent[s]) > timeout;
}

__global__ void __launch_bounds__(kTxBlock)
k_tx_count(const uint32_t *__restrict__ acked, const uint32_t *__restrict__ sent, uint32_t inflight, uint32_t now,
           uint32_t timeout, uint32_t flags, uint32_t *__restrict__ blk) {
    __shared__ uint32_t part[kTxWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kTxBlock + t;
    const bool due = tx_due(acked, sent, s, inflight, now, timeout, flags);
    const uint64_t b = __ballot(due);
    if ((t & 63u) == 0) part[t / 64] = uint32_t(__popcll(b));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kTxWaves; ++w) sum += part[w];
        blk[blockIdx.x] = sum;
    }
}

// Block b ranks its due slots from sum(blk[0 .. b)); nblk <= kTxBlock, one count per lane.
// picked[max_sel] is the selection in d_work (d_sel may be NULL), max_sel <= inflight.
__global__ void __launch_bounds__(kTxBlock)
k_tx_select(const uint32_t *__restrict__ acked, uint32_t *sent, uint32_t inflight, uint32_t now, uint32_t timeout,
            uint32_t flags, const uint32_t *__restrict__ blk, uint32_t nblk, uint32_t max_sel,
            uint32_t *__restrict__ sel, uint32_t *__restrict__ picked, uint32_t *__restrict__ counts) {
    __shared__ uint32_t before[kTxWaves], all[kTxWaves], wave_due[kTxWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kTxBlock + t, w = t / 64, lane = t & 63u;
    const uint32_t c = t < nblk ? blk[t] : 0;
    const uint32_t sum_before = wave_sum(t < blockIdx.x ? c : 0), sum_all = wave_sum(c);
    const bool due = tx_due(acked, sent, s, inflight, now, timeout, flags);
    const uint64_t ballot = __ballot(due);
    if (lane == 0) {
        before[w] = sum_before;
        all[w] = sum_all;
        wave_due[w] = uint32_t(__popcll(ballot));
    }
    __syncthreads();
    uint32_t rank = 0, total = 0;
    for (uint32_t k = 0; k < kTxWaves; ++k) {
        rank += before[k] + (k < w ? wave_due[k] : 0);
        total += all[k];
    }
    rank += uint32_t(__popcll(ballot & ((uint64_t(1) << lane) - 1)));
    if (due && rank < max_sel) {
        if (sel) sel[rank] = s;
        picked[rank] = s;
        sent[s] = now;
    }
    if (s == 0) {
        counts[0] = min(total, max_sel);
        counts[1] = total;
    }
}

// ---- retransmit emit ---------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_tx_emit(const uint8_t *__restrict__ pay, uint64_t total_bytes, uint32_t seq0, const uint32_t *__restrict__ picked,
          const uint32_t *__restrict__ counts, uint32_t max_sel, uint8_t *__restrict__ wire, uint64_t stride,
          uint32_t *__restrict__ wire_len) {
    __shared__ uint32_t tab[4 * 256];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) tab[i] = (&g_tx_table.t[0][0])[i];
    __syncthreads();
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t k = t / kTxGroup;
    const uint32_t g = uint32_t(t % kTxGroup);
    if (k >= max_sel || k >= counts[0]) return;  // counts[0] <= max_sel: the emitted count; whole groups leave
    const uint32_t s = picked[k];
    const uint64_t off = uint64_t(s) * WTP_MAX_PAYLOAD, left = total_bytes - off;  // > 0: s < inflight
    const uint32_t len = left < WTP_MAX_PAYLOAD ? uint32_t(left) : WTP_MAX_PAYLOAD;
    const uint8_t *src = pay + off;
    uint8_t *slot = wire + k * stride, *dst = slot + WTP_HEADER_BYTES;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    // lane g: bytes [seg0, seg0 + seg) of the payload, copied and hashed (init and xorout ~0)
    const uint32_t seg0 = g * kTxSeg, seg = len > seg0 ? min(len - seg0, kTxSeg) : 0;
    uint32_t c = 0xFFFFFFFFu;
    if (vec && len == WTP_MAX_PAYLOAD) {
        const u32x4 *vs = reinterpret_cast<const u32x4 *>(src + seg0);
        u32x4 *vd = reinterpret_cast<u32x4 *>(dst + seg0);
        const uint32_t nv = seg / 16;  // 6, lane 15: 1
        u32x4 v[kTxVecs];
        v[0] = vs[0];
#pragma unroll
        for (uint32_t r = 1; r < kTxVecs; ++r)
            if (nv == kTxVecs) v[r] = vs[r];
        vd[0] = v[0];
#pragma unroll
        for (uint32_t r = 1; r < kTxVecs; ++r)
            if (nv == kTxVecs) vd[r] = v[r];
#pragma unroll
        for (uint32_t r = 0; r < kTxVecs; ++r)
            if (r == 0 || nv == kTxVecs) {
                c = crc_word(tab, c, v[r].x);
                c = crc_word(tab, c, v[r].y);
                c = crc_word(tab, c, v[r].z);
                c = crc_word(tab, c, v[r].w);
            }
    } else {
        // a short chunk, or any other alignment: bytes (exact; no access wider than the
        // buffers' alignment)
#pragma clang loop vectorize(disable) interleave(disable)
        for (uint32_t b = seg0; b < seg0 + seg; ++b) {
            const uint8_t x = src[b];
            dst[b] = x;
            c = tab[(c ^ x) & 0xFFu] ^ (c >> 8);
        }
    }
    // crc32(payload) = xor over the lanes of crc32(segment) * x^(8 * bytes after it)
    const uint32_t part = seg ? ~c : 0u;
    const uint32_t mult = len == WTP_MAX_PAYLOAD ? g_tx_tail.v[g] : gf::xpow8(len - (seg0 + seg));
    uint32_t crc = gf::mul(part, mult);
#pragma unroll
    for (int d = kTxGroup / 2; d > 0; d >>= 1) crc ^= __shfl_xor(crc, d, kTxGroup);
    const uint32_t hdr[4] = {WTP_TYPE_DATA, seq0 + s, len, crc};
    if (vec) {
        // the header: one 16-B store
        if (g == 0) *reinterpret_cast<u32x4 *>(slot) = header_be(hdr[0], hdr[1], hdr[2], hdr[3]);
    } else {
        const uint32_t word = g < 4 ? hdr[0] : g < 8 ? hdr[1] : g < 12 ? hdr[2] : hdr[3];
        slot[g] = uint8_t(word >> (8 * (3 - g % 4)));  // big-endian fields, one byte per lane
    }
    if (g == 0 && wire_len) wire_len[k] = WTP_HEADER_BYTES + len;
}

}  // namespace dev
}  // namespace wtp

namespace wtp {
// wtp_txvar.hip: k_tx_emit_var over the selection picked[m] (m > 0) that k_tx_select left
int tx_emit_var_launch(const void *d_base, size_t base_bytes, const uint64_t *d_offsets, const uint32_t *d_lengths,
                       uint32_t seq0, const uint32_t *picked, const uint32_t *d_counts, uint32_t m, void *d_wire,
                       size_t wire_stride, uint32_t *d_wire_len, uint32_t *d_crc_out, hipStream_t st);
}  // namespace wtp

namespace {

// d_work of wtp_tx_build_retransmit: picked[m], blk[blocks]; m = min(max_sel, inflight)
// entries (no more can be due).
struct TxWork {
    uint32_t m, blocks;
    uint32_t *picked, *blk;
    size_t bytes;
};

TxWork tx_layout(void *d_work, uint32_t inflight, uint32_t max_sel) {
    TxWork w;
    wtp::Work l(d_work, 4);
    w.m = std::min(inflight, max_sel);
    w.blocks = (inflight + wtp::dev::kTxBlock - 1) / wtp::dev::kTxBlock;
    w.picked = l.take<uint32_t>(w.m);
    w.blk = l.take<uint32_t>(w.blocks);
    w.bytes = l.bytes();
    return w;
}

// The ordered selection of both retransmit calls: w.picked and d_counts, after their checks.
int tx_select(const TxWork &w, uint32_t inflight, const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
              uint32_t timeout_ms, uint32_t flags, uint32_t *d_sel, uint32_t *d_counts, hipStream_t st) {
    using namespace wtp;
    int rc = WTP_OK;
    if (w.blocks > 0) {
        if ((rc = launch("k_tx_count", dev::k_tx_count, dim3(w.blocks), dim3(dev::kTxBlock), st, d_acked, d_sent_ms, inflight,
                         now_ms, timeout_ms, flags, w.blk)))
            return rc;
    }
    // inflight == 0: one block, which only writes d_counts = {0, 0}
    return launch("k_tx_select", dev::k_tx_select, dim3(std::max(w.blocks, 1u)), dim3(dev::kTxBlock), st, d_acked, d_sent_ms,
                  inflight, now_ms, timeout_ms, flags, w.blk, w.blocks, w.m, d_sel, w.picked, d_counts);
}

}  // namespace

extern "C" int wtp_tx_ingest_acks(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                                  uint32_t mode, uint32_t seq0, uint32_t inflight, uint32_t *d_acked, uint8_t *d_ok,
                                  uint32_t *d_hit, uint32_t *d_counts, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if (inflight > WTP_TX_MAX_INFLIGHT) return fail(WTP_EINVAL, "inflight %u > %u", inflight, WTP_TX_MAX_INFLIGHT);
    if ((rc = check_mode(mode))) return rc;
    if (!d_counts || (inflight > 0 && !d_acked)) return fail(WTP_EINVAL, "null pointer");
    if (n > 0 && (rc = check_ring(d_dgrams, stride, d_recv_len, d_ok))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(d_counts, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess) return fail(WTP_EHIP, "hipMemsetAsync(d_counts): %s", hipGetErrorString(e));
    if (n > 0 || mode == WTP_ACK_SELECTIVE) {  // n == 0: one block, which only sets d_counts[0]
        const uint64_t blocks = std::max<uint64_t>(1, (uint64_t(n) + 255) / 256);
        if ((rc = launch("k_tx_ingest", dev::k_tx_ingest, dim3(unsigned(blocks)), dim3(256), st,
                         static_cast<const uint8_t *>(d_dgrams), uint64_t(stride), d_recv_len, uint64_t(n), mode, seq0,
                         inflight, d_acked, d_ok, d_hit, d_counts)))
            return rc;
    }
    if (mode == WTP_ACK_SELECTIVE) {
        const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>(1, (uint64_t(inflight) + 255) / 256), 1024);
        return launch("k_tx_lead", dev::k_tx_lead, dim3(unsigned(blocks)), dim3(256), st, inflight, d_acked, d_counts);
    }
    return launch("k_tx_window", dev::k_tx_window, dim3(1), dim3(dev::kTxBlock), st, mode, inflight, d_acked, d_counts);
}

extern "C" size_t wtp_tx_work_bytes(uint32_t inflight, uint32_t max_sel) {
    return tx_layout(nullptr, std::min<uint32_t>(inflight, WTP_TX_MAX_INFLIGHT), max_sel).bytes;
}

extern "C" int wtp_tx_build_retransmit(const void *d_payloads, size_t total_bytes, uint32_t seq0, uint32_t inflight,
                                       const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
                                       uint32_t timeout_ms, uint32_t flags, void *d_wire, size_t wire_stride,
                                       uint32_t max_sel, uint32_t *d_sel, uint32_t *d_wire_len, uint32_t *d_counts,
                                       void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    if (wire_stride < WTP_HEADER_BYTES + WTP_MAX_PAYLOAD) return fail(WTP_EINVAL, "wire_stride %zu < 1472", wire_stride);
    if (inflight > WTP_TX_MAX_INFLIGHT) return fail(WTP_EINVAL, "inflight %u > %u", inflight, WTP_TX_MAX_INFLIGHT);
    if (inflight > 0 && uint64_t(inflight - 1) * WTP_MAX_PAYLOAD >= total_bytes)
        return fail(WTP_EINVAL, "total_bytes %zu does not reach slot %u", total_bytes, inflight - 1);
    const TxWork w = tx_layout(d_work, inflight, max_sel);
    int rc = check_work_bytes(work_bytes, w.bytes);
    if (rc) return rc;
    if (!d_counts || !d_work) return fail(WTP_EINVAL, "null pointer");
    if (inflight > 0 && (!d_payloads || !d_acked || !d_sent_ms)) return fail(WTP_EINVAL, "null pointer");
    if (w.m > 0 && !d_wire) return fail(WTP_EINVAL, "null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = tx_select(w, inflight, d_acked, d_sent_ms, now_ms, timeout_ms, flags, d_sel, d_counts, st)) || w.m == 0) return rc;
    const uint64_t blocks = (uint64_t(w.m) * dev::kTxGroup + 255) / 256;
    return launch("k_tx_emit", dev::k_tx_emit, dim3(unsigned(blocks)), dim3(256), st, static_cast<const uint8_t *>(d_payloads),
                  uint64_t(total_bytes), seq0, w.picked, d_counts, w.m, static_cast<uint8_t *>(d_wire), uint64_t(wire_stride),
                  d_wire_len);
}

extern "C" int wtp_tx_build_retransmit_var(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                                           const uint32_t *d_lengths, uint32_t seq0, uint32_t inflight,
                                           const uint32_t *d_acked, uint32_t *d_sent_ms, uint32_t now_ms,
                                           uint32_t timeout_ms, uint32_t flags, void *d_wire, size_t wire_stride,
                                           uint32_t max_sel, uint32_t *d_sel, uint32_t *d_wire_len, uint32_t *d_crc_out,
                                           uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    if (wire_stride < WTP_HEADER_BYTES + WTP_MAX_PAYLOAD) return fail(WTP_EINVAL, "wire_stride %zu < 1472", wire_stride);
    if (inflight > WTP_TX_MAX_INFLIGHT) return fail(WTP_EINVAL, "inflight %u > %u", inflight, WTP_TX_MAX_INFLIGHT);
    const TxWork w = tx_layout(d_work, inflight, max_sel);
    int rc = check_work_bytes(work_bytes, w.bytes);
    if (rc) return rc;
    if (!d_counts || !d_work) return null_arg("d_counts or d_work");
    if (inflight > 0 && (!d_base || !d_offsets || !d_lengths || !d_acked || !d_sent_ms))
        return null_arg("d_base, d_offsets, d_lengths, d_acked or d_sent_ms");
    if (w.m > 0 && !d_wire) return null_arg("d_wire");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = tx_select(w, inflight, d_acked, d_sent_ms, now_ms, timeout_ms, flags, d_sel, d_counts, st)) || w.m == 0) return rc;
    return tx_emit_var_launch(d_base, base_bytes, d_offsets, d_lengths, seq0, w.picked, d_counts, w.m, d_wire, wire_stride,
                              d_wire_len, d_crc_out, st);
}
