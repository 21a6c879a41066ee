// wtp_tx_flows.hip — the multi-connection sender (include/wtp_crc32.h: wtp_tx_ingest_acks_flows,
// wtp_tx_advance_flows, wtp_tx_build_retransmit_var_flows): the sender windows of many
// connections are fed their ACKs, slid and rebuilt in three calls, whatever the number of
// connections, with the window bases (seq0, rec0) in device memory, so one captured graph
// serves every round.  The mirror of wtp_flows.hip and wtp_flows_flush.hip.
//
// Per-connection semantics are those of wtp_tx.hip, wtp_advance.hip and wtp_txvar.hip; only
// the batching is new.  Flow f owns global slots [f*window, (f+1)*window) of one d_acked and
// one d_sent_ms; slot (f, s) is record rec0[f] + s of one record table, and the flow's window
// holds inflight_f = min(window, rec_end[f] - rec0[f]) slots (txf_inflight, the one place where
// all three calls take it from).
//
//   ingest   k_txf_init     one lane per flow: flow_fresh[f] = 0; flow_adv[f] = inflight_f ("no
//                           un-ACKed slot", selective) or kTxfRaw | 0 (cumulative: the largest
//                           a seen so far, marked as not yet a leading run)
//            k_txf_ingest   one lane per datagram: k_tx_ingest's verdict, then against the
//                           datagram's own flow: selective atomicCAS(&acked[g], 0, 1), whose old
//                           value makes flow_fresh[f] exact under duplicates; cumulative
//                           atomicMax(&flow_adv[f], kTxfRaw | a)
//            k_txf_fill     cumulative only, one lane per global slot: slots below the flow's
//                           largest a go 0 -> 1; a wave counts them per flow with one ballot and
//                           the lowest such lane of each flow adds the count to flow_fresh[f]
//            k_txf_lead     one lane per global slot, k_flows_place's scheme: a wave finds with
//                           one ballot the first un-ACKed slot of every flow it covers, and only
//                           those lanes lower flow_adv[f] (atomicMin: a slot index is below
//                           every kTxfRaw value)
//            k_txf_fin      cumulative only, one lane per flow: a flow_adv[f] that is still
//                           kTxfRaw | a had no un-ACKed slot and becomes inflight_f
//            The two per-flow arrays are the only accumulators.  flow_adv[f] holds two
//            quantities over a cumulative call (the largest a, then the leading run) and the
//            launch boundaries separate them: k_txf_fill only reads it, k_txf_lead only lowers
//            it.  Nothing is serial per flow: every pass is over datagrams, flows or the S
//            global slots, spread over the grid.
//   advance  k_txf_advance  one lane per global slot: k_tx_advance per flow with the flow's own
//                           advance; the lane of slot (f, 0) also moves seq0 and rec0
//   build    k_txf_count, k_txf_select   k_tx_count / k_tx_select over the S global slots with
//                           the wider predicate (s < inflight_f), so the selection is ordered by
//                           global slot: flow-major.  Same d_work layout as wtp_tx.hip's
//                           (picked[m], blk[blocks]), so wtp_tx_work_bytes(S, max_sel) sizes it.
//            k_txf_emit     k_tx_emit_var's body with another index map: datagram k of the ring
//                           is global slot picked[k] = (f, s), record rec0[f] + s (valid only
//                           below nrec), seqNum seq0[f] + s.
//
// Its own copies of the bodies, not templates shared with wtp_tx.hip and wtp_txvar.hip: the
// existing kernels keep their machine code.  The emit body as one
// function template for k_tx_emit_var and k_txf_emit changed both kernels' code and did not
// stay within the parent's spread on every row of tools/tx_flows_bench.py.
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_crc_dev.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kTxfRaw = 0x80000000u;  // flow_adv[f] = kTxfRaw | (largest a so far): not yet a run
constexpr uint32_t kTxfBlock = 1024;       // slots per block of the count / select passes
constexpr uint32_t kTxfWaves = kTxfBlock / 64;
static_assert(WTP_TX_MAX_FLOW_SLOTS <= kTxfBlock * kTxfBlock, "one block count per lane of k_txf_select");
static_assert(WTP_TX_MAX_FLOW_SLOTS < kTxfRaw, "a slot index is below every kTxfRaw value");

__device__ const SliceTable g_tf_table{};  // this unit's own object of the shared type (wtp_crc_dev.hpp)

// The slots of flow f's window that hold a record: the rule of all three calls.
__device__ __forceinline__ uint32_t txf_inflight(const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end,
                                                 uint32_t f, uint32_t window) {
    const uint32_t a = rec0[f], e = rec_end[f];
    return min(window, e > a ? e - a : 0u);  // a saturating subtraction: rec0 past rec_end is an empty window
}

// lanes first .. last of a wave
__device__ __forceinline__ uint64_t lane_span(uint32_t first, uint32_t last) {
    const uint64_t upto = last >= 63u ? ~uint64_t(0) : (uint64_t(1) << (last + 1)) - 1;
    return upto & ~((uint64_t(1) << first) - 1);
}

// ---- ACK ingest ----------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_txf_init(uint32_t mode, const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end, uint32_t nflows,
           uint32_t window, uint32_t *__restrict__ flow_adv, uint32_t *__restrict__ flow_fresh) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    flow_adv[f] = mode == WTP_ACK_SELECTIVE ? txf_inflight(rec0, rec_end, f, window) : kTxfRaw;
    flow_fresh[f] = 0;
}

__global__ void __launch_bounds__(256)
k_txf_ingest(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
             const uint32_t *__restrict__ flow, uint64_t n, uint32_t mode, const uint32_t *__restrict__ seq0,
             const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end, uint32_t nflows, uint32_t window,
             uint32_t *acked, uint8_t *__restrict__ ok, uint32_t *__restrict__ hit, uint32_t *flow_adv,
             uint32_t *flow_fresh) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t rl = recv_len[i];
    const uint32_t f = flow[i];
    const uint8_t *h = ring + i * stride;
    bool good = rl >= WTP_HEADER_BYTES && rl <= stride && rl - WTP_HEADER_BYTES <= WTP_MAX_KERNEL_LEN;
    Header hd{};
    if (good) {
        hd = load_header(h);  // type, seq, sum
        uint32_t c = 0;  // the CRC of the empty payload: a plain ACK is decided here
        if (rl > WTP_HEADER_BYTES) {
            c = 0xFFFFFFFFu;
            for (uint32_t b = WTP_HEADER_BYTES; b < rl; ++b) c = g_tf_table.t[0][(c ^ h[b]) & 0xFFu] ^ (c >> 8);
            c ^= 0xFFFFFFFFu;
        }
        good = hd.sum == c;
    }
    ok[i] = good ? 1 : 0;
    uint32_t where = WTP_NOT_PLACED;
    if (good && hd.type == WTP_TYPE_ACK && f < nflows) {  // f >= nflows: no connection
        const uint32_t inflight = txf_inflight(rec0, rec_end, f, window);
        const uint32_t d = hd.seq - seq0[f];  // unsigned: a wrapping window is well defined
        if (mode == WTP_ACK_SELECTIVE) {
            if (d < inflight) {
                where = d;
                if (atomicCAS(&acked[f * window + d], 0u, 1u) == 0u) atomicAdd(&flow_fresh[f], 1u);
            }
        } else if (d > 0 && d <= inflight) {
            where = d;
            if ((kTxfRaw | d) > __hip_atomic_load(&flow_adv[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&flow_adv[f], kTxfRaw | d);
        }
    }
    if (hit) hit[i] = where;
}

// Cumulative mode: flow_adv[f] = kTxfRaw | (the flow's largest a), only read here.
__global__ void __launch_bounds__(256)
k_txf_fill(const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end, uint32_t window, uint32_t slots,
           uint32_t *__restrict__ acked, const uint32_t *__restrict__ flow_adv, uint32_t *flow_fresh) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t f = 0, s = 0;
    bool fresh = false;
    if (g < slots) {
        f = g / window;
        s = g - f * window;
        const uint32_t top = min(flow_adv[f] & ~kTxfRaw, txf_inflight(rec0, rec_end, f, window));
        fresh = s < top && acked[g] == 0;
        if (fresh) acked[g] = 1;
    }
    // the flow's lanes in this wave are first .. last; the lowest of them that filled a slot
    // reports the count of all of them
    const uint64_t m = __ballot(fresh);
    if (fresh) {
        const uint64_t mine = m & lane_span(lane - min(s, lane), lane + min(63u - lane, window - 1 - s));
        if ((mine & ((uint64_t(1) << lane) - 1)) == 0) atomicAdd(&flow_fresh[f], uint32_t(__popcll(mine)));
    }
}

// flow_adv[f] becomes the flow's first un-ACKed slot, if it has one: a slot index is below
// inflight_f (selective) and below every kTxfRaw value (cumulative), so atomicMin serves both.
__global__ void __launch_bounds__(256)
k_txf_lead(const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end, uint32_t window, uint32_t slots,
           const uint32_t *__restrict__ acked, uint32_t *flow_adv) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t f = 0, s = 0;
    bool open = false;
    if (g < slots) {
        f = g / window;
        s = g - f * window;
        open = s < txf_inflight(rec0, rec_end, f, window) && acked[g] == 0;
    }
    const uint64_t m = __ballot(open);
    if (open) {
        const uint32_t first = lane - min(s, lane);  // the flow's first lane in this wave
        const uint64_t mine = (m >> first) << first;
        if ((mine & ((uint64_t(1) << lane) - 1)) == 0 &&
            s < __hip_atomic_load(&flow_adv[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(&flow_adv[f], s);
    }
}

// Cumulative mode: a flow with no un-ACKed slot still holds kTxfRaw | a.
__global__ void __launch_bounds__(256)
k_txf_fin(const uint32_t *__restrict__ rec0, const uint32_t *__restrict__ rec_end, uint32_t nflows, uint32_t window,
          uint32_t *__restrict__ flow_adv) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nflows) return;
    if (flow_adv[f] & kTxfRaw) flow_adv[f] = txf_inflight(rec0, rec_end, f, window);
}

// ---- slide ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
k_txf_advance(const uint32_t *__restrict__ acked, const uint32_t *__restrict__ sent_ms, uint32_t window, uint32_t slots,
              const uint32_t *__restrict__ flow_adv, uint32_t fill_ms, const uint32_t *__restrict__ seq0,
              const uint32_t *__restrict__ rec0, uint32_t *__restrict__ acked_next, uint32_t *__restrict__ sent_ms_next,
              uint32_t *__restrict__ seq0_next, uint32_t *__restrict__ rec0_next) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= slots) return;
    const uint32_t f = g / window, s = g - f * window;
    const uint32_t a = min(flow_adv[f], window);
    const uint32_t t = s + a;  // <= 2^21
    acked_next[g] = t < window ? acked[g + a] : 0u;
    sent_ms_next[g] = t < window ? sent_ms[g + a] : fill_ms;
    if (s == 0 && seq0_next) {
        seq0_next[f] = seq0[f] + a;
        rec0_next[f] = rec0[f] + a;
    }
}

// ---- retransmit selection --------------------------------------------------------------

__device__ __forceinline__ bool txf_due(const uint32_t *acked, const uint32_t *sent, const uint32_t *__restrict__ rec0,
                                        const uint32_t *__restrict__ rec_end, uint32_t g, uint32_t slots, uint32_t window,
                                        uint32_t now, uint32_t timeout, uint32_t flags) {
    if (g >= slots) return false;
    const uint32_t f = g / window, s = g - f * window;
    if (s >= txf_inflight(rec0, rec_end, f, window) || acked[g] != 0) return false;
    return (flags & WTP_RETX_ALL) || uint32_t(now - sent[g]) > timeout;
}

__global__ void __launch_bounds__(kTxfBlock)
k_txf_count(const uint32_t *__restrict__ acked, const uint32_t *__restrict__ sent, const uint32_t *__restrict__ rec0,
            const uint32_t *__restrict__ rec_end, uint32_t slots, uint32_t window, uint32_t now, uint32_t timeout,
            uint32_t flags, uint32_t *__restrict__ blk) {
    __shared__ uint32_t part[kTxfWaves];
    const uint32_t t = threadIdx.x, g = blockIdx.x * kTxfBlock + t;
    const bool due = txf_due(acked, sent, rec0, rec_end, g, slots, window, now, timeout, flags);
    const uint64_t b = __ballot(due);
    if ((t & 63u) == 0) part[t / 64] = uint32_t(__popcll(b));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kTxfWaves; ++w) sum += part[w];
        blk[blockIdx.x] = sum;
    }
}

// Block b ranks its due slots from sum(blk[0 .. b)); nblk <= kTxfBlock, one count per lane.
// picked[max_sel] is the selection in d_work (d_sel may be NULL), max_sel <= slots.
__global__ void __launch_bounds__(kTxfBlock)
k_txf_select(const uint32_t *__restrict__ acked, uint32_t *sent, const uint32_t *__restrict__ rec0,
             const uint32_t *__restrict__ rec_end, uint32_t slots, uint32_t window, uint32_t now, uint32_t timeout,
             uint32_t flags, const uint32_t *__restrict__ blk, uint32_t nblk, uint32_t max_sel, uint32_t *__restrict__ sel,
             uint32_t *__restrict__ picked, uint32_t *__restrict__ counts) {
    __shared__ uint32_t before[kTxfWaves], all[kTxfWaves], wave_due[kTxfWaves];
    const uint32_t t = threadIdx.x, g = blockIdx.x * kTxfBlock + t, w = t / 64, lane = t & 63u;
    const uint32_t c = t < nblk ? blk[t] : 0;
    const uint32_t sum_before = wave_sum(t < blockIdx.x ? c : 0), sum_all = wave_sum(c);
    const bool due = txf_due(acked, sent, rec0, rec_end, g, slots, window, now, timeout, flags);
    const uint64_t ballot = __ballot(due);
    if (lane == 0) {
        before[w] = sum_before;
        all[w] = sum_all;
        wave_due[w] = uint32_t(__popcll(ballot));
    }
    __syncthreads();
    uint32_t rank = 0, total = 0;
    for (uint32_t k = 0; k < kTxfWaves; ++k) {
        rank += before[k] + (k < w ? wave_due[k] : 0);
        total += all[k];
    }
    rank += uint32_t(__popcll(ballot & ((uint64_t(1) << lane) - 1)));
    if (due && rank < max_sel) {
        if (sel) sel[rank] = g;
        picked[rank] = g;
        sent[g] = now;
    }
    if (g == 0) {
        counts[0] = min(total, max_sel);
        counts[1] = total;
    }
}

// ---- retransmit emit ---------------------------------------------------------------------
// k_tx_emit_var's constants, tables and body (wtp_txvar.hip; the scheme is described at the
// top of wtp_buildvar.hip), this unit's own copy.

constexpr uint32_t kTfBlock = 256;                      // four waves, each with rounds of up to 64 datagrams
constexpr uint32_t kTfWaves = kTfBlock / 64;
constexpr uint32_t kTfVecs = 4;                         // 16-B vectors per piece
constexpr uint32_t kTfPiece = 16 * kTfVecs;             // a lane's contiguous bytes per turn
constexpr uint32_t kTfMaxPieces = (WTP_MAX_PAYLOAD + kTfPiece - 1) / kTfPiece;  // 23
constexpr uint32_t kTfMaxBlocks = 1280;                 // the capped grid: 5 workgroups per CU

// v[k] = x^(8 * kTfPiece * k), k < kTfMaxPieces; v[kTfMaxPieces + r] = x^(8 * r), r <= kTfPiece
constexpr uint32_t kTfPows = kTfMaxPieces + kTfPiece + 1;
struct TfPow {
    uint32_t v[kTfPows];
    constexpr TfPow() : v{} {
        const uint32_t x8 = gf::kOne >> 8;
        uint32_t *piece = v, *byte = v + kTfMaxPieces;
        byte[0] = gf::kOne;
        for (uint32_t r = 1; r <= kTfPiece; ++r) byte[r] = gf::mul(byte[r - 1], x8);
        piece[0] = gf::kOne;
        for (uint32_t k = 1; k < kTfMaxPieces; ++k) piece[k] = gf::mul(piece[k - 1], byte[kTfPiece]);
    }
};
__device__ const TfPow g_tf_pow{};
static_assert(TfPow{}.v[kTfMaxPieces + kTfPiece] == gf::xpow8(kTfPiece) &&
                  TfPow{}.v[kTfMaxPieces - 1] == gf::xpow8(kTfPiece * (kTfMaxPieces - 1)) && kTfPows <= kTfBlock,
              "powers");

// Datagram k < min(counts[0], max_sel) is global slot picked[k] = (f, s): record rec0[f] + s,
// seqNum seq0[f] + s, wire slot k.
__global__ void __launch_bounds__(kTfBlock, 5)  // five waves per SIMD: the capped grid is five workgroups per CU
k_txf_emit(const uint8_t *__restrict__ base, uint64_t base_bytes, const uint64_t *__restrict__ offs,
           const uint32_t *__restrict__ lens, uint64_t nrec, uint32_t max_sel, const uint32_t *__restrict__ seq0,
           const uint32_t *__restrict__ rec0, uint32_t window, const uint32_t *__restrict__ picked,
           const uint32_t *__restrict__ counts, uint8_t *__restrict__ wire, uint64_t stride, uint32_t vec,
           uint32_t *__restrict__ wire_len, uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t tab[4 * 256];
    __shared__ uint32_t pows[kTfPows];
    const uint32_t *ppiece = pows, *pbyte = pows + kTfMaxPieces;
    __shared__ uint32_t s_end[kTfWaves][64], s_lo[kTfWaves][64], s_hi[kTfWaves][64], s_len[kTfWaves][64];
    __shared__ uint32_t s_acc[kTfWaves][64], s_last[kTfWaves][64];
    __shared__ u32x4 s_move[kTfWaves][64 * kTfVecs];  // per wave: 64 pieces between their movers and their hasher
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t / 64;
    // the tables' loads are issued before the count's, so the two latencies overlap; a
    // workgroup that leaves has loaded 4 KiB it did not need
    uint32_t tv[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tv[k] = (&g_tf_table.t[0][0])[t + k * kTfBlock];
    const uint32_t pv = g_tf_pow.v[t < kTfPows ? t : 0];
    const uint32_t n = min(counts[0], max_sel);
    const uint32_t waves = gridDim.x * kTfWaves;
    uint32_t g = 0;  // log2 of the round size
    while (g < 6 && (uint64_t(waves) << g) < n) ++g;
    if ((uint64_t(blockIdx.x) * kTfWaves << g) >= n) return;  // the whole workgroup
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tab[t + k * kTfBlock] = tv[k];
    if (t < kTfPows) pows[t] = pv;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), hi = lo + base_bytes;
    __syncthreads();  // the tables are there; from here on the waves run on their own
    const uint32_t rounds = uint32_t((uint64_t(n) + (1u << g) - 1) >> g);
    const uint32_t step_r = gridDim.x * kTfWaves;
    for (uint32_t r = blockIdx.x * kTfWaves + wv; r < rounds; r += step_r) {
        const uint32_t i = (r << g) + lane;  // datagram i of the ring, n <= 2^20
        const bool has = (lane >> g) == 0 && i < n;  // lanes >= G carry no datagram
        uint32_t len = 0, seq = 0;
        uint64_t off = 0;
        bool valid = false;
        if (has) {
            const uint32_t gs = picked[i];  // the global slot: flow f, slot s
            const uint32_t f = gs / window, s = gs - f * window;
            const uint32_t rec = rec0[f] + s;  // mod 2^32
            seq = seq0[f] + s;
            if (rec < nrec) {  // no entry at or above nrec of either table is read
                off = offs[rec];
                len = lens[rec];
                valid = len <= WTP_MAX_PAYLOAD && off <= base_bytes && len <= base_bytes - off;
            }
        }
        const uint32_t np = valid ? (len + kTfPiece - 1) / kTfPiece : 0;
        uint32_t inc = np;  // inclusive prefix sum over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if (lane >= d) inc += y;
        }
        const uint32_t total = __shfl(inc, 63, 64);
        s_end[wv][lane] = inc;
        s_lo[wv][lane] = uint32_t(off);
        s_hi[wv][lane] = uint32_t(off >> 32);
        s_len[wv][lane] = len;
        s_acc[wv][lane] = 0;
        wave_sync();
        for (uint32_t task0 = 0; task0 < total; task0 += 64) {
            // this lane's piece: its owner is the first datagram whose pieces end after `task`
            const uint32_t task = task0 + lane;
            const bool mine = task < total;
            uint32_t o = 0, onp = 0, q = 0, nbytes = 0;
            uint64_t soff = 0, doff = 0;  // of the piece, from d_base and from d_wire
            if (mine) {
#pragma unroll
                for (uint32_t step = 32; step > 0; step >>= 1)
                    if (s_end[wv][o + step - 1] <= task) o += step;
                const uint32_t olen = s_len[wv][o];
                onp = (olen + kTfPiece - 1) / kTfPiece;
                q = task - (s_end[wv][o] - onp);                 // piece q of onp
                nbytes = min(kTfPiece, olen - kTfPiece * q);  // 1 .. 64, below 64 only in the last
                soff = ((uint64_t(s_hi[wv][o]) << 32) | s_lo[wv][o]) + kTfPiece * q;
                doff = uint64_t((r << g) + o) * stride + WTP_HEADER_BYTES + kTfPiece * q;
            }
            // the move: in turn u, lanes 4m .. 4m + 3 take the four vectors of the piece of lane
            // 16u + m, so a wave's loads and stores of consecutive pieces are contiguous
            const uint32_t m = lane & 3u;
            uint32_t nbv[kTfVecs], shv[kTfVecs];
            const uint8_t *sp[kTfVecs];
            uint8_t *dp[kTfVecs];
            bool fast[kTfVecs];
#pragma unroll
            for (uint32_t u = 0; u < kTfVecs; ++u) {
                const int from = int(16 * u + lane / 4);
                const uint32_t pn = __shfl(nbytes, from, 64);
                const uint64_t ps = (uint64_t(__shfl(uint32_t(soff >> 32), from, 64)) << 32) | __shfl(uint32_t(soff), from, 64);
                const uint64_t pd = (uint64_t(__shfl(uint32_t(doff >> 32), from, 64)) << 32) | __shfl(uint32_t(doff), from, 64);
                nbv[u] = pn > 16 * m ? min(16u, pn - 16 * m) : 0;
                sp[u] = base + ps + 16 * m;
                dp[u] = wire + pd + 16 * m;
                shv[u] = uint32_t(reinterpret_cast<uintptr_t>(sp[u])) & 3u;
                const uintptr_t pa = reinterpret_cast<uintptr_t>(sp[u]) - shv[u];
                fast[u] = nbv[u] && pa >= lo && pa + (shv[u] ? 20u : 16u) <= hi;
            }
            u32x4 d[kTfVecs] = {};
            uint32_t e[kTfVecs] = {};
#pragma unroll
            for (uint32_t u = 0; u < kTfVecs; ++u)
                if (fast[u]) {
                    const uint8_t *p = sp[u] - shv[u];  // the dword that holds the first byte
                    d[u] = *reinterpret_cast<const u32x4_a4 *>(p);
                    e[u] = *reinterpret_cast<const uint32_t *>(p + (shv[u] ? 16 : 12));  // sh == 0: d.w again, unused
                }
#pragma unroll
            for (uint32_t u = 0; u < kTfVecs; ++u) {
                u32x4 v;
                v.x = __builtin_amdgcn_alignbyte(d[u].y, d[u].x, shv[u]);
                v.y = __builtin_amdgcn_alignbyte(d[u].z, d[u].y, shv[u]);
                v.z = __builtin_amdgcn_alignbyte(d[u].w, d[u].z, shv[u]);
                v.w = __builtin_amdgcn_alignbyte(e[u], d[u].w, shv[u]);
                // within 20 bytes of an edge of the buffer: the payload's own bytes, one by one
                if (nbv[u] && !fast[u]) v = load_bytes(sp[u], nbv[u]);
                if (nbv[u]) store_vec(dp[u], v, nbv[u], vec);
                // piece P = 16u + lane / 4 of the wave, vector m, in slot (m + P / 4) % 4 of its 64 bytes
                s_move[wv][4 * (16 * u + lane / 4) + ((m + lane / 16) & 3u)] = v;
            }
            wave_sync();
            // the hash: a lane's own piece, its vectors in order; init ~0 enters with the
            // payload's first piece, xorout ~0 at the owner
            uint32_t c = q == 0 ? 0xFFFFFFFFu : 0u;
            const uint32_t nfull = nbytes / 16;
            u32x4 part = {};  // the payload's last vector, if it is not whole
#pragma unroll
            for (uint32_t k = 0; k < kTfVecs; ++k) {
                const u32x4 v = s_move[wv][4 * lane + ((k + lane / 4) & 3u)];
                if (k < nfull) {
                    c = crc_word(tab, c, v.x);
                    c = crc_word(tab, c, v.y);
                    c = crc_word(tab, c, v.z);
                    c = crc_word(tab, c, v.w);
                }
                if (k == nfull) part = v;
            }
            if (nbytes & 15u) c = crc_vec(tab, c, part, nbytes & 15u);
            if (mine) {
                if (q + 1 == onp)
                    s_last[wv][o] = c;
                else
                    atomicXor(&s_acc[wv][o], gf::mul(c, ppiece[onp - 2 - q]));
            }
            wave_sync();  // the next turn's s_move stores follow these loads
        }
        if (has) {
            uint32_t crc = 0;
            if (valid) {
                if (len) crc = gf::mul(s_acc[wv][lane], pbyte[len - kTfPiece * (np - 1)]) ^ s_last[wv][lane] ^ 0xFFFFFFFFu;
                uint8_t *slot = wire + uint64_t(i) * stride;
                const u32x4 h = header_be(WTP_TYPE_DATA, seq, len, crc);
                if (vec)
                    *reinterpret_cast<u32x4 *>(slot) = h;
                else
                    store_bytes(slot, h, 0, 16);
            }
            if (wire_len) wire_len[i] = valid ? WTP_HEADER_BYTES + len : 0;
            if (crc_out) crc_out[i] = crc;
        }
    }
}

}  // namespace dev
}  // namespace wtp

namespace {

unsigned blocks_of(uint64_t lanes, unsigned block = 256) { return unsigned((lanes + block - 1) / block); }

}  // namespace

extern "C" int wtp_tx_ingest_acks_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                                        const uint32_t *d_flow, size_t n, uint32_t mode, const uint32_t *d_seq0,
                                        const uint32_t *d_rec0, const uint32_t *d_rec_end, uint32_t nflows,
                                        uint32_t window, uint32_t *d_acked, uint8_t *d_ok, uint32_t *d_hit,
                                        uint32_t *d_flow_adv, uint32_t *d_flow_fresh, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if ((rc = check_mode(mode))) return rc;
    if ((rc = check_stride(stride))) return rc;
    if ((rc = check_tx_flows(nflows, window))) return rc;
    const uint32_t slots = nflows * window;
    if (nflows > 0) {
        if (!d_flow_adv) return null_arg("d_flow_adv");
        if (!d_flow_fresh) return null_arg("d_flow_fresh");
        if (!d_seq0) return null_arg("d_seq0");
        if (!d_rec0) return null_arg("d_rec0");
        if (!d_rec_end) return null_arg("d_rec_end");
    }
    if (slots > 0 && !d_acked) return null_arg("d_acked");
    if (n > 0) {
        if (!d_dgrams) return null_arg("d_dgrams");
        if (!d_recv_len) return null_arg("d_recv_len");
        if (!d_flow) return null_arg("d_flow");
        if (!d_ok) return null_arg("d_ok");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool cum = mode == WTP_ACK_CUMULATIVE;
    if (nflows > 0 && (rc = launch("k_txf_init", dev::k_txf_init, dim3(blocks_of(nflows)), dim3(256), st, mode, d_rec0, d_rec_end,
                                   nflows, window, d_flow_adv, d_flow_fresh)))
        return rc;
    if (n > 0 && (rc = launch("k_txf_ingest", dev::k_txf_ingest, dim3(blocks_of(n)), dim3(256), st,
                              static_cast<const uint8_t *>(d_dgrams), uint64_t(stride), d_recv_len, d_flow, uint64_t(n), mode,
                              d_seq0, d_rec0, d_rec_end, nflows, window, d_acked, d_ok, d_hit, d_flow_adv, d_flow_fresh)))
        return rc;
    if (slots > 0) {
        if (cum && (rc = launch("k_txf_fill", dev::k_txf_fill, dim3(blocks_of(slots)), dim3(256), st, d_rec0, d_rec_end, window,
                                slots, d_acked, d_flow_adv, d_flow_fresh)))
            return rc;
        if ((rc = launch("k_txf_lead", dev::k_txf_lead, dim3(blocks_of(slots)), dim3(256), st, d_rec0, d_rec_end, window, slots,
                         d_acked, d_flow_adv)))
            return rc;
    }
    if (cum && nflows > 0)
        return launch("k_txf_fin", dev::k_txf_fin, dim3(blocks_of(nflows)), dim3(256), st, d_rec0, d_rec_end, nflows, window,
                      d_flow_adv);
    return WTP_OK;
}

extern "C" int wtp_tx_advance_flows(const uint32_t *d_acked, const uint32_t *d_sent_ms, uint32_t nflows, uint32_t window,
                                    const uint32_t *d_flow_adv, uint32_t fill_ms, const uint32_t *d_seq0,
                                    const uint32_t *d_rec0, uint32_t *d_acked_next, uint32_t *d_sent_ms_next,
                                    uint32_t *d_seq0_next, uint32_t *d_rec0_next, void *stream) {
    using namespace wtp;
    int rc = check_tx_flows(nflows, window);
    if (rc) return rc;
    if (!d_seq0 != !d_seq0_next)
        return fail(WTP_EINVAL, "null pointer: %s without %s", d_seq0 ? "d_seq0" : "d_seq0_next", d_seq0 ? "d_seq0_next" : "d_seq0");
    if (!d_rec0 != !d_rec0_next)
        return fail(WTP_EINVAL, "null pointer: %s without %s", d_rec0 ? "d_rec0" : "d_rec0_next", d_rec0 ? "d_rec0_next" : "d_rec0");
    if (!d_seq0 != !d_rec0) return fail(WTP_EINVAL, "null pointer: %s without %s", d_seq0 ? "d_seq0" : "d_rec0", d_seq0 ? "d_rec0" : "d_seq0");
    const uint32_t slots = nflows * window;
    if (slots == 0) return WTP_OK;
    if (!d_flow_adv) return fail(WTP_EINVAL, "null pointer: d_flow_adv with %u slots", slots);
    if (!d_acked) return fail(WTP_EINVAL, "null pointer: d_acked with %u slots", slots);
    if (!d_sent_ms) return fail(WTP_EINVAL, "null pointer: d_sent_ms with %u slots", slots);
    if (!d_acked_next) return fail(WTP_EINVAL, "null pointer: d_acked_next with %u slots", slots);
    if (!d_sent_ms_next) return fail(WTP_EINVAL, "null pointer: d_sent_ms_next with %u slots", slots);
    // an output over an input: another workgroup may still read what this one writes
    {
        const void *in[2] = {d_acked, d_sent_ms}, *out[2] = {d_acked_next, d_sent_ms_next};
        const char *in_name[2] = {"d_acked", "d_sent_ms"}, *out_name[2] = {"d_acked_next", "d_sent_ms_next"};
        for (int o = 0; o < 2; ++o)
            for (int i = 0; i < 2; ++i)
                if (overlap(in[i], out[o], uint64_t(slots) * 4))
                    return fail(WTP_EINVAL, "%s overlaps %s (%u slots)", out_name[o], in_name[i], slots);
        if (overlap(d_acked_next, d_sent_ms_next, uint64_t(slots) * 4))
            return fail(WTP_EINVAL, "d_sent_ms_next overlaps d_acked_next (%u slots)", slots);
    }
    if (d_seq0) {
        const void *in[3] = {d_seq0, d_rec0, d_flow_adv}, *out[2] = {d_seq0_next, d_rec0_next};
        const char *in_name[3] = {"d_seq0", "d_rec0", "d_flow_adv"}, *out_name[2] = {"d_seq0_next", "d_rec0_next"};
        for (int o = 0; o < 2; ++o)
            for (int i = 0; i < 3; ++i)
                if (overlap(in[i], out[o], uint64_t(nflows) * 4))
                    return fail(WTP_EINVAL, "%s overlaps %s (nflows %u)", out_name[o], in_name[i], nflows);
        if (overlap(d_seq0_next, d_rec0_next, uint64_t(nflows) * 4))
            return fail(WTP_EINVAL, "d_rec0_next overlaps d_seq0_next (nflows %u)", nflows);
    }
    return launch("k_txf_advance", dev::k_txf_advance, dim3(blocks_of(slots)), dim3(256), static_cast<hipStream_t>(stream),
                  d_acked, d_sent_ms, window, slots, d_flow_adv, fill_ms, d_seq0, d_rec0, d_acked_next, d_sent_ms_next,
                  d_seq0_next, d_rec0_next);
}

extern "C" int wtp_tx_build_retransmit_var_flows(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                                                 const uint32_t *d_lengths, size_t nrec, const uint32_t *d_seq0,
                                                 const uint32_t *d_rec0, const uint32_t *d_rec_end, uint32_t nflows,
                                                 uint32_t window, const uint32_t *d_acked, uint32_t *d_sent_ms,
                                                 uint32_t now_ms, uint32_t timeout_ms, uint32_t flags, void *d_wire,
                                                 size_t wire_stride, uint32_t max_sel, uint32_t *d_sel,
                                                 uint32_t *d_wire_len, uint32_t *d_crc_out, uint32_t *d_counts,
                                                 void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    if (wire_stride < WTP_HEADER_BYTES + WTP_MAX_PAYLOAD) return fail(WTP_EINVAL, "wire_stride %zu < 1472", wire_stride);
    int rc = check_tx_flows(nflows, window);
    if (rc) return rc;
    const uint32_t slots = nflows * window;
    // wtp_tx.hip's layout over the global slots: picked[m], blk[blocks]
    Work l(d_work, 4);
    const uint32_t m = std::min(slots, max_sel), nblk = (slots + dev::kTxfBlock - 1) / dev::kTxfBlock;
    uint32_t *picked = l.take<uint32_t>(m), *blk = l.take<uint32_t>(nblk);
    if ((rc = check_work_bytes(work_bytes, wtp_tx_work_bytes(slots, max_sel)))) return rc;
    if (!d_counts || !d_work) return null_arg("d_counts or d_work");
    if (slots > 0) {
        if (!d_base || !d_offsets || !d_lengths) return null_arg("d_base, d_offsets or d_lengths");
        if (!d_acked || !d_sent_ms) return null_arg("d_acked or d_sent_ms");
        if (!d_seq0 || !d_rec0 || !d_rec_end) return null_arg("d_seq0, d_rec0 or d_rec_end");
    }
    if (m > 0 && !d_wire) return null_arg("d_wire");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nblk > 0 && (rc = launch("k_txf_count", dev::k_txf_count, dim3(nblk), dim3(dev::kTxfBlock), st, d_acked, d_sent_ms, d_rec0,
                                 d_rec_end, slots, window, now_ms, timeout_ms, flags, blk)))
        return rc;
    // no slots: one block, which only writes d_counts = {0, 0}
    rc = launch("k_txf_select", dev::k_txf_select, dim3(std::max(nblk, 1u)), dim3(dev::kTxfBlock), st, d_acked, d_sent_ms, d_rec0,
                d_rec_end, slots, window, now_ms, timeout_ms, flags, blk, nblk, m, d_sel, picked, d_counts);
    if (rc || m == 0) return rc;
    const uint32_t vec = (reinterpret_cast<uintptr_t>(d_wire) & 15u) == 0 && wire_stride % 16 == 0;
    const unsigned blocks = std::min((m + dev::kTfWaves - 1) / dev::kTfWaves, dev::kTfMaxBlocks);
    return launch("k_txf_emit", dev::k_txf_emit, dim3(blocks), dim3(dev::kTfBlock), st, static_cast<const uint8_t *>(d_base),
                  uint64_t(base_bytes), d_offsets, d_lengths, uint64_t(nrec), m, d_seq0, d_rec0, window, picked, d_counts,
                  static_cast<uint8_t *>(d_wire), uint64_t(wire_stride), vec, d_wire_len, d_crc_out);
}
