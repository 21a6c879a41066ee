// wtp_ack.hip — device-side ACK generation (include/wtp_crc32.h: wtp_rx_build_acks), the
// receiver's reply ring: the call that follows wtp_accept_data_packets on the same batch
// and precedes the sender's wtp_tx_ingest_acks.
//
// Semantics: one ACK per accepted DATA datagram, in arrival order.  Selective repeat
// (cpp/src/opt/Receiver.cpp:211-237) answers with the datagram's own seqNum; go-back-N
// (cpp/src/base/Receiver.cpp:206-237, and wReceiver.cpp's `ack_seq = expected`) answers
// with the next expected seqNum at that moment, i.e. seq0 + the leading run of filled slots
// after datagrams 0 .. i.  That running value is a prefix problem over the window: give
// every slot a fill time (0: filled before the batch, j + 1: filled by datagram j, never
// otherwise), take the inclusive prefix maximum T over the slots, and slot s belongs to
// the leading run after datagram i iff T[s] <= i + 1.  T is monotone, so the run's length
// is an upper bound found by binary search.
//
// Stream-ordered launches, scratch in the caller's d_work (blk[ceil(n / 1024)], and in
// cumulative mode T[window], bmax[ceil(window / 1024)]):
//   k_ack_init   cumulative: T[s] = kPre (filled before) or kNever (empty) from d_slot_len
//   k_ack_mark   one lane per datagram: the eligibility predicate, wave64 ballot + popcount
//                -> a count per 1024-datagram block; cumulative: atomicMin(&T[place[i]],
//                i + 1), so the lowest index wins for any d_place (kPre and kNever lie above
//                every index, and a slot that d_place names takes its fill time from there)
//   k_ack_bmax   cumulative: the maximum fill time of each 1024-slot block
//   k_ack_scan   cumulative: every block reduces the block maxima before it (<= 1024, one
//                per lane) and scans its own 1024 slots; T in place
//   k_ack_emit   one lane per datagram: the block sums the counts before it (<= 16 Ki, 16
//                per lane), recomputes the predicate, ranks its eligible lanes (an ordered
//                compaction, as k_tx_select), finds the running ACK in T and stores the
//                header of rank r in [skip, skip + max_acks) as entry r - skip; d_counts.
// Every word of d_work that a kernel reads was written by an earlier launch of the same
// call; the call keeps no state and reads no library table.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kAckBlock = 1024;  // datagrams (mark, emit) or slots (bmax, scan) per block
constexpr uint32_t kAckWaves = kAckBlock / 64;
constexpr uint32_t kAckCounts = WTP_RX_MAX_BATCH / kAckBlock / kAckBlock;  // block counts per lane of k_ack_emit
static_assert(kAckCounts * kAckBlock * kAckBlock == WTP_RX_MAX_BATCH, "16 counts per lane cover the largest batch");
static_assert(WTP_RX_MAX_WINDOW <= kAckBlock * kAckBlock, "one block maximum per lane of k_ack_scan");
constexpr uint32_t kNever = 0xFFFFFFFFu;  // raw T: an empty slot that no datagram fills
constexpr uint32_t kPre = 0xFFFFFFFEu;    // raw T: filled before the batch (fill time 0) unless d_place names it

// Fill time of a slot from its raw word: 0 = before the batch, j + 1 = by datagram j.
__device__ __forceinline__ uint32_t ack_fill_time(uint32_t raw) { return raw == kPre ? 0u : raw; }

// Is datagram i answered?  The header is read only where ok says it is there.
__device__ __forceinline__ bool ack_eligible(const uint8_t *__restrict__ ring, uint64_t stride,
                                             const uint32_t *__restrict__ recv_len, const uint8_t *__restrict__ ok,
                                             uint32_t i, uint32_t n, uint32_t seq0, uint32_t window, uint32_t &seq) {
    if (i >= n || ok[i] == 0) return false;
    const uint32_t len = recv_len[i] - WTP_HEADER_BYTES;  // unsigned: a length below 16 is never <= 1456
    const Header hd = load_header(ring + uint64_t(i) * stride);  // type, seq
    seq = hd.seq;
    const uint32_t d = seq - seq0;  // unsigned: a wrapping window is well defined
    return hd.type == WTP_TYPE_DATA && len <= WTP_MAX_PAYLOAD && (d < window || d >= 0x80000000u);
}

__global__ void __launch_bounds__(256)
k_ack_init(const uint32_t *__restrict__ slot_len, uint32_t window, uint32_t *__restrict__ T) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < window) T[s] = slot_len[s] == WTP_SLOT_EMPTY ? kNever : kPre;
}

__global__ void __launch_bounds__(kAckBlock)
k_ack_mark(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
           const uint8_t *__restrict__ ok, uint32_t n, uint32_t seq0, uint32_t window,
           const uint32_t *__restrict__ place, uint32_t *T, uint32_t *__restrict__ blk) {
    __shared__ uint32_t part[kAckWaves];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kAckBlock + t;
    uint32_t seq = 0;
    const bool ans = ack_eligible(ring, stride, recv_len, ok, i, n, seq0, window, seq);
    if (T && i < n) {  // cumulative mode with a window: T[window]
        const uint32_t s = place[i];
        if (s < window) atomicMin(&T[s], i + 1);  // an entry >= window counts as WTP_NOT_PLACED
    }
    const uint64_t b = __ballot(ans);
    if ((t & 63u) == 0) part[t / 64] = uint32_t(__popcll(b));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kAckWaves; ++w) sum += part[w];
        blk[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(kAckBlock)
k_ack_bmax(const uint32_t *__restrict__ T, uint32_t window, uint32_t *__restrict__ bmax) {
    __shared__ uint32_t part[kAckWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kAckBlock + t;
    const uint32_t m = wave_max(s < window ? ack_fill_time(T[s]) : 0u);
    if ((t & 63u) == 0) part[t / 64] = m;
    __syncthreads();
    if (t == 0) {
        uint32_t top = 0;
        for (uint32_t w = 0; w < kAckWaves; ++w) top = max(top, part[w]);
        bmax[blockIdx.x] = top;
    }
}

// T[s] <- max(fill time of slots 0 .. s), in place: a block reads and writes only its own
// 1024 slots of T, and what lies before them comes from bmax.
__global__ void __launch_bounds__(kAckBlock)
k_ack_scan(uint32_t *T, uint32_t window, const uint32_t *__restrict__ bmax) {
    __shared__ uint32_t before[kAckWaves], wave_top[kAckWaves];
    const uint32_t t = threadIdx.x, s = blockIdx.x * kAckBlock + t, w = t / 64, lane = t & 63u;
    const uint32_t prev = wave_max(t < blockIdx.x ? bmax[t] : 0u);  // gridDim.x <= 1024
    uint32_t v = s < window ? ack_fill_time(T[s]) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= uint32_t(d)) v = max(v, up);
    }
    if (lane == 0) before[w] = prev;
    if (lane == 63) wave_top[w] = v;
    __syncthreads();
    uint32_t pre = 0;
    for (uint32_t k = 0; k < kAckWaves; ++k) pre = max(pre, max(before[k], k < w ? wave_top[k] : 0u));
    if (s < window) T[s] = max(v, pre);
}

__global__ void __launch_bounds__(kAckBlock)
k_ack_emit(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
           const uint8_t *__restrict__ ok, uint32_t n, uint32_t mode, uint32_t seq0, uint32_t window,
           const uint32_t *__restrict__ T, const uint32_t *__restrict__ blk, uint32_t nblk, uint8_t *__restrict__ wire,
           uint64_t ack_stride, uint32_t skip, uint32_t max_acks, uint32_t *__restrict__ src,
           uint32_t *__restrict__ counts) {
    __shared__ uint32_t before[kAckWaves], all[kAckWaves], wave_ans[kAckWaves];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kAckBlock + t, w = t / 64, lane = t & 63u;
    uint32_t c_before = 0, c_all = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < kAckCounts; ++k) {
        const uint32_t b = k * kAckBlock + t;
        const uint32_t c = b < nblk ? blk[b] : 0u;
        c_all += c;
        c_before += b < blockIdx.x ? c : 0u;
    }
    c_before = wave_sum(c_before);
    c_all = wave_sum(c_all);
    uint32_t seq = 0;
    const bool ans = ack_eligible(ring, stride, recv_len, ok, i, n, seq0, window, seq);
    const uint64_t ballot = __ballot(ans);
    if (lane == 0) {
        before[w] = c_before;
        all[w] = c_all;
        wave_ans[w] = uint32_t(__popcll(ballot));
    }
    __syncthreads();
    uint32_t rank = 0, total = 0;
    for (uint32_t k = 0; k < kAckWaves; ++k) {
        rank += before[k] + (k < w ? wave_ans[k] : 0u);
        total += all[k];
    }
    rank += __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u));
    if (i == 0) {  // n == 0: the one block's thread 0
        counts[0] = total > skip ? min(total - skip, max_acks) : 0u;
        counts[1] = total;
    }
    if (!ans || rank < skip || rank - skip >= max_acks) return;
    const uint32_t k = rank - skip;
    if (mode == WTP_ACK_CUMULATIVE) {
        // the leading run after datagrams 0 .. i: the slots with T[s] <= i + 1, an upper bound
        // in the monotone T (window <= 2^20: at most 20 dependent loads)
        uint32_t lo = 0, hi = T ? window : 0u;  // no T: window == 0
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (T[mid] <= i + 1)
                lo = mid + 1;
            else
                hi = mid;
        }
        seq = seq0 + lo;
    }
    store_ack(wire + uint64_t(k) * ack_stride, seq);
    if (src) src[k] = i;
}

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_rx_build_acks: blk[nblk], then in cumulative mode T[window] and bmax[wblk].
struct AckWork {
    uint32_t nblk, wblk;
    uint32_t *blk, *T, *bmax;
    size_t bytes;
};

AckWork ack_layout(void *d_work, size_t n, uint32_t window, uint32_t mode) {
    AckWork w;
    wtp::Work l(d_work, 4);
    const uint32_t slots = mode == WTP_ACK_SELECTIVE ? 0u : window;
    w.nblk = uint32_t((n + wtp::dev::kAckBlock - 1) / wtp::dev::kAckBlock);
    w.wblk = (slots + wtp::dev::kAckBlock - 1) / wtp::dev::kAckBlock;
    w.blk = l.take<uint32_t>(w.nblk);
    w.T = l.take<uint32_t>(slots);
    w.bmax = l.take<uint32_t>(w.wblk);
    w.bytes = l.bytes();
    return w;
}

}  // namespace

extern "C" size_t wtp_rx_ack_work_bytes(size_t n, uint32_t window, uint32_t mode) {
    return ack_layout(nullptr, std::min<size_t>(n, WTP_RX_MAX_BATCH), std::min<uint32_t>(window, WTP_RX_MAX_WINDOW), mode).bytes;
}

extern "C" int wtp_rx_build_acks(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, size_t n,
                                 uint32_t mode, uint32_t seq0, uint32_t window, const uint8_t *d_ok,
                                 const uint32_t *d_place, const uint32_t *d_slot_len, void *d_ack_wire,
                                 size_t ack_stride, uint32_t skip, uint32_t max_acks, uint32_t *d_src,
                                 uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    if (n > WTP_RX_MAX_BATCH) return fail(WTP_EINVAL, "n %zu > %u", n, WTP_RX_MAX_BATCH);
    int rc = check_mode(mode);
    if (rc) return rc;
    const bool cum = mode == WTP_ACK_CUMULATIVE;
    if (cum && window > WTP_RX_MAX_WINDOW) return fail(WTP_EINVAL, "window %u > %u", window, WTP_RX_MAX_WINDOW);
    if ((rc = check_stride(stride))) return rc;
    if (ack_stride < 16) return fail(WTP_EINVAL, "ack_stride %zu < 16", ack_stride);
    const AckWork w = ack_layout(d_work, n, window, mode);
    if ((rc = check_work_bytes(work_bytes, w.bytes))) return rc;
    if (!d_counts || !d_work) return fail(WTP_EINVAL, "null pointer");
    if (n > 0) {
        if ((rc = check_ring(d_dgrams, stride, d_recv_len, d_ok))) return rc;
        if (cum && window > 0 && (!d_place || !d_slot_len)) return fail(WTP_EINVAL, "null pointer");
        if (max_acks > 0 && !d_ack_wire) return fail(WTP_EINVAL, "null pointer");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *ring = static_cast<const uint8_t *>(d_dgrams);
    // T: cumulative mode with datagrams and a window; otherwise no slot is ever looked up
    uint32_t *T = cum && n > 0 && window > 0 ? w.T : nullptr;
    const uint32_t n32 = uint32_t(n);
    if (T) {
        if ((rc = launch("k_ack_init", dev::k_ack_init, dim3((window + 255) / 256), dim3(256), st, d_slot_len, window, T))) return rc;
    }
    if (n > 0) {
        rc = launch("k_ack_mark", dev::k_ack_mark, dim3(w.nblk), dim3(dev::kAckBlock), st, ring, uint64_t(stride), d_recv_len,
                    d_ok, n32, seq0, window, d_place, T, w.blk);
        if (rc) return rc;
    }
    if (T) {
        if ((rc = launch("k_ack_bmax", dev::k_ack_bmax, dim3(w.wblk), dim3(dev::kAckBlock), st, T, window, w.bmax))) return rc;
        if ((rc = launch("k_ack_scan", dev::k_ack_scan, dim3(w.wblk), dim3(dev::kAckBlock), st, T, window, w.bmax))) return rc;
    }
    // n == 0: one block, which only writes d_counts = {0, 0}.  The kernel picks the 16-B
    // store per slot from the slot's own address: with an aligned ring and ack_stride % 16
    // == 0 that is every slot, otherwise only a slot that happens to be aligned.
    return launch("k_ack_emit", dev::k_ack_emit, dim3(std::max(w.nblk, 1u)), dim3(dev::kAckBlock), st, ring, uint64_t(stride),
                  d_recv_len, d_ok, n32, mode, seq0, window, T, w.blk, w.nblk, static_cast<uint8_t *>(d_ack_wire),
                  uint64_t(ack_stride), skip, max_acks, d_src, d_counts);
}
