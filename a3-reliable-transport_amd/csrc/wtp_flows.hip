// wtp_flows.hip — multi-connection receive (include/wtp_crc32.h: wtp_accept_data_packets_flows,
// wtp_rx_build_acks_flows): the arrivals of many connections, interleaved in arrival order,
// are verified, placed into their own flow's window and answered in one stream-ordered pass.
//
// Per-connection semantics are those of wtp_accept.hip and wtp_ack.hip (the reference serves
// one connection at a time, cpp/src/opt/Receiver.cpp:145-150); only the batching is new.
// Flow f owns slots [f*window, (f+1)*window) of one slot_len array and one image, so the
// global slot of (f, s) is f*window + s and the per-flow flush and slide keep using
// wtp_rx_deliver / wtp_rx_advance on the sub-window.
//
//   accept   1. verify         wtp_crc32_verify_batch -> ok[]
//            2. k_flows_claim  one lane per datagram: an intact in-window DATA datagram of a
//                              known flow claims its global slot with atomicMin(&slot_len[g],
//                              0x80000000 | i).  A global slot belongs to one flow, so the
//                              same seqNum in two flows never meets, and within a flow the
//                              order EMPTY > claim > stored length makes the lowest index win
//                              exactly as in k_accept_claim.  Lanes [0, nflows) also set
//                              ack[f] = seq0[f] + window ("no EMPTY slot").
//            3. k_flows_place  16 lanes per datagram copy the owner's payload and publish
//                              slot_len and place; every lane also scans its share of all
//                              nflows*window slots for the per-flow ACK: consecutive lanes take
//                              consecutive global slots, a wave finds with one ballot the
//                              first EMPTY slot of every flow it covers, and only those lanes
//                              lower ack[f].  Many small windows and one large window are
//                              both just slots spread over the grid; no launch or serial walk
//                              per flow.
//   acks     k_flows_ack_mark  one lane per datagram: the eligibility predicate with the
//                              flow's base, a count per 1024-datagram block
//            k_flows_ack_emit  ranks the eligible lanes in arrival order (the ordered
//                              compaction of k_ack_emit) and stores the ACKs; the cumulative
//                              seqNum is the flow's ACK after the whole batch, flow_ack[f].
//
// From wtp_common.hpp, with wtp_accept.hip and wtp_ack.hip: the claim constant, ack_lower, the
// 16-lane slot copy (copy_slot16) and the ACK datagram's store (store_ack).  The ordered
// compaction keeps its own body here as there.
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kFlowBlock = 1024;         // datagrams per block of the ACK kernels
constexpr uint32_t kFlowWaves = kFlowBlock / 64;
constexpr uint32_t kFlowCounts = WTP_RX_MAX_BATCH / kFlowBlock / kFlowBlock;  // block counts per lane of k_flows_ack_emit
static_assert(kFlowCounts * kFlowBlock * kFlowBlock == WTP_RX_MAX_BATCH, "16 counts per lane cover the largest batch");

// Global slot of datagram i if it may be placed (intact, a known flow, DATA, payload <= 1456 B,
// inside its flow's window), else WTP_NOT_PLACED; s is the slot within the flow.  ok[i] != 0
// already says 16 <= recv_len <= stride.  nflows * window <= 2^24, so a global slot is never
// WTP_NOT_PLACED.
__device__ __forceinline__ uint32_t flow_slot(const uint8_t *__restrict__ ring, uint64_t stride,
                                              const uint32_t *__restrict__ recv_len, const uint8_t *__restrict__ ok,
                                              const uint32_t *__restrict__ flow, uint64_t i,
                                              const uint32_t *__restrict__ seq0, uint32_t nflows, uint32_t window,
                                              uint32_t &s, uint32_t &len) {
    const uint8_t good = ok[i];
    const uint32_t rl = recv_len[i];
    const uint32_t f = flow[i];
    if (!good || f >= nflows) return WTP_NOT_PLACED;  // the header is read only where verify saw >= 16 bytes
    const uint8_t *h = ring + i * stride;
    const uint32_t type = be32(h), seq = be32(h + 4);
    len = rl - WTP_HEADER_BYTES;
    s = seq - seq0[f];  // unsigned: wrap is well defined
    return len <= WTP_MAX_PAYLOAD && type == WTP_TYPE_DATA && s < window ? f * window + s : WTP_NOT_PLACED;
}

__global__ void __launch_bounds__(256)
k_flows_claim(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
              const uint8_t *__restrict__ ok, const uint32_t *__restrict__ flow, uint64_t n,
              const uint32_t *__restrict__ seq0, uint32_t nflows, uint32_t window, uint32_t *slot_len, uint32_t *ack) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (ack && i < nflows) ack[i] = seq0[i] + window;  // "no EMPTY slot": k_flows_place lowers it
    if (i >= n) return;
    uint32_t s = 0, len = 0;
    const uint32_t g = flow_slot(ring, stride, recv_len, ok, flow, i, seq0, nflows, window, s, len);
    if (g != WTP_NOT_PLACED) atomicMin(&slot_len[g], kClaim | uint32_t(i));
}

__global__ void __launch_bounds__(256)
k_flows_place(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
              const uint8_t *__restrict__ ok, const uint32_t *__restrict__ flow, uint64_t n,
              const uint32_t *__restrict__ seq0, uint32_t nflows, uint32_t window, uint8_t *__restrict__ out,
              uint32_t *slot_len, uint32_t *__restrict__ place, uint32_t *ack) {
    const uint64_t t = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    // Per-flow cumulative ACK: the first EMPTY slot of every flow.  Every claim made by
    // k_flows_claim is placed below, so a claimed slot counts as filled.  Lane l of a wave
    // looks at global slot base + l; the lanes of its flow in this wave start at lane l -
    // min(s, l), and it reports its slot only if none of them below it is EMPTY too, so a
    // wave makes at most one report per flow it covers.
    if (ack) {
        const uint32_t slots = nflows * window;  // <= WTP_RX_MAX_FLOW_SLOTS
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t step = uint64_t(gridDim.x) * blockDim.x;
        for (uint64_t base = t - lane; base < slots; base += step) {  // uniform over the wave
            const uint32_t g = uint32_t(base) + lane;
            const bool empty = g < slots && __hip_atomic_load(&slot_len[g], __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT) == WTP_SLOT_EMPTY;
            const uint64_t m = __ballot(empty);
            if (empty) {
                const uint32_t f = g / window, s = g - f * window;
                const uint32_t first = lane - min(s, lane);
                const uint64_t mine = (m >> first) << first;           // lanes first .. 63
                if ((mine & ((uint64_t(1) << lane) - 1)) == 0) ack_lower(&ack[f], seq0[f], s);
            }
        }
    }
    const uint64_t i = t / kGroup;
    const uint32_t g = uint32_t(t % kGroup);
    if (i >= n) return;
    uint32_t s = 0, len = 0;
    uint32_t gs = flow_slot(ring, stride, recv_len, ok, flow, i, seq0, nflows, window, s, len);
    // the owner's claim is still in the slot: only this group publishes over it, and it
    // does so after this load (the 16 lanes of a group share a wave)
    if (gs != WTP_NOT_PLACED && slot_len[gs] != (kClaim | uint32_t(i))) gs = WTP_NOT_PLACED;
    if (gs == WTP_NOT_PLACED) {
        if (place && g == 0) place[i] = WTP_NOT_PLACED;
        return;
    }
    const uint8_t *src = ring + i * stride + WTP_HEADER_BYTES;
    uint8_t *dst = out + uint64_t(gs) * WTP_MAX_PAYLOAD;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    copy_slot16<true, true>(src, dst, len, g, vec);
    if (g == 0) {
        slot_len[gs] = len;
        if (place) place[i] = s;  // the slot within the flow
    }
}

// Is datagram i answered?  wtp_rx_build_acks' rule with the flow's base; the header is read
// only where ok says it is there.  f is the datagram's flow where the answer is yes.
__device__ __forceinline__ bool flow_ack_eligible(const uint8_t *__restrict__ ring, uint64_t stride,
                                                  const uint32_t *__restrict__ recv_len,
                                                  const uint8_t *__restrict__ ok, const uint32_t *__restrict__ flow,
                                                  uint32_t i, uint32_t n, const uint32_t *__restrict__ seq0,
                                                  uint32_t nflows, uint32_t window, uint32_t &seq, uint32_t &f) {
    if (i >= n || ok[i] == 0) return false;
    f = flow[i];
    if (f >= nflows) return false;  // no connection
    const uint32_t len = recv_len[i] - WTP_HEADER_BYTES;  // unsigned: a length below 16 is never <= 1456
    const Header hd = load_header(ring + uint64_t(i) * stride);  // type, seq
    seq = hd.seq;
    const uint32_t d = seq - seq0[f];  // unsigned: a wrapping window is well defined
    return hd.type == WTP_TYPE_DATA && len <= WTP_MAX_PAYLOAD && (d < window || d >= 0x80000000u);
}

__global__ void __launch_bounds__(kFlowBlock)
k_flows_ack_mark(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
                 const uint8_t *__restrict__ ok, const uint32_t *__restrict__ flow, uint32_t n,
                 const uint32_t *__restrict__ seq0, uint32_t nflows, uint32_t window, uint32_t *__restrict__ blk) {
    __shared__ uint32_t part[kFlowWaves];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kFlowBlock + t;
    uint32_t seq = 0, f = 0;
    const bool ans = flow_ack_eligible(ring, stride, recv_len, ok, flow, i, n, seq0, nflows, window, seq, f);
    const uint64_t b = __ballot(ans);
    if ((t & 63u) == 0) part[t / 64] = uint32_t(__popcll(b));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kFlowWaves; ++w) sum += part[w];
        blk[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(kFlowBlock)
k_flows_ack_emit(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ recv_len,
                 const uint8_t *__restrict__ ok, const uint32_t *__restrict__ flow, uint32_t n, uint32_t mode,
                 const uint32_t *__restrict__ seq0, uint32_t nflows, uint32_t window,
                 const uint32_t *__restrict__ flow_ack, const uint32_t *__restrict__ blk, uint32_t nblk,
                 uint8_t *__restrict__ wire, uint64_t ack_stride, uint32_t skip, uint32_t max_acks,
                 uint32_t *__restrict__ src, uint32_t *__restrict__ counts) {
    __shared__ uint32_t before[kFlowWaves], all[kFlowWaves], wave_ans[kFlowWaves];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kFlowBlock + t, w = t / 64, lane = t & 63u;
    uint32_t c_before = 0, c_all = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < kFlowCounts; ++k) {
        const uint32_t b = k * kFlowBlock + t;
        const uint32_t c = b < nblk ? blk[b] : 0u;
        c_all += c;
        c_before += b < blockIdx.x ? c : 0u;
    }
    c_before = wave_sum(c_before);
    c_all = wave_sum(c_all);
    uint32_t seq = 0, f = 0;
    const bool ans = flow_ack_eligible(ring, stride, recv_len, ok, flow, i, n, seq0, nflows, window, seq, f);
    const uint64_t ballot = __ballot(ans);
    if (lane == 0) {
        before[w] = c_before;
        all[w] = c_all;
        wave_ans[w] = uint32_t(__popcll(ballot));
    }
    __syncthreads();
    uint32_t rank = 0, total = 0;
    for (uint32_t k = 0; k < kFlowWaves; ++k) {
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
    if (mode == WTP_ACK_CUMULATIVE) seq = flow_ack[f];  // the flow's ACK after the whole batch
    store_ack(wire + uint64_t(k) * ack_stride, seq);
    if (src) src[k] = i;
}

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_rx_build_acks_flows: blk[ceil(n / 1024)].
struct AckFlowsWork {
    uint32_t *blk;
    size_t bytes;
};

AckFlowsWork ack_flows_layout(void *d_work, size_t n) {
    wtp::Work l(d_work, 4);
    uint32_t *blk = l.take<uint32_t>((n + wtp::dev::kFlowBlock - 1) / wtp::dev::kFlowBlock);
    return {blk, l.bytes()};
}

}  // namespace

extern "C" int wtp_accept_data_packets_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                                             const uint32_t *d_flow, size_t n, const uint32_t *d_seq0,
                                             uint32_t nflows, uint32_t window, void *d_out, uint32_t *d_slot_len,
                                             uint8_t *d_ok, uint32_t *d_place, uint32_t *d_ack, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if ((rc = check_stride(stride))) return rc;
    if ((rc = check_flows(nflows, window))) return rc;
    const uint64_t slots = uint64_t(nflows) * window;
    if (n > 0) {
        if (!d_dgrams) return null_arg("d_dgrams");
        if (!d_recv_len) return null_arg("d_recv_len");
        if (!d_flow) return null_arg("d_flow");
        if (!d_ok) return null_arg("d_ok");
        if (!d_out) return null_arg("d_out");
        if (!d_slot_len) return null_arg("d_slot_len");
    }
    if (nflows > 0 && (n > 0 || d_ack) && !d_seq0) return null_arg("d_seq0");
    if (n == 0) {
        if (!d_ack || nflows == 0) return WTP_OK;  // nothing to place, nothing to report
        if (window > 0 && !d_slot_len) return null_arg("d_slot_len");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *ring = static_cast<const uint8_t *>(d_dgrams);
    rc = wtp_crc32_verify_batch(d_dgrams, stride, d_recv_len, n, d_ok, nullptr, stream);
    if (rc) return rc;
    {
        const uint64_t lanes = std::max<uint64_t>(n, d_ack ? nflows : 0);
        const uint64_t blocks = std::max<uint64_t>(1, (lanes + 255) / 256);
        rc = launch("k_flows_claim", dev::k_flows_claim, dim3(unsigned(blocks)), dim3(256), st, ring, uint64_t(stride),
                    d_recv_len, d_ok, d_flow, uint64_t(n), d_seq0, nflows, window, d_slot_len, d_ack);
        if (rc) return rc;
    }
    // one 16-lane group per datagram; at least enough lanes to scan a small state at once
    const uint64_t scan = d_ack ? std::min<uint64_t>((slots + 255) / 256, 1024) : 0;
    const uint64_t blocks = std::max<uint64_t>({1, (uint64_t(n) * dev::kGroup + 255) / 256, scan});
    return launch("k_flows_place", dev::k_flows_place, dim3(unsigned(blocks)), dim3(256), st, ring, uint64_t(stride),
                  d_recv_len, d_ok, d_flow, uint64_t(n), d_seq0, nflows, window, static_cast<uint8_t *>(d_out), d_slot_len,
                  d_place, d_ack);
}

extern "C" size_t wtp_rx_ack_flows_work_bytes(size_t n) {
    return ack_flows_layout(nullptr, std::min<size_t>(n, WTP_RX_MAX_BATCH)).bytes;
}

extern "C" int wtp_rx_build_acks_flows(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len,
                                       const uint32_t *d_flow, size_t n, uint32_t mode, const uint32_t *d_seq0,
                                       uint32_t nflows, uint32_t window, const uint8_t *d_ok,
                                       const uint32_t *d_flow_ack, void *d_ack_wire, size_t ack_stride,
                                       uint32_t skip, uint32_t max_acks, uint32_t *d_src, uint32_t *d_counts,
                                       void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    if (n > WTP_RX_MAX_BATCH) return fail(WTP_EINVAL, "n %zu > %u", n, WTP_RX_MAX_BATCH);
    int rc = check_mode(mode);
    if (rc) return rc;
    const bool cum = mode == WTP_ACK_CUMULATIVE;
    if (cum && window > WTP_RX_MAX_WINDOW) return fail(WTP_EINVAL, "window %u > %u", window, WTP_RX_MAX_WINDOW);
    if ((rc = check_stride(stride))) return rc;
    if (ack_stride < 16) return fail(WTP_EINVAL, "ack_stride %zu < 16", ack_stride);
    const AckFlowsWork w = ack_flows_layout(d_work, n);
    if ((rc = check_work_bytes(work_bytes, w.bytes))) return rc;
    if (!d_counts) return null_arg("d_counts");
    if (!d_work) return null_arg("d_work");
    if (n > 0) {
        if (!d_dgrams) return null_arg("d_dgrams");
        if (!d_recv_len) return null_arg("d_recv_len");
        if (!d_ok) return null_arg("d_ok");
        if (!d_flow) return null_arg("d_flow");
        if (nflows > 0 && !d_seq0) return null_arg("d_seq0");
        if (cum && nflows > 0 && !d_flow_ack) return null_arg("d_flow_ack");
        if (max_acks > 0 && !d_ack_wire) return null_arg("d_ack_wire");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *ring = static_cast<const uint8_t *>(d_dgrams);
    const uint32_t n32 = uint32_t(n), nblk = uint32_t((n + dev::kFlowBlock - 1) / dev::kFlowBlock);
    if (n > 0) {
        rc = launch("k_flows_ack_mark", dev::k_flows_ack_mark, dim3(nblk), dim3(dev::kFlowBlock), st, ring, uint64_t(stride),
                    d_recv_len, d_ok, d_flow, n32, d_seq0, nflows, window, w.blk);
        if (rc) return rc;
    }
    // n == 0: one block, which only writes d_counts = {0, 0}
    return launch("k_flows_ack_emit", dev::k_flows_ack_emit, dim3(std::max(nblk, 1u)), dim3(dev::kFlowBlock), st, ring,
                  uint64_t(stride), d_recv_len, d_ok, d_flow, n32, mode, d_seq0, nflows, window, d_flow_ack, w.blk, nblk,
                  static_cast<uint8_t *>(d_ack_wire), uint64_t(ack_stride), skip, max_acks, d_src, d_counts);
}
