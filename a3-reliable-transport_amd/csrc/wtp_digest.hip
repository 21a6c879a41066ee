// wtp_digest.hip — the running whole-file CRC-32 of every connection (include/wtp_crc32.h:
// wtp_rx_digest_flows): per flow a CRC and a byte count in caller-owned device memory, folded
// each round with the bytes wtp_rx_deliver_flows delivered for the flow, gathered for the flows
// that closed and zeroed for the flows that opened.
//
// A zero-initialised CRC register is linear in the message and leading zero bytes leave it at
// zero, so the raw register of a flow's segment is the XOR of the raw registers of its pieces,
// each times x^(8 * bytes of the segment after the piece); init and xorout enter once per flow
// as (~0) x^(8 bytes) ^ ~0 (plan_edge's initc in wtp_concat.hip).
//
// Units.  With ph = d_stream's address mod 4096, flow f's valid range [B_f, B_f + bytes_f) is
// [s, e) = [ph + B_f, ph + B_f + bytes_f) in coordinates whose origin is the 4-KiB boundary at
// or below d_stream.  It is cut at the multiples of 4096: units floor(s / 4096) .. floor((e - 1)
// / 4096), the first and the last partial, every 16-B vector of a unit aligned in memory
// whatever the phases of d_stream and B_f.  Units are numbered flow-major through the prefix
// sums P[0 .. nflows] of the unit counts (64-bit: ranges may overlap); T = P[nflows].
//
//   1. k_dig_count   one lane per flow: the unit count; sums per 1024 flows
//   2. k_dig_scan    the counts again, scanned behind the earlier blocks' sums: P; acc[f] = 0
//   3. k_dig_hash    a capped persistent grid; wave w owns the contiguous units [w span, (w +
//                    1) span), span = ceil(T / waves).  A unit is 256 vectors: lane l loads
//                    vectors l, l + 64, l + 128, l + 192 (coalesced; a vector that the range
//                    covers in part is masked, and loaded bytewise where it crosses an edge of
//                    the buffer), the vectors go through 4 KiB of LDS per wave (k_build_var's
//                    rotation: both maps free of bank conflicts) and lane l hashes bytes [64 l,
//                    64 l + 64) of the unit in one slice-by-4 chain from registers.  Bytes
//                    outside the range count as zeros: in front they change nothing, behind
//                    the last byte they multiply by a power of x that the flush divides out
//                    again (x^(8 (2^32 - 1)) = 1, so a negative exponent is a positive one).
//                    While the owner flow stays the same the lane registers are carried by
//                    Horner's rule, a_l = a_l x^(8 * 4096) ^ r_l, through the byte-table
//                    operator of that constant (four lookups).  When the owner changes or the
//                    span ends the wave flushes: a_l times the lane constant x^(8 * 64 (63 - l)),
//                    XORed over the wave, times x^(8 * bytes of the flow after the last unit's
//                    end) from k_concat_var's four tables of powers.  A flush for a flow that
//                    lies inside the wave's span is one atomicXor on acc[f]; a wave's first and
//                    last flush, whose flows may go on in the neighbouring waves, are joined per
//                    workgroup in LDS, and the workgroup's own first and last flow leave as two
//                    (flow, value) records, in unit order.
//   4. k_dig_merge   one workgroup: a segmented XOR scan over the records (their flows are in
//                    rising order), one plain XOR into acc[f] per distinct flow.  So the
//                    atomics on one word are at most the waves of one workgroup, and in all
//                    at most (waves of the grid + flows with units): a flow of any size costs
//                    what 64 flows of the same bytes cost.
//   5. k_dig_fold    one lane per flow: crc = (old ^ ~0) x^(8 bytes) ^ acc ^ ~0, bytes += ;
//                    the counts, summed per workgroup
//   6. k_dig_report  the gather for d_report; one lane writes d_counts
//   7. k_dig_reset   zeroes the flows of d_reset
//
// All tables are this unit's own, built at compile time; nothing is allocated and every word
// of d_work that is read was written earlier in the same call.  A separate translation unit:
// see wtp_common.hpp.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_crc_dev.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kDgUnit = 4096;       // bytes of a unit: 256 vectors, four per lane
constexpr uint32_t kDgShift = 12;
constexpr uint32_t kDgPiece = kDgUnit / 64;  // a lane's contiguous bytes of a unit
constexpr uint32_t kDgBlock = 512;       // the hash kernel: eight waves, 44 KiB of LDS
constexpr uint32_t kDgWaves = kDgBlock / 64;
constexpr uint32_t kDgMaxBlocks = 512;   // the capped grid: two workgroups per CU (114 VGPRs)
constexpr uint32_t kDgMinSpan = 4;       // units per wave below which the grid shrinks
constexpr uint32_t kDgFlowBlock = 1024;  // flows per workgroup of the per-flow kernels
constexpr uint32_t kDgFlowWaves = kDgFlowBlock / 64;
constexpr uint32_t kDgMaxFlowBlocks = WTP_RX_MAX_FLOWS / kDgFlowBlock;
constexpr uint32_t kDgMaxRec = 2 * kDgMaxBlocks;
constexpr uint32_t kDgScan = 1024;       // the merge kernel's LDS entries, one per thread
constexpr uint32_t kDgNone = 0xFFFFFFFFu;  // a record without a flow; sorts behind every flow
constexpr uint32_t kDgHdr = 4;           // u64 {bytes folded, flows folded, ranges refused, unused}
constexpr uint32_t kDgListBlocks = 4096; // the capped grid of the two list kernels
static_assert(kDgPiece == 64 && (1u << kDgShift) == kDgUnit && kDgMaxRec <= kDgScan && kDgScan == kDgFlowBlock, "unit");
static_assert(kDgMaxFlowBlocks <= kDgFlowBlock, "k_dig_scan sums the block sums with one load per thread");

__device__ const SliceTable g_dg_table{};  // this unit's own object of the shared type (wtp_crc_dev.hpp)

// The byte-table operator of m = x^(8 * kDgUnit): t[256 k + b] = (b << 8k) * m.
struct DgOperator {
    uint32_t t[1024];
    constexpr DgOperator() : t{} {
        const uint32_t m = gf::xpow8(kDgUnit);
        uint32_t img[32] = {};
        for (uint32_t bit = 0; bit < 32; ++bit) img[bit] = gf::mul(1u << bit, m);
        for (uint32_t k = 0; k < 4; ++k)
            for (uint32_t b = 0; b < 256; ++b)
                for (uint32_t j = 0; j < 8; ++j)
                    if (b & (1u << j)) t[256 * k + b] ^= img[8 * k + j];
    }
};
__device__ const DgOperator g_dg_op{};

// k_concat_var's four tables of powers: t[256 k + b] = x^(8 * b * 2^(8k)).
struct DgPowers {
    uint32_t t[1024];
    constexpr DgPowers() : t{} {
        const gf::Pow8 pw{};
        for (uint32_t k = 0; k < 4; ++k) {
            t[256 * k] = gf::kOne;
            for (uint32_t b = 1; b < 256; ++b) {
                uint32_t j = 0;
                while (!(b & (1u << j))) ++j;
                t[256 * k + b] = gf::mul(t[256 * k + (b & (b - 1))], pw.v[8 * k + j]);
            }
        }
    }
};
__device__ const DgPowers g_dg_pow{};

// c[l] = x^(8 * kDgPiece * (63 - l)): the bytes of a unit behind lane l's piece.
struct DgLanes {
    uint32_t c[64];
    constexpr DgLanes() : c{} {
        const uint32_t step = gf::xpow8(kDgPiece);
        c[63] = gf::kOne;
        for (uint32_t l = 63; l > 0; --l) c[l - 1] = gf::mul(c[l], step);
    }
};
__device__ const DgLanes g_dg_lane{};
static_assert(DgOperator{}.t[0x80] == gf::mul(0x80u, gf::xpow8(kDgUnit)) && DgLanes{}.c[0] == gf::xpow8(kDgUnit - kDgPiece),
              "tables");
static_assert(DgPowers{}.t[3] == gf::xpow8(3) && DgPowers{}.t[256 * 3 + 2] == gf::xpow8(uint64_t(2) << 24), "powers");

// a * x^(8 e) from the four tables of powers (in LDS)
__device__ __forceinline__ uint32_t dg_mul_pow8(uint32_t a, uint32_t e, const uint32_t *X) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b = (e >> (8 * k)) & 255u;
        if (b) a = gf::mul(a, X[256 * k + b]);
    }
    return a;
}

// Flow f's range in unit coordinates, [s, s + bytes), and its unit count; 0 units for a range
// that is refused or empty.  valid: wtp_build_data_packets_var's rule.
__device__ __forceinline__ uint64_t dg_units(const uint64_t *__restrict__ info, uint32_t f, uint64_t stream_bytes, uint32_t ph,
                                             uint64_t &s, uint64_t &bytes, bool &valid) {
    const uint64_t B = info[4 * uint64_t(f) + 2];
    bytes = info[4 * uint64_t(f) + 3];
    valid = B <= stream_bytes && bytes <= stream_bytes - B;
    s = ph + B;  // valid: below 2^64, d_stream + stream_bytes is an address
    return valid && bytes ? ((s + bytes - 1) >> kDgShift) - (s >> kDgShift) + 1 : 0;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The sum of v over the workgroup (kDgFlowBlock threads), in every thread.
__device__ __forceinline__ uint64_t block_sum64(uint64_t v, uint64_t *part) {
    const uint32_t t = threadIdx.x;
    v = wave_sum64(v);
    __syncthreads();  // part may still be read from an earlier call
    if ((t & 63u) == 0) part[t / 64] = v;
    __syncthreads();
    uint64_t sum = 0;
    for (uint32_t w = 0; w < kDgFlowWaves; ++w) sum += part[w];
    return sum;
}

__global__ void __launch_bounds__(kDgFlowBlock)
k_dig_count(const uint64_t *__restrict__ info, uint32_t nflows, uint64_t stream_bytes, uint32_t ph,
            uint64_t *__restrict__ blk) {
    __shared__ uint64_t part[kDgFlowWaves];
    const uint32_t f = blockIdx.x * kDgFlowBlock + threadIdx.x;
    uint64_t s, bytes, u = 0;
    bool valid;
    if (f < nflows) u = dg_units(info, f, stream_bytes, ph, s, bytes, valid);
    const uint64_t sum = block_sum64(u, part);
    if (threadIdx.x == 0) blk[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(kDgFlowBlock)
k_dig_scan(const uint64_t *__restrict__ info, uint32_t nflows, uint64_t stream_bytes, uint32_t ph,
           const uint64_t *__restrict__ blk, uint64_t *__restrict__ P, uint32_t *__restrict__ acc,
           uint64_t *__restrict__ hdr) {
    __shared__ uint64_t part[kDgFlowWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, f = blockIdx.x * kDgFlowBlock + t;
    if (blockIdx.x == 0 && t < kDgHdr) hdr[t] = 0;
    const uint64_t before = block_sum64(t < blockIdx.x ? blk[t] : 0, part);  // gridDim.x <= kDgFlowBlock
    uint64_t s, bytes, u = 0;
    bool valid;
    if (f < nflows) u = dg_units(info, f, stream_bytes, ph, s, bytes, valid);
    uint64_t inc = u;  // inclusive over the wave, then over the workgroup
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    __syncthreads();
    if (lane == 63) part[t / 64] = inc;
    __syncthreads();
    for (uint32_t w = 0; w < t / 64; ++w) inc += part[w];
    if (f < nflows) {
        P[f] = before + inc - u;
        acc[f] = 0;
        if (f == nflows - 1) P[nflows] = before + inc;
    }
}

// Vector `off` (unit coordinates, a multiple of 16) of the stream, the bytes outside the range
// [s, e) as zeros.  The buffer is [ph, bend); p = d_stream - ph, so p + off is the vector's
// address, 16-B aligned.  A vector that the range covers whole is inside the buffer.
__device__ __forceinline__ u32x4 dg_load(const uint8_t *__restrict__ p, uint64_t off, uint64_t s, uint64_t e, uint64_t ph,
                                         uint64_t bend) {
    if (off >= s && off + 16 <= e) return *reinterpret_cast<const u32x4 *>(p + off);
    u32x4 v = {0, 0, 0, 0};
    if (off + 16 <= s || off >= e) return v;
    const uint32_t from = s > off ? uint32_t(s - off) : 0u, to = e < off + 16 ? uint32_t(e - off) : 16u;
    if (off >= ph && off + 16 <= bend) {  // the whole vector is the caller's: load it, mask it
        v = *reinterpret_cast<const u32x4 *>(p + off);
        const uint64_t lo = below_lo(to) & ~below_lo(from), hi = below_hi(to) & ~below_hi(from);
        v.x &= uint32_t(lo);
        v.y &= uint32_t(lo >> 32);
        v.z &= uint32_t(hi);
        v.w &= uint32_t(hi >> 32);
        return v;
    }
    // at an edge of the buffer: the range's own bytes, one by one
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
        if (b >= from && b < to) w[b / 4] |= uint32_t(p[off + b]) << (8 * (b % 4));
    v.x = w[0];
    v.y = w[1];
    v.z = w[2];
    v.w = w[3];
    return v;
}

__global__ void __launch_bounds__(kDgBlock)
k_dig_hash(const uint8_t *__restrict__ stream, uint64_t stream_bytes, const uint64_t *__restrict__ info, uint32_t nflows,
           const uint64_t *__restrict__ P, uint32_t *__restrict__ acc, uint32_t *__restrict__ rec_key,
           uint32_t *__restrict__ rec_val) {
    __shared__ uint32_t tab[1024], op[1024], X[1024];
    __shared__ u32x4 s_move[kDgWaves][kDgUnit / 16];  // per wave: a unit between its loaders and its hashers
    __shared__ uint32_t s_key[2 * kDgWaves], s_val[2 * kDgWaves];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t / 64;
    for (uint32_t i = t; i < 1024; i += kDgBlock) {
        tab[i] = (&g_dg_table.t[0][0])[i];
        op[i] = g_dg_op.t[i];
        X[i] = g_dg_pow.t[i];
    }
    const uint32_t clane = g_dg_lane.c[lane];
    const uint64_t ph = reinterpret_cast<uintptr_t>(stream) & (kDgUnit - 1), bend = ph + stream_bytes;
    const uint8_t *__restrict__ p = stream - ph;  // unit coordinate 0; only addresses inside the buffer are formed from it
    __syncthreads();  // the tables are there; until the records the waves run on their own
    const uint64_t T = P[nflows];
    const uint64_t nw = uint64_t(gridDim.x) * kDgWaves, span = (T + nw - 1) / nw;
    const uint64_t w = uint64_t(blockIdx.x) * kDgWaves + wv;
    const uint64_t t0 = w * span < T ? w * span : T, t1 = t0 + span < T ? t0 + span : T;  // w * span < T + nw
    uint32_t head_key = kDgNone, head_val = 0, tail_key = kDgNone, tail_val = 0;
    if (t0 < t1) {
        uint32_t f = __builtin_amdgcn_readfirstlane(owner_wave(P, nflows, t0, lane));  // t0 < T: f < nflows
        uint64_t u = t0;
        while (u < t1) {
            const uint64_t pf = P[f], fend = P[f + 1];
            const uint64_t s = ph + info[4 * uint64_t(f) + 2], e = s + info[4 * uint64_t(f) + 3];
            const uint64_t run_end = fend < t1 ? fend : t1;
            uint64_t n = (s >> kDgShift) + (u - pf);  // the unit's number in unit coordinates
            uint32_t a = 0;
            for (; u < run_end; ++u, ++n) {
                const uint64_t ub = n << kDgShift;
                u32x4 v[4];
                if (ub >= s && ub + kDgUnit <= e) {  // wave-uniform: an inner unit
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const u32x4 *>(p + ub + 16 * (64 * j + lane));
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) v[j] = dg_load(p, ub + 16 * (64 * j + lane), s, e, ph, bend);
                }
                // piece q = 16 j + lane / 4 of the unit, vector m = lane % 4, in slot (m + q / 4) % 4 of its 64 bytes
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    s_move[wv][4 * (16 * j + lane / 4) + (((lane & 3u) + 4 * j + lane / 16) & 3u)] = v[j];
                wave_sync();
                uint32_t c = 0;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const u32x4 x = s_move[wv][4 * lane + ((k + lane / 4) & 3u)];
                    c = crc_word(tab, c, x.x);
                    c = crc_word(tab, c, x.y);
                    c = crc_word(tab, c, x.z);
                    c = crc_word(tab, c, x.w);
                }
                a = op[a & 255u] ^ op[256 + ((a >> 8) & 255u)] ^ op[512 + ((a >> 16) & 255u)] ^ op[768 + (a >> 24)] ^ c;
                wave_sync();  // the next unit's s_move stores follow these loads
            }
            // the flush: the run ends at unit coordinate n * 4096, the flow at e (before it only in the last unit)
            const uint64_t rend = n << kDgShift;
            const uint32_t ex = e >= rend ? uint32_t((e - rend) % gf::kOrder) : gf::kOrder - uint32_t(rend - e);
            uint32_t val = gf::mul(a, clane);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) val ^= __shfl_xor(val, d, 64);
            val = dg_mul_pow8(val, ex, X);
            if (head_key == kDgNone) {
                head_key = f;
                head_val = val;
            } else if (u == t1) {
                tail_key = f;
                tail_val = val;
            } else if (lane == 0) {
                atomicXor(&acc[f], val);  // the flow begins and ends inside this wave's span
            }
            if (u < t1) {  // u == P[f + 1]: the next flow with units, among the next 64 or by the search
                const uint32_t idx = f + 1 + lane;
                const bool le = idx <= nflows && P[idx] <= u;
                const uint32_t cnt = uint32_t(__popcll(__ballot(le)));  // P is monotone: a prefix of the lanes, >= 1
                f = cnt < 64 ? f + cnt : __builtin_amdgcn_readfirstlane(owner_wave(P, nflows, u, lane));
            }
        }
    }
    if (tail_key == kDgNone) tail_key = head_key;  // keeps the keys in rising order
    if (lane == 0) {
        s_key[2 * wv] = head_key;
        s_val[2 * wv] = head_val;
        s_key[2 * wv + 1] = tail_key;
        s_val[2 * wv + 1] = tail_val;
    }
    __syncthreads();
    if (t == 0) {
        // the workgroup's first and last flow may go on in its neighbours: two records; what lies
        // strictly between them is this workgroup's alone
        const uint32_t k0 = s_key[0], k1 = s_key[2 * kDgWaves - 1];
        uint32_t v0 = 0, v1 = 0;
        for (uint32_t i = 0; i < 2 * kDgWaves; ++i) {
            const uint32_t k = s_key[i], x = s_val[i];
            if (k == k0)
                v0 ^= x;
            else if (k == k1)
                v1 ^= x;
            else if (x)
                atomicXor(&acc[k], x);  // k0 < k < k1: a flow
        }
        rec_key[2 * blockIdx.x] = k0;
        rec_val[2 * blockIdx.x] = v0;
        rec_key[2 * blockIdx.x + 1] = k1;
        rec_val[2 * blockIdx.x + 1] = v1;
    }
}

// nrec <= kDgMaxRec records whose keys rise; kDgNone holds no flow.
__global__ void __launch_bounds__(kDgFlowBlock)
k_dig_merge(const uint32_t *__restrict__ rec_key, const uint32_t *__restrict__ rec_val, uint32_t nrec,
            uint32_t *__restrict__ acc) {
    __shared__ uint32_t key[kDgScan], val[kDgScan];
    const uint32_t t = threadIdx.x;
    const uint32_t k = t < nrec ? rec_key[t] : kDgNone;
    key[t] = k;
    val[t] = t < nrec ? rec_val[t] : 0u;
    __syncthreads();
    // equal keys are neighbours, so key[t - d] == key[t] says that everything between is the same flow
    for (uint32_t d = 1; d < kDgScan; d <<= 1) {
        const uint32_t x = t >= d && key[t - d] == k ? val[t - d] : 0u;
        __syncthreads();
        val[t] ^= x;
        __syncthreads();
    }
    if (k != kDgNone && (t + 1 == kDgScan || key[t + 1] != k) && val[t]) acc[k] ^= val[t];  // the flow's last record
}

__global__ void __launch_bounds__(kDgFlowBlock)
k_dig_fold(const uint64_t *__restrict__ info, uint32_t nflows, uint64_t stream_bytes, const uint32_t *__restrict__ acc,
           uint32_t *__restrict__ flow_crc, uint64_t *__restrict__ flow_bytes, uint64_t *__restrict__ hdr) {
    __shared__ uint32_t X[1024];
    __shared__ uint64_t part[kDgFlowWaves];
    const uint32_t t = threadIdx.x, f = blockIdx.x * kDgFlowBlock + t;
    X[t] = g_dg_pow.t[t];
    __syncthreads();
    uint64_t s, bytes = 0;
    bool valid = true;
    if (f < nflows) dg_units(info, f, stream_bytes, 0u, s, bytes, valid);
    const bool folded = f < nflows && valid && bytes > 0;
    if (folded) {
        flow_crc[f] = dg_mul_pow8(~flow_crc[f], uint32_t(bytes % gf::kOrder), X) ^ acc[f] ^ 0xFFFFFFFFu;
        flow_bytes[f] += bytes;
    }
    const uint64_t nbytes = block_sum64(folded ? bytes : 0, part), nfolded = block_sum64(folded, part);
    const uint64_t nrefused = block_sum64(!valid, part);
    const uint64_t mine = t == 0 ? nbytes : t == 1 ? nfolded : nrefused;  // one atomic per workgroup and count
    if (t < 3 && mine) atomicAdd(reinterpret_cast<unsigned long long *>(&hdr[t]), static_cast<unsigned long long>(mine));
}

// hdr == NULL: nflows == 0, nothing was folded.  list == NULL: no report list.
__global__ void __launch_bounds__(256)
k_dig_report(const uint32_t *__restrict__ list, const uint32_t *__restrict__ count, uint32_t max_list, uint32_t nflows,
             const uint32_t *__restrict__ flow_crc, const uint64_t *__restrict__ flow_bytes,
             uint32_t *__restrict__ out_crc, uint64_t *__restrict__ out_bytes, const uint64_t *__restrict__ hdr,
             uint64_t *__restrict__ counts) {
    const uint32_t k = list ? min(*count, max_list) : 0u;
    for (uint64_t q = blockIdx.x * 256u + threadIdx.x; q < k; q += uint64_t(gridDim.x) * 256u) {
        const uint32_t g = list[q];
        out_crc[q] = g < nflows ? flow_crc[g] : 0u;
        out_bytes[q] = g < nflows ? flow_bytes[g] : ~uint64_t(0);
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) counts[threadIdx.x] = threadIdx.x == 3 ? k : hdr ? hdr[threadIdx.x] : 0;
}

__global__ void __launch_bounds__(256)
k_dig_reset(const uint32_t *__restrict__ list, const uint32_t *__restrict__ count, uint32_t max_list, uint32_t nflows,
            uint32_t *__restrict__ flow_crc, uint64_t *__restrict__ flow_bytes) {
    const uint32_t k = min(*count, max_list);
    for (uint64_t j = blockIdx.x * 256u + threadIdx.x; j < k; j += uint64_t(gridDim.x) * 256u) {
        const uint32_t g = list[j];
        if (g < nflows) {  // duplicates store the same zeros
            flow_crc[g] = 0;
            flow_bytes[g] = 0;
        }
    }
}

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_rx_digest_flows: hdr[4], blk[1024], P[nflows + 1] (u64), then the records'
// flows and values [1024 each] and acc[nflows] (u32).
struct DigestWork {
    uint64_t *hdr, *blk, *P;
    uint32_t *rec_key, *rec_val, *acc;
    size_t bytes;
};

DigestWork digest_layout(void *d_work, uint32_t nflows) {
    wtp::Work l(d_work, 8);
    DigestWork w;
    w.hdr = l.take<uint64_t>(wtp::dev::kDgHdr);
    w.blk = l.take<uint64_t>(wtp::dev::kDgMaxFlowBlocks);
    w.P = l.take<uint64_t>(size_t(nflows) + 1);
    w.rec_key = l.take<uint32_t>(wtp::dev::kDgMaxRec);
    w.rec_val = l.take<uint32_t>(wtp::dev::kDgMaxRec);
    w.acc = l.take<uint32_t>(nflows);
    w.bytes = l.bytes();
    return w;
}

unsigned list_blocks(uint32_t max_list) {
    return std::min(wtp::dev::kDgListBlocks, max_list / 256u + 1u);
}

}  // namespace

extern "C" size_t wtp_rx_digest_scratch_bytes(uint32_t nflows) {
    return digest_layout(nullptr, std::min(nflows, WTP_RX_MAX_FLOWS)).bytes;
}

extern "C" int wtp_rx_digest_flows(const void *d_stream, size_t stream_bytes, const uint64_t *d_flow_info, uint32_t nflows,
                                   uint32_t *d_flow_crc, uint64_t *d_flow_bytes, const uint32_t *d_reset,
                                   const uint32_t *d_reset_count, uint32_t max_reset, const uint32_t *d_report,
                                   const uint32_t *d_report_count, uint32_t max_report, uint32_t *d_report_crc,
                                   uint64_t *d_report_bytes, uint64_t *d_counts, void *d_work, size_t work_bytes,
                                   void *stream) {
    using namespace wtp;
    if (nflows > WTP_RX_MAX_FLOWS) return fail(WTP_EINVAL, "nflows %u > %u", nflows, WTP_RX_MAX_FLOWS);
    const DigestWork w = digest_layout(d_work, nflows);
    int rc = check_work_bytes(work_bytes, w.bytes);
    if (rc) return rc;
    if (!d_counts) return null_arg("d_counts");
    if (!d_work) return null_arg("d_work");
    if (nflows > 0) {
        if (!d_flow_info) return null_arg("d_flow_info");
        if (!d_flow_crc) return null_arg("d_flow_crc");
        if (!d_flow_bytes) return null_arg("d_flow_bytes");
        if (stream_bytes > 0 && !d_stream) return null_arg("d_stream");
    }
    if (!d_reset != !d_reset_count) return fail(WTP_EINVAL, "exactly one of d_reset and d_reset_count is null");
    if (!d_report != !d_report_count) return fail(WTP_EINVAL, "exactly one of d_report and d_report_count is null");
    if (d_report && max_report > 0) {
        if (!d_report_crc) return null_arg("d_report_crc");
        if (!d_report_bytes) return null_arg("d_report_bytes");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nflows > 0) {
        const uint8_t *base = static_cast<const uint8_t *>(d_stream);
        const uint32_t ph = uint32_t(reinterpret_cast<uintptr_t>(base) & (dev::kDgUnit - 1));
        const dim3 per_flow((nflows + dev::kDgFlowBlock - 1) / dev::kDgFlowBlock), flow_block(dev::kDgFlowBlock);
        // the hash grid from host values: the units of ranges that do not overlap, kDgMinSpan a wave
        const uint64_t units = uint64_t(stream_bytes) / dev::kDgUnit + 2 * uint64_t(nflows);
        const uint64_t per_block = uint64_t(dev::kDgWaves) * dev::kDgMinSpan;
        const unsigned blocks = unsigned(std::min<uint64_t>(dev::kDgMaxBlocks, (units + per_block - 1) / per_block));
        rc = launch("k_dig_count", dev::k_dig_count, per_flow, flow_block, st, d_flow_info, nflows, uint64_t(stream_bytes), ph,
                    w.blk);
        if (rc) return rc;
        rc = launch("k_dig_scan", dev::k_dig_scan, per_flow, flow_block, st, d_flow_info, nflows, uint64_t(stream_bytes), ph,
                    w.blk, w.P, w.acc, w.hdr);
        if (rc) return rc;
        rc = launch("k_dig_hash", dev::k_dig_hash, dim3(blocks), dim3(dev::kDgBlock), st, base, uint64_t(stream_bytes),
                    d_flow_info, nflows, w.P, w.acc, w.rec_key, w.rec_val);
        if (rc) return rc;
        rc = launch("k_dig_merge", dev::k_dig_merge, dim3(1), flow_block, st, w.rec_key, w.rec_val, 2 * blocks, w.acc);
        if (rc) return rc;
        rc = launch("k_dig_fold", dev::k_dig_fold, per_flow, flow_block, st, d_flow_info, nflows, uint64_t(stream_bytes), w.acc,
                    d_flow_crc, d_flow_bytes, w.hdr);
        if (rc) return rc;
    }
    const uint32_t nrep = d_report ? max_report : 0u;
    rc = launch("k_dig_report", dev::k_dig_report, dim3(list_blocks(nrep)), dim3(256), st, nrep ? d_report : nullptr,
                d_report_count, nrep, nflows, d_flow_crc, d_flow_bytes, d_report_crc, d_report_bytes,
                nflows > 0 ? w.hdr : nullptr, d_counts);
    if (rc || !d_reset || max_reset == 0 || nflows == 0) return rc;
    return launch("k_dig_reset", dev::k_dig_reset, dim3(list_blocks(max_reset)), dim3(256), st, d_reset, d_reset_count,
                  max_reset, nflows, d_flow_crc, d_flow_bytes);
}
