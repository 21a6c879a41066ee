// wtp_buildvar.hip — fused DATA builder for mixed-length payloads (include/wtp_crc32.h:
// wtp_build_data_packets_var), the sender-side counterpart of what wtp_accept.hip does
// for every payload length.
//
// One stream-ordered launch, no scratch, no library table (so no wtp_init):
//   k_build_var     a wave takes 64 datagrams per round, one lane per datagram for the
//                   metadata (coalesced offset / length loads, the validity test), and cuts
//                   the valid payloads into pieces of 64 B (four destination-aligned 16-B
//                   vectors; the last piece of a payload is shorter).  A prefix sum of the
//                   piece counts over the wave numbers the pieces of the round and the 64
//                   lanes take them in turns (piece p, p + 64, ...), one piece per lane: a
//                   round of 64 four-byte payloads and a round of 1456-byte ones keep the
//                   same share of lanes busy (16 lanes per datagram, k_tx_emit's shape, leave
//                   15 of 16 idle on a 4-byte payload).  A lane finds the owner of its piece
//                   by a binary search of the prefix sums (LDS).  After the tables are in
//                   LDS the waves of a workgroup never wait for each other.
//                   The move and the hash of a turn use two lane-to-byte maps, joined by a
//                   4-KiB LDS buffer per wave.  The move: lanes 4m .. 4m + 3 take the four
//                   vectors of lane m's piece (16 pieces per step, four steps, all loads
//                   issued before the first use), so consecutive lanes load and store
//                   consecutive 16-B vectors.  The source has any byte alignment: a lane
//                   loads the four dwords that hold its vector from the 4-B aligned address
//                   below it (one 16-B load, which needs no more than dword alignment) plus
//                   the dword that follows, and v_alignbyte_b32 by (address & 3) yields the
//                   destination-aligned vector.  These widened loads are issued only when
//                   all of their bytes lie inside [d_base, d_base + base_bytes); a vector
//                   within 20 bytes of either edge of the buffer is gathered bytewise from the
//                   payload's own bytes.  The last vector of a payload is stored as dwords
//                   and bytes, so the slot's tail is not touched.  The vector then goes to
//                   LDS (slot rotated by piece / 4: both maps are free of bank conflicts).
//                   The hash: a lane reads its own piece back, 64 contiguous bytes, and
//                   hashes them from registers in one chain (slice-by-4, tables in LDS, built
//                   at compile time; the last vector over its len % 16 bytes only).
//                   The piece CRCs combine as in k_tx_emit, crc = xor of crc_q * x^(8 * bytes
//                   after piece q), but the multipliers depend on len.  With r = the last
//                   piece's byte count (1 .. 64) the bytes after piece q are 64 * (np - 2 -
//                   q) + r, so a lane multiplies by x^(8 * 64 k) from a 23-entry LDS table,
//                   the products xor into the datagram's LDS accumulator (ds_xor), and the
//                   owner lane multiplies the sum once by x^(8 r) (65 entries) and adds the
//                   last piece's CRC: no square-and-multiply anywhere.  The owner lane then
//                   stores the 16-B header, d_wire_len and d_crc_out.
//                   What was tried before: one vector per lane and turn
//                   (fully coalesced, but a GF(2) multiply of about 200 VALU instructions
//                   and an owner search per 16 bytes); the same with four vectors in flight;
//                   a lane moving its own 64 contiguous bytes (one multiply per 64 bytes,
//                   but lanes 64 B apart in every load and store: slower than either).
//                   A wire ring that is not 16-B aligned, or a stride that is no multiple of
//                   16, takes the same loads and bytewise stores.
//
// A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_crc_dev.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kBvBlock = 256;                      // four waves, each with rounds of 64 datagrams
constexpr uint32_t kBvWaves = kBvBlock / 64;
constexpr uint32_t kBvVecs = 4;                         // 16-B vectors per piece
constexpr uint32_t kBvPiece = 16 * kBvVecs;             // a lane's contiguous bytes per turn
constexpr uint32_t kBvMaxPieces = (WTP_MAX_PAYLOAD + kBvPiece - 1) / kBvPiece;  // 23
constexpr uint32_t kBvMaxBlocks = 1280;                 // the capped grid: 5 workgroups per CU (96 VGPRs, 27 KB LDS)

__device__ const SliceTable g_bv_table{};  // this unit's own object of the shared type (wtp_crc_dev.hpp)

// piece[k] = x^(8 * kBvPiece * k), k whole pieces after a piece; byte[r] = x^(8 * r), r <= kBvPiece
struct BvPow {
    uint32_t piece[kBvMaxPieces];
    uint32_t byte[kBvPiece + 1];
    constexpr BvPow() : piece{}, byte{} {
        const uint32_t x8 = gf::kOne >> 8;
        byte[0] = gf::kOne;
        for (uint32_t r = 1; r <= kBvPiece; ++r) byte[r] = gf::mul(byte[r - 1], x8);
        piece[0] = gf::kOne;
        for (uint32_t k = 1; k < kBvMaxPieces; ++k) piece[k] = gf::mul(piece[k - 1], byte[kBvPiece]);
    }
};
__device__ const BvPow g_bv_pow{};
static_assert(BvPow{}.byte[kBvPiece] == gf::xpow8(kBvPiece) &&
                  BvPow{}.piece[kBvMaxPieces - 1] == gf::xpow8(kBvPiece * (kBvMaxPieces - 1)),
              "powers");

__global__ void __launch_bounds__(kBvBlock)
k_build_var(const uint8_t *__restrict__ base, uint64_t base_bytes, const uint64_t *__restrict__ offs,
            const uint32_t *__restrict__ lens, uint32_t n, uint32_t seq0, uint8_t *__restrict__ wire, uint64_t stride,
            uint32_t vec, uint32_t *__restrict__ wire_len, uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t tab[4 * 256];
    __shared__ uint32_t ppiece[kBvMaxPieces], pbyte[kBvPiece + 1];
    __shared__ uint32_t s_end[kBvWaves][64], s_lo[kBvWaves][64], s_hi[kBvWaves][64], s_len[kBvWaves][64];
    __shared__ uint32_t s_acc[kBvWaves][64], s_last[kBvWaves][64];
    __shared__ u32x4 s_move[kBvWaves][64 * kBvVecs];  // per wave: 64 pieces between their movers and their hasher
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t / 64;
    for (uint32_t i = t; i < 4 * 256; i += kBvBlock) tab[i] = (&g_bv_table.t[0][0])[i];
    if (t < kBvMaxPieces) ppiece[t] = g_bv_pow.piece[t];
    if (t <= kBvPiece) pbyte[t] = g_bv_pow.byte[t];
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), hi = lo + base_bytes;
    __syncthreads();  // the tables are there; from here on the waves run on their own
    const uint32_t rounds = (n + 63) / 64, step_r = gridDim.x * kBvWaves;
    for (uint32_t r = blockIdx.x * kBvWaves + wv; r < rounds; r += step_r) {
        const uint32_t i = r * 64 + lane;  // n < 2^31
        uint32_t len = 0;
        uint64_t off = 0;
        bool valid = false;
        if (i < n) {
            off = offs[i];
            len = lens[i];
            valid = len <= WTP_MAX_PAYLOAD && off <= base_bytes && len <= base_bytes - off;
        }
        const uint32_t np = valid ? (len + kBvPiece - 1) / kBvPiece : 0;
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
                onp = (olen + kBvPiece - 1) / kBvPiece;
                q = task - (s_end[wv][o] - onp);                 // piece q of onp
                nbytes = min(kBvPiece, olen - kBvPiece * q);  // 1 .. 64, below 64 only in the last
                soff = ((uint64_t(s_hi[wv][o]) << 32) | s_lo[wv][o]) + kBvPiece * q;
                doff = uint64_t(r * 64 + o) * stride + WTP_HEADER_BYTES + kBvPiece * q;
            }
            // the move: in turn u, lanes 4m .. 4m + 3 take the four vectors of the piece of lane
            // 16u + m, so a wave's loads and stores of consecutive pieces are contiguous
            const uint32_t m = lane & 3u;
            uint32_t nbv[kBvVecs], shv[kBvVecs];
            const uint8_t *sp[kBvVecs];
            uint8_t *dp[kBvVecs];
            bool fast[kBvVecs];
#pragma unroll
            for (uint32_t u = 0; u < kBvVecs; ++u) {
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
            u32x4 d[kBvVecs] = {};
            uint32_t e[kBvVecs] = {};
#pragma unroll
            for (uint32_t u = 0; u < kBvVecs; ++u)
                if (fast[u]) {
                    const uint8_t *p = sp[u] - shv[u];  // the dword that holds the first byte
                    d[u] = *reinterpret_cast<const u32x4_a4 *>(p);
                    e[u] = *reinterpret_cast<const uint32_t *>(p + (shv[u] ? 16 : 12));  // sh == 0: d.w again, unused
                }
#pragma unroll
            for (uint32_t u = 0; u < kBvVecs; ++u) {
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
            for (uint32_t k = 0; k < kBvVecs; ++k) {
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
        if (i < n) {
            uint32_t crc = 0;
            if (valid) {
                if (len) crc = gf::mul(s_acc[wv][lane], pbyte[len - kBvPiece * (np - 1)]) ^ s_last[wv][lane] ^ 0xFFFFFFFFu;
                uint8_t *slot = wire + uint64_t(i) * stride;
                const u32x4 h = header_be(WTP_TYPE_DATA, seq0 + i, len, crc);
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

extern "C" int wtp_build_data_packets_var(const void *d_base, size_t base_bytes, const uint64_t *d_offsets,
                                          const uint32_t *d_lengths, size_t n, uint32_t seq0, void *d_wire,
                                          size_t wire_stride, uint32_t *d_wire_len, uint32_t *d_crc_out, void *stream) {
    using namespace wtp;
    if (wire_stride < WTP_HEADER_BYTES + WTP_MAX_PAYLOAD) return fail(WTP_EINVAL, "wire_stride %zu < 1472", wire_stride);
    const int rc = check_batch(n);
    if (rc) return rc;
    if (n == 0) return WTP_OK;
    if (!d_base || !d_offsets || !d_lengths || !d_wire) return fail(WTP_EINVAL, "null pointer");
    const uint32_t vec = (reinterpret_cast<uintptr_t>(d_wire) & 15u) == 0 && wire_stride % 16 == 0;
    const uint64_t rounds = (uint64_t(n) + dev::kBvBlock - 1) / dev::kBvBlock;  // of a workgroup: one of 64 per wave
    const unsigned blocks = unsigned(std::min<uint64_t>(rounds, dev::kBvMaxBlocks));
    return launch("k_build_var", dev::k_build_var, dim3(blocks), dim3(dev::kBvBlock), static_cast<hipStream_t>(stream),
                  static_cast<const uint8_t *>(d_base), uint64_t(base_bytes), d_offsets, d_lengths, uint32_t(n), seq0,
                  static_cast<uint8_t *>(d_wire), uint64_t(wire_stride), vec, d_wire_len, d_crc_out);
}
