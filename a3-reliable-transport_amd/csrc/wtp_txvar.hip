// wtp_txvar.hip — the emit pass of wtp_tx_build_retransmit_var (include/wtp_crc32.h): the
// sender window's ordered selection (wtp_tx.hip: k_tx_count, k_tx_select, unchanged) in
// front of the mixed-length builder's move-and-hash scheme.
//
//   k_tx_emit_var   k_build_var's body (the scheme is described at the top of wtp_buildvar.hip)
//                   with two changes.  The index map: datagram k of the ring is record
//                   picked[k] of d_work, one more coalesced load per datagram in the metadata
//                   phase; its header carries seq0 + picked[k] and it fills wire slot k.  The
//                   datagram count is min(d_counts[0], max_sel), one uniform load per wave:
//                   the host never reads it.  The round size: the builder hands a wave 64
//                   datagrams per round, right for a million payloads and wrong for a
//                   retransmit set (658 full-size datagrams would sit in 11 waves for 23
//                   turns each).  Here a round is G datagrams, G the smallest power of two for
//                   which G * (waves of the grid) covers the count, at most 64, and the grid
//                   is one wave per ring entry up to the builder's cap of 1280 workgroups =
//                   5120 waves.  So G = 1 up to 5120 emitted datagrams, whatever the ring, 2
//                   up to 10 240, ... 16 for a whole window of 65 536, 64 above 163 840.  A
//                   workgroup whose first datagram is past the count leaves at once (its
//                   table loads are in flight by then: they are issued before the count's, so
//                   that a working group waits for both at once); a lane past the count
//                   writes nothing.
//
// Its own copy of the body, not a header shared with wtp_buildvar.hip: as a template in a
// header (index map and round size as parameters, the builder's instance with identity and
// 64) the body compiled to other machine code for k_build_var, and so did the parent's body
// moved unchanged into an inline function; in an A/B of the two builds, alternated twice, the
// builder's 1 M x 1456 B case came out 1.4 % and 4 % slower, outside its interquartile range
// (DESIGN.md 3.12).  So k_build_var stays as it is, as in DESIGN.md 3.8.
//
// A translation unit of its own: wtp_tx.hip's kernels keep their machine code (a kernel
// added there moves their tables), and so does everything else (wtp_common.hpp).  The entry
// point, its checks and the two selection launches are in wtp_tx.hip, which calls
// tx_emit_var_launch below: a host call, no relocatable device code.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_crc_dev.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kTvBlock = 256;                      // four waves, each with rounds of 64 datagrams
constexpr uint32_t kTvWaves = kTvBlock / 64;
constexpr uint32_t kTvVecs = 4;                         // 16-B vectors per piece
constexpr uint32_t kTvPiece = 16 * kTvVecs;             // a lane's contiguous bytes per turn
constexpr uint32_t kTvMaxPieces = (WTP_MAX_PAYLOAD + kTvPiece - 1) / kTvPiece;  // 23
constexpr uint32_t kTvMaxBlocks = 1280;                 // the capped grid: 5 workgroups per CU (96 VGPRs, 27 KB LDS)

__device__ const SliceTable g_tv_table{};  // this unit's own object of the shared type (wtp_crc_dev.hpp)

// One table, so that a workgroup fills it with one load per lane: v[k] = x^(8 * kTvPiece * k), k
// whole pieces after a piece, k < kTvMaxPieces; v[kTvMaxPieces + r] = x^(8 * r), r <= kTvPiece
constexpr uint32_t kTvPows = kTvMaxPieces + kTvPiece + 1;
struct TvPow {
    uint32_t v[kTvPows];
    constexpr TvPow() : v{} {
        const uint32_t x8 = gf::kOne >> 8;
        uint32_t *piece = v, *byte = v + kTvMaxPieces;
        byte[0] = gf::kOne;
        for (uint32_t r = 1; r <= kTvPiece; ++r) byte[r] = gf::mul(byte[r - 1], x8);
        piece[0] = gf::kOne;
        for (uint32_t k = 1; k < kTvMaxPieces; ++k) piece[k] = gf::mul(piece[k - 1], byte[kTvPiece]);
    }
};
__device__ const TvPow g_tv_pow{};
static_assert(TvPow{}.v[kTvMaxPieces + kTvPiece] == gf::xpow8(kTvPiece) &&
                  TvPow{}.v[kTvMaxPieces - 1] == gf::xpow8(kTvPiece * (kTvMaxPieces - 1)) && kTvPows <= kTvBlock,
              "powers");

// Datagram k < min(counts[0], max_sel) is record picked[k] and fills wire slot k.
__global__ void __launch_bounds__(kTvBlock, 5)  // five waves per SIMD: the capped grid is five workgroups per CU
k_tx_emit_var(const uint8_t *__restrict__ base, uint64_t base_bytes, const uint64_t *__restrict__ offs,
              const uint32_t *__restrict__ lens, uint32_t max_sel, uint32_t seq0, const uint32_t *__restrict__ picked,
              const uint32_t *__restrict__ counts, uint8_t *__restrict__ wire, uint64_t stride, uint32_t vec,
              uint32_t *__restrict__ wire_len, uint32_t *__restrict__ crc_out) {
    __shared__ uint32_t tab[4 * 256];
    __shared__ uint32_t pows[kTvPows];
    const uint32_t *ppiece = pows, *pbyte = pows + kTvMaxPieces;
    __shared__ uint32_t s_end[kTvWaves][64], s_lo[kTvWaves][64], s_hi[kTvWaves][64], s_len[kTvWaves][64];
    __shared__ uint32_t s_acc[kTvWaves][64], s_last[kTvWaves][64];
    __shared__ u32x4 s_move[kTvWaves][64 * kTvVecs];  // per wave: 64 pieces between their movers and their hasher
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t / 64;
    // the tables' loads are issued before the count's, so the two latencies overlap; a
    // workgroup that leaves has loaded 4 KiB it did not need
    uint32_t tv[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tv[k] = (&g_tv_table.t[0][0])[t + k * kTvBlock];
    const uint32_t pv = g_tv_pow.v[t < kTvPows ? t : 0];
    const uint32_t n = min(counts[0], max_sel);
    const uint32_t waves = gridDim.x * kTvWaves;
    uint32_t g = 0;  // log2 of the round size
    while (g < 6 && (uint64_t(waves) << g) < n) ++g;
    if ((uint64_t(blockIdx.x) * kTvWaves << g) >= n) return;  // the whole workgroup
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tab[t + k * kTvBlock] = tv[k];
    if (t < kTvPows) pows[t] = pv;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), hi = lo + base_bytes;
    __syncthreads();  // the tables are there; from here on the waves run on their own
    const uint32_t rounds = uint32_t((uint64_t(n) + (1u << g) - 1) >> g);
    const uint32_t step_r = gridDim.x * kTvWaves;
    for (uint32_t r = blockIdx.x * kTvWaves + wv; r < rounds; r += step_r) {
        const uint32_t i = (r << g) + lane;  // datagram i of the ring, n <= 2^20
        const bool has = (lane >> g) == 0 && i < n;  // lanes >= G carry no datagram
        uint32_t len = 0, rec = 0;
        uint64_t off = 0;
        bool valid = false;
        if (has) {
            rec = picked[i];  // the slot, and the record
            off = offs[rec];
            len = lens[rec];
            valid = len <= WTP_MAX_PAYLOAD && off <= base_bytes && len <= base_bytes - off;
        }
        const uint32_t np = valid ? (len + kTvPiece - 1) / kTvPiece : 0;
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
                onp = (olen + kTvPiece - 1) / kTvPiece;
                q = task - (s_end[wv][o] - onp);                 // piece q of onp
                nbytes = min(kTvPiece, olen - kTvPiece * q);  // 1 .. 64, below 64 only in the last
                soff = ((uint64_t(s_hi[wv][o]) << 32) | s_lo[wv][o]) + kTvPiece * q;
                doff = uint64_t((r << g) + o) * stride + WTP_HEADER_BYTES + kTvPiece * q;
            }
            // the move: in turn u, lanes 4m .. 4m + 3 take the four vectors of the piece of lane
            // 16u + m, so a wave's loads and stores of consecutive pieces are contiguous
            const uint32_t m = lane & 3u;
            uint32_t nbv[kTvVecs], shv[kTvVecs];
            const uint8_t *sp[kTvVecs];
            uint8_t *dp[kTvVecs];
            bool fast[kTvVecs];
#pragma unroll
            for (uint32_t u = 0; u < kTvVecs; ++u) {
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
            u32x4 d[kTvVecs] = {};
            uint32_t e[kTvVecs] = {};
#pragma unroll
            for (uint32_t u = 0; u < kTvVecs; ++u)
                if (fast[u]) {
                    const uint8_t *p = sp[u] - shv[u];  // the dword that holds the first byte
                    d[u] = *reinterpret_cast<const u32x4_a4 *>(p);
                    e[u] = *reinterpret_cast<const uint32_t *>(p + (shv[u] ? 16 : 12));  // sh == 0: d.w again, unused
                }
#pragma unroll
            for (uint32_t u = 0; u < kTvVecs; ++u) {
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
            for (uint32_t k = 0; k < kTvVecs; ++k) {
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
                if (len) crc = gf::mul(s_acc[wv][lane], pbyte[len - kTvPiece * (np - 1)]) ^ s_last[wv][lane] ^ 0xFFFFFFFFu;
                uint8_t *slot = wire + uint64_t(i) * stride;
                const u32x4 h = header_be(WTP_TYPE_DATA, seq0 + rec, len, crc);
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

int tx_emit_var_launch(const void *d_base, size_t base_bytes, const uint64_t *d_offsets, const uint32_t *d_lengths,
                       uint32_t seq0, const uint32_t *picked, const uint32_t *d_counts, uint32_t m, void *d_wire,
                       size_t wire_stride, uint32_t *d_wire_len, uint32_t *d_crc_out, hipStream_t st) {
    const uint32_t vec = (reinterpret_cast<uintptr_t>(d_wire) & 15u) == 0 && wire_stride % 16 == 0;
    const unsigned blocks = std::min((m + dev::kTvWaves - 1) / dev::kTvWaves, dev::kTvMaxBlocks);
    return launch("k_tx_emit_var", dev::k_tx_emit_var, dim3(blocks), dim3(dev::kTvBlock), st, static_cast<const uint8_t *>(d_base),
                  uint64_t(base_bytes), d_offsets, d_lengths, m, seq0, picked, d_counts, static_cast<uint8_t *>(d_wire),
                  uint64_t(wire_stride), vec, d_wire_len, d_crc_out);
}

}  // namespace wtp
