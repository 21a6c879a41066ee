// crc32_braid.hpp — the braided fixed-length kernel k_fixed_braid<ROWS, DIAG, BEpi> and its
// epilogues: CrcBEpi and CrcHoldBEpi (CRC), VerifyBEpi (receiver verify over a ring; its
// fix-up phase, verify_fixup, is in crc32_pieces.hpp) and BuildBEpi (fused DATA builder).
// A part of the one translation unit crc32_kernels.hip, included there after crc32_dev.hpp
// and crc32_pieces.hpp; not a header for other units.
#pragma once

namespace wtp {
namespace dev {

// ------------------------------------------------------------------------------------
// 1. braided fixed-length kernel
// ------------------------------------------------------------------------------------
// Packet p occupies base[p*stride, p*stride + len); base, stride and len are multiples
// of 16 and 256*(ROWS-1) < len <= 256*ROWS.  The packet is placed in a frame of ROWS
// rows x 256 B whose start is 128-B aligned when the frame still covers the packet end
// (else 64-B aligned, else right-aligned): each wave instruction then reads four
// line-aligned 256-B segments (right-aligned frames were 4% slower, kbench A/B).  Frame
// bytes before the packet are free zeros (R_0(0^k || M) = R_0(M)); the T = 16t zero
// bytes after it are undone at the flush with x^(-128 t).
__device__ __forceinline__ uint32_t braid_lead(uintptr_t st, uint32_t len, uint32_t frame) {
    const uint32_t l128 = uint32_t(st & 127u), l64 = uint32_t(st & 63u);
    return l128 + len <= frame ? l128 : (l64 + len <= frame ? l64 : frame - len);
}

// Epilogues of the braided kernel.  A flush hands lane 2P + h (h = 0) the result of
// packet slot q = P & 3 of round k = P >> 2 of its 8-round group; pre() issues, one
// group ahead, the loads put() will need (so a flush never waits on memory).
struct CrcBEpi {  // out[p] = crc
    static constexpr bool kCopy = false;  // see BuildBEpi
    static constexpr bool kFixup = false;  // see VerifyBEpi
    static constexpr int kThreads = 512;  // the launcher's workgroup size (launch_fixed_braid)
    static constexpr int kDiag = 0;       // DIAG of the production instantiation
    static constexpr int kBound = 1024;   // __launch_bounds__ (tools/kbench.hip launches up to 1024 threads)
    static constexpr int kLoadAux = 2;   // rows >= 1 stream (nt); row 0 is temporal (see k_fixed_braid)
    static constexpr bool kHold = false;  // CrcHoldBEpi: results held in LDS, stored in bursts
    static constexpr const char *kName = "CrcBEpi";  // wtp_last_kernel()
    __device__ __forceinline__ uint32_t lead(uint64_t, uint32_t st, uint32_t len, uint32_t frame) const {
        return braid_lead(st, len, frame);
    }
    uint32_t *out;
    uint32_t cinit;  // init_const(len)
    struct Pre {};
    __device__ __forceinline__ void pre(uint64_t, Pre &) const {}
    __device__ __forceinline__ bool listed(bool, const Pre &) const { return false; }
    __device__ __forceinline__ void put(uint64_t p, uint32_t v, bool on, const Pre &) const {
        if (on) out[p] = v ^ cinit;
    }
};
// The same epilogue for long batches (the launcher's rule): k_fixed_braid holds the CRCs in
// LDS and stores them in bursts (see kDump there).
struct CrcHoldBEpi : CrcBEpi {
    static constexpr bool kHold = true;
    static constexpr const char *kName = "CrcHoldBEpi";
};
// Receiver verify over a datagram ring: the kernel runs on base = ring + 16 with the
// ring's "full" payload length len (1456 for a WTP ring: 1472-B datagrams, whatever the
// slot stride, e.g. wReceiver's 1504-B slots that hold a 1500-B recvfrom buffer).
// Datagrams with recv_len == 16 + len are decided here (Receiver.cpp:203-206:
// ntohl(header.checksum) == crc32(payload)).  Every other datagram (short, empty, runt,
// 1473-1500 B, oversize) first gets ok = 0, crc = 0, is counted, and the workgroup's
// fix-up phase (verify_fixup, after its braided rounds) recomputes it with the
// reference's semantics: one launch, no state outside the caller's buffers.
struct VerifyBEpi {
    static constexpr bool kHold = false;  // see CrcBEpi
    static constexpr const char *kName = "VerifyBEpi";
    static constexpr bool kCopy = false;
    static constexpr bool kFixup = true;  // see VerifyBEpi
    static constexpr int kThreads = 512;  // verify_fixup's LDS layout assumes 8 waves
    static constexpr int kDiag = 0;
    static constexpr int kBound = 1024;
    static constexpr int kLoadAux = 2;   // rows >= 1 stream (nt); row 0 is temporal (see k_fixed_braid)
    __device__ __forceinline__ uint32_t lead(uint64_t, uint32_t st, uint32_t len, uint32_t frame) const {
        return braid_lead(st, len, frame);
    }
    const uint32_t *rl;
    const uint8_t *ring;  // 16-B aligned, stride % 16 == 0: header words are aligned
    uint64_t stride;
    uint8_t *ok;
    uint32_t *crc;  // may be null
    uint32_t *status;
    uint32_t cinit;
    uint64_t n;
    uint32_t full;  // recv_len of the datagrams this pass decides (16 + len)
    struct Pre {
        uint32_t r, h;
    };
    __device__ __forceinline__ void pre(uint64_t p, Pre &q) const {
        typedef const __attribute__((address_space(1))) uint32_t gu32;
        const uint64_t pc = p < n ? p : n - 1;
        q.r = ((gu32 *)rl)[pc];
        q.h = *(gu32 *)((gu8 *)ring + pc * stride + 12);
    }
    // true for a datagram the fix-up phase must finish
    __device__ __forceinline__ bool listed(bool on, const Pre &q) const { return on && q.r != full; }
    __device__ __forceinline__ void put(uint64_t p, uint32_t v, bool on, const Pre &q) const {
        if (!on) return;
        const uint32_t c = v ^ cinit;
        const bool mine = q.r == full;
        ok[p] = mine && bswap32(q.h) == c ? 1 : 0;
        if (crc) crc[p] = mine ? c : 0u;
    }
};

// Fused DATA packet builder (Packet.cpp:9-14,40-47,
// Sender.cpp:187-197): payload p (stride len) -> wire[p*wstride ..) = big-endian
// PacketHeader{DATA, seq0 + p, len, crc} || payload.  kCopy: every 16-B chunk the
// kernel loads is also stored into its wire slot in the same round (one buffer store
// per row, out-of-range offset for chunks outside the packet), so the payload is read
// from HBM once; the header follows at the flush.
struct BuildBEpi {
    static constexpr bool kHold = false;  // see CrcBEpi
    static constexpr const char *kName = "BuildBEpi";
    static constexpr bool kCopy = true;
    static constexpr bool kFixup = false;  // see VerifyBEpi
    // launched at 128 threads: the bound lets the copy rows keep their registers (at the
    // generic 1024 bound the compiler had 128 VGPRs and spilled 192-240 of them, 484 B of
    // scratch per lane)
    static constexpr int kThreads = 128;
    static constexpr int kDiag = WTP_BUILD_DIAG;  // ablation builds only (wrong CRCs)
    static constexpr int kBound = kThreads;
    static constexpr int kLoadAux = 2;  // rows >= 1 stream (nt), as in CrcBEpi
    uint8_t *wire;
    uint64_t wstride;  // multiple of 16
    uint32_t seq0, len;
    uint32_t *wire_len;  // may be null
    uint32_t cinit;
    struct Pre {};
    __device__ __forceinline__ void pre(uint64_t, Pre &) const {}
    // frame lead: the frame rows map to 64-B aligned wire addresses (lead = wire payload
    // address mod 64) when the frame still covers the packet
    __device__ __forceinline__ uint32_t lead(uint64_t p, uint32_t st, uint32_t l, uint32_t frame) const {
        const uint32_t w = (uint32_t(reinterpret_cast<uintptr_t>(wire)) + uint32_t(p) * uint32_t(wstride) + 16u) & 63u;
        if (w + l <= frame) return w;
        return braid_lead(st, l, frame);
    }
    // buffer resource over the 4 wire slots of round packets p0 .. p0+3
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t round_rsrc(uint64_t p0) const {
        return make_rsrc(wire + p0 * wstride, uint32_t(4 * wstride));
    }
    __device__ __forceinline__ void copy(__amdgpu_buffer_rsrc_t rs, uint32_t q, int32_t rel, bool valid, u32x4 w,
                                         bool row0) const {
        const uint32_t o = valid ? q * uint32_t(wstride) + 16u + uint32_t(rel) : 0x80000000u;
        // The frame lead follows the wire slot (lead()), so rows >= 1 store whole 64-B
        // segments of the slot and stream (nt); row 0 shares its first segment with the
        // header written at the flush and stays write-back, so L2 merges the two.
        // Interleaved A/B, 1 M x 1456 B -> 1472-B slots (profiles/r03h, r03m): all
        // write-back with the source's frame lead 635.9 us; nt rows >= 1 615.1 / 619.7 us;
        // wire-aligned lead + nt rows >= 1 597.1 us; the same with temporal loads 606.2;
        // nt row 0 too 637.3; wire-aligned, all write-back 631.5.
        if (row0)
            __builtin_amdgcn_raw_buffer_store_b128(w, rs, int(o), 0, 0);
        else
            __builtin_amdgcn_raw_buffer_store_b128(w, rs, int(o), 0, 2);
    }
    __device__ __forceinline__ bool listed(bool, const Pre &) const { return false; }
    __device__ __forceinline__ void put(uint64_t p, uint32_t v, bool on, const Pre &) const {
        if (!on) return;
        const u32x4 h = {bswap32(WTP_TYPE_DATA), bswap32(seq0 + uint32_t(p)), bswap32(len), bswap32(v ^ cinit)};
        *reinterpret_cast<u32x4 *>(wire + p * wstride) = h;
        if (wire_len) wire_len[p] = 16u + len;
    }
};

// k_fixed_braid<ROWS> — 16 lanes own one packet, a wave holds 4 packets per round.
//
// Main loop (per round, per lane): ROWS 16-B loads, one per frame row; each dword
// feeds one of the lane's 4 braids (CRC streams over every 64th dword of the frame,
// tables advancing 256 B).  B <- T(B ^ w) with the next row's word folded into the
// lookup XOR.  The 4 braids are folded in-lane, b0 ^ x^-32 (b1 ^ x^-32 (b2 ^ x^-32 b3)),
// giving one column value v_j per lane; the packet's CRC register is T applied to
// XOR_j x^(-128 j) v_j times x^(-128 t) for its t trailing zero chunks (the last row's
// advance T commutes with the x^-k, so it runs once per packet at the flush instead of
// once per braid per round: 16 of 108 lookups per round gone).
//
// Combine (Horner through LDS): each round writes its 64 column values into the wave's
// 2 KiB transposition slot at [k][q][j]; every 8 rounds the flush has lane 2P + h read
// columns 8h .. 8h+7 of packet P = 4k + q (two ds_read_b128), evaluate them by Horner's
// rule with x^-128 (7 applies), move the h = 1 half by x^-1024, apply the trailing-zero
// fix to both halves (t <= 15 masked x^-128 steps, wave-uniform count) and XOR the pair
// (DPP lane ^ 1).  This replaced a 4-level cross-lane tree in which half the lanes of
// each level idled: 6.07 -> 6.43 TB/s.
//
// Loads: all rows go through one buffer resource per round (SGPRs) whose range ends at
// the last byte of packet n-1, so lanes of packets past n and rounds past the end read
// zeros without a request; frame bytes outside a packet (first and last row only) use an
// out-of-range offset, which needs neither a clamp nor zeroing.  Row 0 holds the cache
// line a packet shares with the previous packet's last row: a normal (temporal) load
// keeps it in L2 for that row, every other row streams (nt).  All-nt re-fetched those
// lines (HBM traffic 1.069x algorithmic, 4.7% slower); all-temporal was 8.7% slower.
//
// Power: the MI355X runs this kernel at its board limit; the effective clock under the
// lookups is ~4% below the load-only skeleton's, and the kernel's cycle count is the
// skeleton's (kbench + GRBM_GUI_ACTIVE, profiles/).  Every VALU/LDS instruction in the
// loop therefore costs bandwidth: XORs are v_bitop3_b32 (3-input, new on gfx950), a
// lookup address is one v_perm_b32 into the staggered conflict-free tables, results are
// stored once per 8 rounds (on gfx950 stores share vmcnt with loads), and long batches
// (CrcHoldBEpi) hold them in LDS and store them once per 128 rounds (see kDump).
//
// DIAG (ablation builds only, tools/kbench.hip): bit0 replaces the table lookups by
// XOR/shift, bit1 skips the in-lane fold, bit2 drops the per-round wave-priority rotation;
// access-pattern ablations: bit4 drops the result stores, bit5 loads row 0
// nt as well, bit6 right-aligns every frame to its packet end (lead = frame - len), bit10
// holds the results in LDS for any CRC epilogue (CrcHoldBEpi does without it, see kDump),
// bit11 turns that off.  Production instantiations use DIAG = 0.  (Rejected round-4 forms,
// in git history at commit ba1b383: blocked-8 round order, a workgroup result ring, a
// deferred flush.)
template <int ROWS, int DIAG = 0, class BEpi = CrcBEpi>
__global__ __launch_bounds__(BEpi::kBound) void k_fixed_braid(const uint8_t *__restrict__ base, uint32_t stride,
                                                      uint32_t len, uint64_t n, BEpi epi,
                                                      const uint32_t *__restrict__ gtab) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_w[kBraidLdsWords];
    char *lds = reinterpret_cast<char *>(lds_w);
    constexpr uint32_t kGroup = 8;  // rounds per flush (2 KiB slot per wave)

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    PC_PROBE(0, __builtin_amdgcn_s_memrealtime());
    const uint32_t nwave = blockDim.x >> 6;
    const uint32_t j = lane & (kG - 1);  // braid group (column) within the packet
    const uint32_t q = lane >> 4;        // packet slot within the wave (0..3)
    const StagKeys K(lane);

    constexpr uint32_t kFrame = 256u * ROWS;
    const uint64_t rounds = (n + 3) >> 2;
    // Round order: grid-interleaved, wave (b, w) takes rounds b*nwave + w + i*rstep, so the
    // whole grid moves through the batch as one front.  (A contiguous block of rounds per
    // workgroup, and one per XCD class b % 8, were built in round 4 and measured slower at
    // every size, DESIGN 7.10, as was a translation-prefetch wave; code in git history,
    // commits f56e6d4 and 8c994a0.)
    const uint64_t rstep = uint64_t(gridDim.x) * nwave;
    const uint32_t qoff = q * stride;
    gu8 *const gbase = (gu8 *)base;

    struct Round {
        u32x4 w[ROWS];
        uint32_t lead;
    };
    // Round rr: packets 4rr .. 4rr+3.  rr is wave-uniform.
    auto load_round = [&](uint64_t rr, Round &R) {
        const bool live = rr < rounds;
        const uint64_t p0 = rr * 4;
        gu8 *sb = gbase + (live ? p0 * stride : 0);
        const uint64_t last = live ? n - 1 - p0 : 0;
        const uint32_t nrec = !live ? 0u : (last >= 3 ? 3u * stride + len : uint32_t(last) * stride + len);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc((const void *)sb, nrec);
        const uint32_t lead = (DIAG & 64) ? kFrame - len
                                          : epi.lead(p0 + q, uint32_t(reinterpret_cast<uintptr_t>((const void *)sb)) + qoff, len, kFrame);
        R.lead = lead;
        const uint32_t fo = qoff - lead + j * 16u;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            uint32_t o = fo + uint32_t(i) * 256u;
            if (i == 0 || i == ROWS - 1) {  // may hold frame bytes outside the packet
                const int32_t rel = int32_t(uint32_t(i) * 256u + j * 16u) - int32_t(lead);
                o = (rel >= 0 && rel < int32_t(len)) ? o : 0x80000000u;
            }
            if (i == 0)
                R.w[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, int(o), 0, (DIAG & 32) ? BEpi::kLoadAux : 0));
            else
                R.w[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, int(o), 0, BEpi::kLoadAux));
        }
    };

    lchar *const xs = (lchar *)(lds + kBraidXpose + wave * 2048u);
    uint32_t k = 0;            // rounds written to the slot since the last flush
    uint64_t rfirst = 0;       // round of slot row 0
    typename BEpi::Pre pre{};  // epilogue loads for the current group
    uint32_t nfix = 0;         // datagrams this wave left to the fix-up phase (verify)
    // Results (CrcHoldBEpi): a flush writes its 32 CRCs into the wave's LDS result buffer (2 KiB
    // at transposition slot 8 + wave, free at 8 waves) instead of storing them, and every
    // 16 flushes (128 rounds) the wave stores the buffer in one burst of two dwordx4 stores
    // per lane.  A 1 M batch then writes its 4 MiB of results near the end of the launch
    // instead of 32 B per wave every 8 rounds among the reads: 1 M x 1456 B alternating
    // between two buffers 232.8 -> 225.9 us, same buffer 221.9 -> 220.5 us (interleaved
    // kbench, profiles/r04r; no stores at all: 221.7 / 219.1).  Waiting for the store acks
    // was not it (deferring the flush past the next loads: neutral, profiles/r04q), nor
    // partial lines (whole-line stores per wave: neutral, profiles/r04o).
    constexpr bool kDump = ((BEpi::kHold && !(DIAG & 2048)) || (DIAG & 1024)) && !BEpi::kCopy && !BEpi::kFixup;
    // (the launcher picks CrcHoldBEpi for long batches only; the buffer needs 8 waves)
    const bool hold = kDump && nwave <= 8;
    constexpr uint32_t kHoldG = 16;  // flushes held per burst: 16 x 8 rows x 16 B fill the 2 KiB buffer
    lchar *const rbuf = (lchar *)(lds + kBraidXpose + (8u + wave) * 2048u);
    uint32_t dgroups = 0;    // flushes held in rbuf
    uint64_t dfirst = 0;     // round of the first held flush's row 0 (this wave)
    auto dump = [&]() {
        if constexpr (kDump) {
            __builtin_amdgcn_wave_barrier();
            // buffer resource from this dump's first packet: its offsets stay below
            // 16 * kHoldG * 8 * rstep (< 2^31) and the range ends at packet n for any n
            const uint64_t pb0 = 4 * dfirst, left = n > pb0 ? n - pb0 : 0;
            const __amdgpu_buffer_rsrc_t ors =
                make_rsrc(epi.out + pb0, left >= (1ull << 29) ? 0x80000000u : uint32_t(4 * left));
#pragma unroll
            for (uint32_t t = 0; t < (kHoldG * 8 + 63) / 64; ++t) {
                const uint32_t si = lane + 64u * t;  // segment: flush si >> 3, row si & 7
                const u32x4 v = *(const lu32x4 *)(rbuf + si * 16u);
                const uint64_t rr = dfirst + (8u * uint64_t(si >> 3) + (si & 7u)) * rstep;
                const uint64_t pb = 4 * rr;
                const uint32_t o = uint32_t(4 * (pb - pb0));
                const bool live = (si >> 3) < dgroups && rr < rounds;
                if (__builtin_amdgcn_ballot_w64(live && pb + 4 > n) == 0) {
                    __builtin_amdgcn_raw_buffer_store_b128(v, ors, live ? int(o) : int(0x80000000u), 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(v.x, ors, live && pb + 0 < n ? int(o) : int(0x80000000u), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(v.y, ors, live && pb + 1 < n ? int(o + 4) : int(0x80000000u), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(v.z, ors, live && pb + 2 < n ? int(o + 8) : int(0x80000000u), 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(v.w, ors, live && pb + 3 < n ? int(o + 12) : int(0x80000000u), 0, 0);
                }
            }
            __builtin_amdgcn_wave_barrier();
            dgroups = 0;
        }
    };
    auto group_packet = [&](uint64_t g0) { return (g0 + uint64_t(lane >> 3) * rstep) * 4 + ((lane >> 1) & 3u); };

    auto flush = [&](uint64_t next_g0, bool more) {
        __builtin_amdgcn_wave_barrier();
        const u32x4 lo = *(const lu32x4 *)(xs + lane * 32u), hi = *(const lu32x4 *)(xs + lane * 32u + 16u);
        uint32_t acc = hi.w;
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, hi.z);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, hi.y);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, hi.x);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, lo.w);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, lo.z);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, lo.y);
        acc = stag_apply3x<0>(lds, K.kB, K.sel, acc, lo.x);
        const uint32_t h = lane & 1u;
        {
            const uint32_t y = stag_apply3<128>(lds, K.kB, K.sel, acc);  // x^-1024
            acc = h ? y : acc;
        }
        const uint64_t rr = rfirst + uint64_t(lane >> 3) * rstep;
        const uint64_t p = rr * 4 + ((lane >> 1) & 3u);
        const uint32_t st = uint32_t(reinterpret_cast<uintptr_t>(base)) + uint32_t(p) * stride;
        const uint32_t t = (kFrame - len - ((DIAG & 64) ? kFrame - len : epi.lead(p, st, len, kFrame))) >> 4;
        const uint32_t tmax = (kFrame - len) >> 4;  // wave-uniform
        for (uint32_t s2 = 0; s2 < tmax; ++s2) {
            const uint32_t y = stag_apply3<0>(lds, K.kB, K.sel, acc);  // x^-128
            acc = s2 < t ? y : acc;
        }
        acc ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(acc), 0xB1, 0xF, 0xF, false));  // lane ^ 1
        // the advance T past the last row, deferred from the rounds (it commutes with
        // every x^-k above): once per packet instead of four times per lane per round
        if (!(DIAG & 1)) acc = stag_apply3<0>(lds, K.kA, K.sel, acc);
        const bool on = h == 0 && (lane >> 3) < k && rr < rounds && p < n;
        if constexpr (kDump) {
            if (hold) {  // the buffer sits in the transposition slots of waves 8..15
                if (dgroups == 0) dfirst = rfirst;
                // flush dgroups, row lane >> 3, packet (lane >> 1) & 3: segment 8 dgroups + row
                if (h == 0)
                    *(__attribute__((address_space(3))) uint32_t *)(rbuf + (dgroups * 8u + (lane >> 3)) * 16u +
                                                                     ((lane >> 1) & 3u) * 4u) = acc ^ epi.cinit;
                if (++dgroups == kHoldG) dump();
            } else if (!(DIAG & 16)) {
                epi.put(p, acc, on, pre);
            }
        } else if (!(DIAG & 16)) {
            epi.put(p, acc, on, pre);
        }
        if constexpr (BEpi::kFixup) nfix += uint32_t(__popcll(__ballot(epi.listed(on, pre))));
        if (more) epi.pre(group_packet(next_g0), pre);
        k = 0;
    };

    auto crc_round = [&](uint64_t rr, const Round &R) {
        if constexpr (BEpi::kCopy) {
            const auto crs = epi.round_rsrc(rr * 4);
            const bool qlive = rr * 4 + q < n;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const int32_t rel = int32_t(uint32_t(i) * 256u + j * 16u) - int32_t(R.lead);
                const bool in = (i == 0 || i == ROWS - 1) ? (rel >= 0 && rel < int32_t(len)) : true;
                epi.copy(crs, q, rel, in && qlive, R.w[i], i == 0);
            }
        }
        uint32_t b0 = R.w[0].x, b1 = R.w[0].y, b2 = R.w[0].z, b3 = R.w[0].w;  // B ^ w of the current row
#pragma unroll
        for (int i = 1; i < ROWS; ++i) {
            const u32x4 w = R.w[i];
            if (DIAG & 1) {
                b0 = (b0 ^ w.x) + (b0 >> 3);
                b1 = (b1 ^ w.y) + (b1 >> 3);
                b2 = (b2 ^ w.z) + (b2 >> 3);
                b3 = (b3 ^ w.w) + (b3 >> 3);
                continue;
            }
            b0 = stag_apply3x<0>(lds, K.kA, K.sel, b0, w.x);
            b1 = stag_apply3x<0>(lds, K.kA, K.sel, b1, w.y);
            b2 = stag_apply3x<0>(lds, K.kA, K.sel, b2, w.z);
            b3 = stag_apply3x<0>(lds, K.kA, K.sel, b3, w.w);
        }
        // braid b = 4j + k holds R_0(frame_b) * x^(32 b) / T (the last row's advance T is
        // applied at the flush): fold with x^-32 (Horner in-lane)
        uint32_t v;
        if (DIAG & 2) {
            v = xor3(b0, b1, b2) ^ b3;
        } else {
            v = stag_apply3x<128>(lds, K.kA, K.sel, b3, b2);
            v = stag_apply3x<128>(lds, K.kA, K.sel, v, b1);
            v = stag_apply3x<128>(lds, K.kA, K.sel, v, b0);
        }
        if (k == 0) rfirst = rr;
        *(__attribute__((address_space(3))) uint32_t *)(xs + k * 256u + lane * 4u) = v;
        if (++k == kGroup) flush(rr + rstep, true);
    };

    uint64_t r = uint64_t(blockIdx.x) * nwave + wave;
    // the first loads are issued before the LDS table fill so the fill overlaps them
    Round A, B;
    // braid tables, x^-32 (region A); x^-128, x^-1024 (region B): their loads go out
    // first, the first round's data loads overlap the LDS writes
    const StagSet sets[4] = {{gtab + OFF_BRAID, 0u},
                             {gtab + OFF_INV + 0 * 1024, 128u},
                             {gtab + OFF_INV + 2 * 1024, 65536u},
                             {gtab + OFF_INV + 5 * 1024, 65536u + 128u}};
    constexpr int kT = BEpi::kThreads;  // the launcher's workgroup size
    StagFill<4, kT> fill;
    const bool batched = blockDim.x == kT;  // other sizes (tools/kbench.hip) take the fill_stag loop below
    if (batched && WTP_BR_PROLOGUE_DIAG == 0) fill.load(sets);
    if constexpr (WTP_BR_PROLOGUE_DIAG == 1)
        for (int kk = 0; kk < fill.PER; ++kk) fill.v[kk] = threadIdx.x + kk;
    epi.pre(group_packet(r), pre);
    load_round(r, A);
    PC_PROBE(1, __builtin_amdgcn_s_memrealtime());
    if (WTP_BR_PROLOGUE_DIAG == 2) {
    } else if (batched) {
        fill.store(lds, sets);
    } else {
        for (int q2 = 0; q2 < 4; ++q2) fill_stag(lds, sets[q2].off >> 16, (sets[q2].off >> 7) & 1u, sets[q2].g);
    }
    PC_PROBE(2, __builtin_amdgcn_s_memrealtime());
    __syncthreads();
    PC_PROBE(3, __builtin_amdgcn_s_memrealtime());

    // 2-way unrolled: one round in flight while the previous one is hashed, no register
    // copies between the two sets.  (A variant keeping two rounds in flight, with the
    // per-wave invariants hoisted and 8 rounds unrolled, was 0.7-1.3% slower under
    // sustained load, interleaved A/B; it was 7% faster on 64K-packet batches.)
    // rotating s_setprio per round, offset by the wave's age rank (as in k_pieces): at 8
    // waves per CU +0.9% sustained (kbench x4, profiles/r01i/kbench_512_prio.log; it lost
    // 1% at 16 waves).  DIAG bit2 turns it off for ablations.
    uint32_t prio_round = wave >> 2;
    // (Three register sets, two rounds in flight, were tried for the fused builder's 2 waves
    // per CU and rejected: profiles/r01g/kbench_depth3_rejected_*.log.)
    while (r < rounds) {
        if (!(DIAG & 4)) rotate_prio(++prio_round);
        load_round(r + rstep, B);
        crc_round(r, A);
        if (WTP_PROBE && prio_round == (wave >> 2) + 1) PC_PROBE(4, __builtin_amdgcn_s_memrealtime());
        r += rstep;
        if (r >= rounds) break;
        load_round(r + rstep, A);
        crc_round(r, B);
        r += rstep;
    }
    if (k) flush(0, false);
    if constexpr (kDump) {
        if (dgroups) dump();
    }
    PC_PROBE(5, __builtin_amdgcn_s_memrealtime());
    if constexpr (BEpi::kFixup) verify_fixup(lds, epi, gtab, nfix, rstep, wave, lane);
}

}  // namespace dev
}  // namespace wtp
