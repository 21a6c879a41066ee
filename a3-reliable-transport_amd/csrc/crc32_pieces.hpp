// crc32_pieces.hpp — the piece kernel k_pieces<Prov, Epi> (general shapes) and the braided
// verify's fix-up phase, which runs the same piece loop.  A part of the one translation
// unit crc32_kernels.hip, included there after crc32_dev.hpp; not a header for other units.
//   MetaRaw, RangeDesc, CrcEpi, VerifyEpi; the LDS layout; WaveSplit (wave ranges by piece
//   count); SpanDma (span staging); pieces_loop; PcTables; k_pieces; LdsIdxDgramProv and
//   verify_fixup.  The providers of the C-ABI entry points are in crc32_launch.hpp.
#pragma once

namespace wtp {
namespace dev {

// ------------------------------------------------------------------------------------
// 2. pieces kernel (general shapes)
// ------------------------------------------------------------------------------------
// Raw metadata words of one packet as loaded by a provider (crc32_launch.hpp, and
// LdsIdxDgramProv below).
struct MetaRaw {
    uint64_t a;
    uint32_t b, c, d;
};
// One sub-launch of a packed batch >= 2 GiB (launch_packed_ranges): packets [begin, end)
// of the caller's arrays, read through a < 2 GiB view that starts `rebase` bytes into the
// 16-B aligned buffer.  Written on the device by k_cut_ranges.  `bad` holds two flags:
// kCutBad, set by k_cut_ranges (an offset past the buffer; fixed before any piece
// sub-launch starts, so every wave of a sub-launch reads the same value), and kRunBad, set
// by the piece kernel when a packet lies outside the view (the offsets were not packed).
// Either one makes the gated k_stream launch recompute the whole batch.
constexpr uint32_t kRunBad = 1u, kCutBad = 2u;
struct RangeDesc {
    uint64_t begin, end, rebase;
    uint32_t nbytes, bad;
};
static_assert(sizeof(RangeDesc) == 32, "RangeDesc");
// providers whose packet range and view are bound on the device (bind(), at kernel entry)
template <class P>
constexpr bool kDevRange = requires { requires P::kDevRange; };  // declared and true

// Epilogues store through buffer resources: lanes without a result use an out-of-range
// offset, so the store is one unconditional instruction (no exec branch, so the
// compiler's vmcnt accounting keeps the round's prefetches in flight).  n < 2^29 (the
// host splits larger batches).
struct CrcEpi {
    static constexpr const char *kName = "CrcEpi";  // wtp_last_kernel()
    uint32_t *out;
    uint32_t n;
    __device__ __forceinline__ void rebase(uint64_t first, uint32_t cnt) {  // a device-bound sub-range
        out += first;
        n = cnt;
    }
    __device__ __forceinline__ void put(uint64_t p, uint32_t crc, bool, uint32_t, bool on) const {
        __builtin_amdgcn_raw_buffer_store_b32(crc, make_rsrc(out, 4 * n), on ? int(4 * p) : int(0x80000000u), 0, 0);
    }
};
// Receiver.cpp:203-206: (int)ntohl(hdr.checksum) == (int)crc32(payload).  aux carries the
// header checksum (host order) from the provider.
struct VerifyEpi {
    static constexpr const char *kName = "VerifyEpi";
    uint8_t *ok;
    uint32_t *crc;  // may be null
    uint32_t n;
    __device__ __forceinline__ void put(uint64_t p, uint32_t c, bool valid, uint32_t want, bool on) const {
        const bool good = valid && want == c;
        __builtin_amdgcn_raw_buffer_store_b8(uint8_t(good ? 1 : 0), make_rsrc(ok, n), on ? int(p) : int(0x80000000u),
                                             0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(valid ? c : 0u, make_rsrc(crc, crc ? 4 * n : 0u),
                                              on ? int(4 * p) : int(0x80000000u), 0, 0);
    }
};

// LDS of k_pieces: region 0 holds two staggered table sets (set 0 = slice-by-4, set 1 =
// the x^(8*64) scan operator), then the scan operators x^(8*64*d), d = 2..32, as plain
// 4 KiB tables, the 65-word head-init table, and one staging slot per wave.  A slot
// holds a span of 16-B chunks with 16 B of padding after every 256 B (chunk c at
// 16*(c + c/16)): the windows of consecutive pieces are 64 B apart, and the padding
// spreads their 16-B reads over all bank groups instead of four.
constexpr uint32_t kPcThreads = 1024, kPcLogT = __builtin_ctz(kPcThreads), kPcWaves = kPcThreads / 64;
constexpr uint32_t kPcWords = uint32_t(kPieceS) / 4;                // window words per lane
constexpr uint32_t kPcNOps = 5;                                      // plain scan operators in LDS
constexpr uint32_t kPcOps = 65536;
constexpr uint32_t kPcHinit = kPcOps + kPcNOps * kOpBytes;
constexpr uint32_t kPcStage = kPcHinit + 4 * kHinitWords;
constexpr uint32_t kPcChunks = 4 * uint32_t(kPieceS) + 16;  // span chunks a slot holds: 64 pieces + gaps + head slack
constexpr uint32_t kPcSlot = 16 * (kPcChunks + kPcChunks / 16 + 1);  // windows read one chunk past
constexpr uint32_t kPcFlags = kPcStage + kPcWaves * kPcSlot;  // 64 B per wave: packet-start flags
constexpr uint32_t kPcBal = kPcFlags + kPcWaves * 64;         // wave split: 16 piece sums, 17 u64 starts
constexpr uint32_t kPcSpre = kPcBal + 64 + 17 * 8;       // 17 u32: pieces before each wave's range
// 16 u32: pieces each wave has left, by SIMD (read as one 16-B vector per SIMD, so the
// base is 16-B aligned: pieces_loop takes the LDS base as a pointer, the compiler assumes
// natural alignment, and a misaligned ds_read_b128 here cost C5 3.3 us per launch)
constexpr uint32_t kPcRem = (kPcSpre + 17 * 4 + 15) & ~15u;
constexpr uint32_t kPcLdsWords = (kPcRem + 64) / 4;      // 161,904 B
static_assert(kPcRem % 16 == 0 && kPcStage % 16 == 0 && kPcSlot % 16 == 0 && kPcOps % 16 == 0, "LDS vector alignment");
static_assert(16 * (kPcChunks + kPcChunks / 16 + 1) <= kPcSlot, "staging slot");
static_assert(kPcLdsWords * 4 <= 163840, "LDS");

__device__ __forceinline__ uint32_t stage_addr(uint32_t chunk) { return 16u * (chunk + (chunk >> 4)); }

// Inclusive prefix sum over the wave with DPP (no LDS round trips): Hillis-Steele within
// each 16-lane row (row_shr 1, 2, 4, 8), then row_bcast:15 / row_bcast:31 carry the row
// totals into the rows above.
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false));
    return v;
}

// Pieces of a packet of payload length len as the main loop counts them (an empty or
// over-long packet is one).  Providers with variable lengths expose len_array() (the
// array of the one metadata word per packet the length comes from) and len_of(word).
__device__ __forceinline__ uint32_t pieces_of_len(uint32_t len) {
    return (len == 0 || len > kMaxVarLen) ? 1u : (len + kPieceS - 1) / kPieceS;
}

// Wave ranges of a workgroup's packets [g0, g1) with equal piece counts (rounds), not
// equal packet counts: with Zipf lengths, equal counts left the busiest wave 1.43x the
// mean number of rounds (C5, s = 1.1) and the launch waited for it.  Each thread owns a
// contiguous sub-range; load() issues the length loads of its first kReg packets (they
// fly while the LDS tables fill), finish() sums their pieces, a block scan places the sub-ranges,
// and the thread whose sub-range holds wave w's target (total * w / waves) walks it, from
// registers, to the first packet at or past the target.  Every thread of the block must
// call finish() (two barriers).  k_pieces runs 1024-thread blocks: the divisions by the
// thread and wave counts are shifts (64-bit divisions by a runtime value cost ~100 VALU
// each, and the target loop had 15 of them).
static_assert(kPcThreads >= 128 && kPcThreads <= 1024 && (kPcThreads & (kPcThreads - 1)) == 0, "k_pieces block");
// Pieces of packets [p, min(p + 16, b)) from four 16-B length loads issued together (4-B
// aligned offsets; words at or past g1 read 0 and are not counted).  Packets are taken
// while the running count is below `want` (~0u: all; the boundary walk passes the pieces
// left to its target), and *taken (if given) receives how many were.
template <class Prov>
__device__ __forceinline__ uint32_t chunk_pieces(const Prov &prov, uint64_t g1, uint64_t p, uint64_t b, uint32_t want,
                                                 uint32_t *taken) {
    const __amdgpu_buffer_rsrc_t lr = make_rsrc(prov.len_array(), uint32_t(4 * g1));
    u32x4 q[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) q[j] = buf_ld16(lr, uint32_t(4 * (p + 4 * j)));
    const uint32_t w[16] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w,
                            q[2].x, q[2].y, q[2].z, q[2].w, q[3].x, q[3].y, q[3].z, q[3].w};
    uint32_t sum = 0, n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const bool step = p + i < b && sum < want;
        sum += step ? pieces_of_len(prov.len_of(w[i])) : 0u;
        n += step ? 1u : 0u;
    }
    if (taken) *taken = n;
    return sum;
}
struct WaveSplit {
    static constexpr uint32_t kReg = 8, kThreads = kPcThreads, kWaves = kThreads / 64;
    uint32_t raw[kReg];  // length words of the first kReg packets of the sub-range
    uint64_t a, b;
    template <class Prov>
    __device__ __forceinline__ void load(const Prov &prov, uint64_t g0, uint64_t g1) {
        const uint64_t R = g1 - g0;
        a = g0 + ((R * threadIdx.x) >> kPcLogT);
        b = g0 + ((R * (threadIdx.x + 1)) >> kPcLogT);
        // the sub-range's first 8 length words as two 16-B buffer loads (4-B aligned is
        // enough; words at or past g1 read 0 and are never used): a quarter of the vector
        // memory instructions of 8 dword loads, in the prologue where they queue behind
        // the table loads
        static_assert(kReg == 8, "two 16-B loads");
        const __amdgpu_buffer_rsrc_t lr = make_rsrc(prov.len_array(), uint32_t(4 * g1));
        const u32x4 l0 = buf_ld16(lr, uint32_t(4 * a)), l1 = buf_ld16(lr, uint32_t(4 * a + 16));
        raw[0] = l0.x; raw[1] = l0.y; raw[2] = l0.z; raw[3] = l0.w;
        raw[4] = l1.x; raw[5] = l1.y; raw[6] = l1.z; raw[7] = l1.w;
    }
    template <class Prov>
    __device__ __forceinline__ void finish(const Prov &prov, uint64_t g0, uint64_t g1, char *lds, uint32_t wave,
                                           uint32_t lane, uint64_t &lo, uint64_t &hi, uint32_t &wpieces) {
        constexpr uint32_t nw = kWaves;
        const uint64_t m = b - a;
        uint32_t k[kReg], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kReg; ++j) {
            k[j] = j < m ? pieces_of_len(prov.len_of(raw[j])) : 0u;
            sum += k[j];
        }
        // > kReg packets per thread (launches of more than 2 M packets): the rest in chunks
        // of 16 length words, four 16-B loads in flight per chunk.  (A dword loop waited on
        // each load: at 15 M packets per launch, ~50 serial loads here and up to ~57 in the
        // boundary walk below cost ~0.1 ms per launch.)  Counts only balance the waves: the
        // ranges stay a partition of [g0, g1) whatever they hold.
        for (uint64_t p = a + kReg; p < b; p += 16) sum += chunk_pieces(prov, g1, p, b, ~0u, nullptr);
        const uint32_t incl = wave_incl_add(sum);
        uint32_t *const wsum = reinterpret_cast<uint32_t *>(lds + kPcBal);
        uint64_t *const starts = reinterpret_cast<uint64_t *>(lds + kPcBal + 64);
        uint32_t *const spre = reinterpret_cast<uint32_t *>(lds + kPcSpre);
        if (lane == 63u) wsum[wave] = incl;
        if (threadIdx.x == 0) {
            starts[0] = g0;
            starts[nw] = g1;
            spre[0] = 0;
        }
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t v = wsum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        const uint32_t excl = before + incl - sum;
        for (uint32_t w = 1; w < nw; ++w) {
            const uint32_t target = uint32_t((uint64_t(total) * w) >> (kPcLogT - 6));
            if (target >= excl && target - excl < sum) {
                uint32_t pre = excl;
                uint64_t p = a;
#pragma unroll
                for (uint32_t j = 0; j < kReg; ++j) {
                    const bool step = j < m && pre < target;
                    pre += step ? k[j] : 0u;
                    p += step ? 1u : 0u;
                }
                while (p < b && pre < target) {
                    uint32_t taken = 0;
                    pre += chunk_pieces(prov, g1, p, b, target - pre, &taken);
                    p += taken;
                }
                starts[w] = p;
                spre[w] = pre;
            }
        }
        if (threadIdx.x == 0) spre[nw] = total;
        __syncthreads();
        // Every starts[w] was written above: pieces_of_len() >= 1, so total >= g1 - g0 > 0
        // and each target < total lies in exactly one thread's [excl, excl + sum).  The
        // clamp keeps a wave inside [g0, g1] even if that invariant were ever broken: a
        // round-3 development build counted 0 pieces for small packets, so an all-small
        // workgroup wrote no starts[1..15] and its waves ran over the previous kernel's
        // stale LDS indices (hipErrorIllegalAddress).
        const uint64_t s0 = uniform64(starts[wave]), s1 = uniform64(starts[wave + 1]);
        lo = s0 < g0 ? g0 : (s0 > g1 ? g1 : s0);
        hi = s1 < lo ? lo : (s1 > g1 ? g1 : s1);
        wpieces = uint32_t(__builtin_amdgcn_readfirstlane(int(spre[wave + 1] - spre[wave])));
    }
};

// Span staging by LDS-DMA: the span of kPcChunks 16-B chunks from a view offset, written
// into the slot (chunk c at stage_addr(c)) by `buffer_load_dwordx4 ... lds` straight from
// memory.  An LDS-DMA instruction writes 64 consecutive 16-B positions (wave-uniform base
// in M0 + 16 * lane), so the per-256-B padding is made on the SOURCE side: position q of
// the slot holds chunk q - q/17 (the inverse of stage_addr; every 17th position is padding
// and receives a duplicate chunk that no window reads).  Positions 0..kPcSlotPos-1: four
// full instructions and 34 lanes of a fifth.  Issued as inline asm, so the compiler keeps
// no count of them: the loop waits for them itself (vmcnt(0) before the slot is read) and
// lets the window reads finish (lgkmcnt(0)) before the next span may overwrite the slot.
constexpr uint32_t kPcSlotPos = kPcSlot / 16;                 // 290 positions of 16 B
constexpr uint32_t kPcDmaRegs = (kPcSlotPos + 63) / 64;       // 5 instructions
static_assert(kPcSlotPos - 64 * (kPcDmaRegs - 1) <= 64, "slot positions");
struct SpanDma {
    uint32_t coff[kPcDmaRegs];  // per lane: 16 * (source chunk of slot position 64 i + lane)
    uint32_t slot;              // LDS byte address of the wave's slot (wave-uniform)
    __device__ __forceinline__ SpanDma(uint32_t slot_addr, uint32_t lane) : slot(slot_addr) {
#pragma unroll
        for (uint32_t i = 0; i < kPcDmaRegs; ++i) {
            const uint32_t q = 64u * i + lane;
            coff[i] = 16u * (q - q / 17u);
        }
    }
    // the span of 16-B chunks from view offset b16 (16-aligned, may be "negative" or past
    // the view: those offsets read 0 without touching memory) into the slot
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rs, int32_t b16, uint32_t lane) const {
        // lgkmcnt(0) first: this wave's window reads of the slot have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (uint32_t i = 0; i < kPcDmaRegs; ++i) {
            const uint32_t voff = uint32_t(b16) + coff[i];
            const uint32_t m0v = slot + 1024u * i;
            uint32_t keep;
            if (i + 1 < kPcDmaRegs || lane < kPcSlotPos - 64u * (kPcDmaRegs - 1))
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
                             "s_mov_b32 m0, %0"
                             : "=&s"(keep)
                             : "v"(voff), "s"(rs), "s"(m0v)
                             : "memory");
        }
    }
    // The same, leaving out the chunks that start at or past view byte `lim` (their lanes
    // get an out-of-range offset: no request).  The tail clamp (WTP_PC_TAILCLAMP) below.
    __device__ __forceinline__ void issue_below(__amdgpu_buffer_rsrc_t rs, int32_t b16, uint32_t lane, int32_t lim) const {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (uint32_t i = 0; i < kPcDmaRegs; ++i) {
            const int32_t c0 = b16 + int32_t(coff[i]);
            const uint32_t voff = c0 < lim ? uint32_t(c0) : 0x80000000u;
            const uint32_t m0v = slot + 1024u * i;
            uint32_t keep;
            if (i + 1 < kPcDmaRegs || lane < kPcSlotPos - 64u * (kPcDmaRegs - 1))
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
                             "s_mov_b32 m0, %0"
                             : "=&s"(keep)
                             : "v"(voff), "s"(rs), "s"(m0v)
                             : "memory");
        }
    }
    __device__ __forceinline__ static void wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// Maximum over the wave (unsigned; 0 is neutral), by the same DPP steps as wave_incl_add
// (a __shfl_xor ladder here changed how the compiler lowered the loop's other
// shuffles and cost C5 ~2 us per launch).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, false)));
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, false)));
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, false)));
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, false)));
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false)));
    v = mx(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false)));
    return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

// Tail clamp of the span prefetch: a wave's last rounds used to prefetch a full 4352-B
// span past the end of its last packet, i.e. into the first bytes of the next wave's
// range, which that wave had read ~40 us earlier (its first round), so they came from
// memory twice: ~3.4 KB per wave boundary, 14.1 MB of C5's 26 MB excess read
// (tools/c5_span_model.py, profiles/r05).  When the round's view holds every packet the
// wave has left, the prefetch stops at the end of the last of them.  WTP_PC_TAILCLAMP
// (top of crc32_kernels.hip) turns it on: measured and not shipped.

// The wave's packets form one stream of 64-B pieces (each packet cut into pieces counted
// back from its end, the head piece possibly shorter).  A round takes the next pieces,
// one per lane, up to 64 and up to the first piece whose window falls outside the span
// one LDS slot holds (kPcChunks chunks from the round's first window): packed and
// strided batches always fill all 64 lanes, scattered offsets make shorter rounds.  A
// packet may straddle rounds: its CRC register after its last piece in round r seeds the
// chain of its next piece in round r+1.  Per round a wave
//   1. scans the piece counts of the next 64 packets (metadata prefetched during the
//      previous round) and assigns lane -> (packet, piece);
//   2. stages the span into its LDS slot: it was loaded during the previous round (it
//      starts at most 64 B before that round's last window ends: speculative, exact for
//      packed and strided batches); a miss loads it now.  The span goes from memory
//      straight into the slot by LDS-DMA (SpanDma, 5 instructions of 1 KiB; round 3
//      loaded it into 20 VGPRs and stored it with 5 ds_write_b128: C5 47.9 -> 46.1 us);
//   3. reads each lane's 64-B window from the slot and issues the next round's metadata
//      and span loads;
//   4. runs the slice-by-4 chain over the window (bytes before the packet masked to
//      zero; the head piece adds shift(~0, head length), the CRC's initial value), then a
//      segmented scan with x^(8*64*d) combines each packet's pieces and the lane holding
//      a packet's last piece emits crc = W ^ ~0.
// Loads and stores are branch-free (out-of-range buffer offsets for idle lanes), so the
// prefetches stay in flight across the round.
// Metadata of packets q0 .. q0+63 for one round: lane i loads packet q0 + i (clamped to
// hi - 1: branch-free).  The caller of pieces_loop issues the first round's (raw) before
// its last prologue waits, so that latency overlaps them.
template <class Prov>
__device__ __forceinline__ void pieces_meta(const Prov &prov, uint64_t q0, uint64_t hi, uint32_t lane, MetaRaw &raw,
                                            __amdgpu_buffer_rsrc_t rs) {
    if constexpr (Prov::kGroupLoad) {
        prov.load_group(q0, lane, raw);  // buffer loads: lanes past the arrays read 0
    } else {
        const uint64_t pi = q0 + lane;
        prov.load(pi < hi ? pi : hi - 1, raw, rs);
    }
}

// The piece-stream main loop: packets [lo, hi) of the provider (wpieces = their piece
// total, for the work-left priority of variable-length providers), tables already in LDS
// (PcTables), raw = the first round's metadata (pieces_meta(lo)).  Used by k_pieces and
// by the braided verify's fix-up phase.
template <class Prov, class Epi>
__device__ __forceinline__ void pieces_loop(char *lds, __amdgpu_buffer_rsrc_t rs, const Prov &prov, const Epi &epi,
                                            uint64_t lo, uint64_t hi, uint32_t wpieces, uint32_t *status,
                                            uint32_t wave, uint32_t lane, MetaRaw raw) {
    const StagKeys K(lane);
    lchar *const slot = (lchar *)lds + kPcStage + wave * kPcSlot;
    constexpr int32_t kSpanBytes = int32_t(16 * kPcChunks);
    constexpr int32_t kNoSpan = 0x7FFFF000;  // out of range: loads return 0, no traffic

    auto meta = [&](uint64_t q0) { pieces_meta(prov, q0, hi, lane, raw, rs); };
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the loop entry then matches its back edge

    PC_PROBE(3, __builtin_amdgcn_s_memrealtime());
    uint32_t skip = 0, carry = 0;  // pieces of packet p0 done in earlier rounds, their register
    int32_t spec = kNoSpan;        // view offset of the prefetched span
    const SpanDma dma(__builtin_amdgcn_readfirstlane(uint32_t(uintptr_t(slot))), lane);
    uint32_t nrounds = 0, done = 0;
    hi = uniform64(hi);  // wave-uniform in SGPRs: the round's packet arithmetic stays scalar
    for (uint64_t p0 = uniform64(lo); p0 < hi;) {
        uint64_t off;
        uint32_t len, aux = 0, oslot = 0;
        bool valid;
        prov.decode(raw, off, len, valid, aux, oslot);
        const uint32_t inview = hi - p0 > 64u ? 64u : uint32_t(hi - p0);  // wave-uniform (SALU)
        const bool have = lane < inview;
        if constexpr (kDevRange<Prov>) {
            if (have && !valid) prov.flag_outside();  // not packed: the gated k_stream redoes the batch
        }
        if (have && len > kMaxVarLen) {
            atomicOr(status, 1u);
            len = 0;
            valid = false;
        }
        const uint32_t k = have ? (len == 0 ? 1u : (len + kPieceS - 1) / kPieceS) : 64u;
        const uint32_t kr = k - (lane == 0 ? skip : 0u);  // pieces still to do
        const uint32_t incl = wave_incl_add(kr);
        const uint32_t excl = incl - kr;
        const uint32_t navail = __popcll(__ballot(have));  // packets of the wave left in view
        const uint32_t covered = uint32_t(__builtin_amdgcn_readlane(int(incl), int(navail - 1)));  // pieces in view

        // --- lane -> (packet, piece): flag the first lane of every packet in LDS, then
        // pk = (# flagged lanes <= this lane) - 1 from a ballot ----------------------------
        lu8 *const flags = (lu8 *)lds + kPcFlags + wave * 64u;
        flags[lane] = 0;
        if (have && excl < 64u) flags[excl] = 1;
        __builtin_amdgcn_wave_barrier();
        const bool start = flags[lane] != 0;
        __builtin_amdgcn_wave_barrier();
        const uint64_t starts = __ballot(start);
        uint32_t pk = __builtin_amdgcn_mbcnt_hi(uint32_t(starts >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(starts), 0u)) +
                      (start ? 1u : 0u) - 1u;
        const bool mapped = lane < covered;
        pk = mapped ? pk : 0;
        const uint32_t pex = __shfl(excl, pk);
        const uint32_t pkk = __shfl(k, pk);
        const uint32_t plen = __shfl(len, pk);
        const uint32_t poff = __shfl(uint32_t(off), pk);  // < 2^31: the view is < 2 GiB
        const bool pvalid = __shfl(valid ? 1u : 0u, pk) != 0;
        const uint32_t paux = __shfl(aux, pk);
        const uint64_t pout = Prov::kIndexed ? uint64_t(uint32_t(__shfl(oslot, pk))) : p0 + pk;  // output index
        const uint32_t lp = lane - pex;                  // piece index within this round
        const uint32_t gp = lp + (pk == 0 ? skip : 0u);  // piece index within the packet

        // --- piece window: the 64 bytes ending at this piece's end ----------------------
        const int32_t we = int32_t(poff + plen) - int32_t(pkk - 1 - gp) * kPieceS;
        const int32_t ws = we - kPieceS;
        // the round: lanes up to the first one whose window leaves [lo16, lo16 + span)
        const int32_t lo16 = __builtin_amdgcn_readlane(ws, 0) & ~15;
        const bool out = !mapped || ws < lo16 || we - lo16 > kSpanBytes;
        const uint64_t outm = __ballot(out);
        const uint32_t total = outm ? uint32_t(__builtin_ctzll(outm)) : 64u;  // >= 1: lane 0 fits
        const bool active = lane < total;
        const int32_t vf0 = int32_t(poff) - ws;  // bytes of the window before the packet
        const int32_t vf = active ? (vf0 > kPieceS ? kPieceS : vf0) : kPieceS;

        // --- stage the span ---------------------------------------------------------------
        const bool hit = __ballot(active && (ws < spec || we - spec > kSpanBytes)) == 0;
        int32_t sbase = spec;
        if (!hit) {
            dma.issue(rs, lo16, lane);  // the miss pays its latency here
            sbase = lo16;
        }
        SpanDma::wait();  // the slot holds the span (prefetched, or just loaded)
        __builtin_amdgcn_wave_barrier();
        // the window's five 16-B blocks, aligned (dword-aligned variants without the
        // rotation below were slower on C5: ds_read2_b32 pairs at the 64-B lane stride
        // conflict 4-way, +13%; unaligned ds_read_b128 from inline asm, which gfx950
        // executes correctly, +39%)
        uint32_t d[kPcWords + 4];
        {
            const uint32_t blk = active ? uint32_t(ws - sbase) >> 4 : 0u;
#pragma unroll
            for (uint32_t u = 0; u < kPcWords / 4 + 1; ++u) {
                const u32x4 y = *(const lu32x4 *)(slot + stage_addr(blk + u));
                d[4 * u + 0] = y.x;
                d[4 * u + 1] = y.y;
                d[4 * u + 2] = y.z;
                d[4 * u + 3] = y.w;
            }
        }
        __builtin_amdgcn_wave_barrier();

        // --- round bookkeeping and the next round's prefetch ------------------------------
        const uint32_t tl = total - 1;
        const uint32_t last_pk = __builtin_amdgcn_readlane(pk, tl);
        const uint32_t last_gp = __builtin_amdgcn_readlane(gp, tl);
        const uint32_t last_k = __builtin_amdgcn_readlane(pkk, tl);
        const int32_t last_we = __builtin_amdgcn_readlane(we, tl);
        const bool partial = last_gp + 1 < last_k;
        const uint64_t p0n = p0 + last_pk + (partial ? 0u : 1u);
        meta(p0n);  // first: the next round waits for these, not for the span
        spec = p0n < hi ? ((last_we - kPieceS) & ~15) : kNoSpan;
        // the tail clamp (WTP_PC_TAILCLAMP builds only; not in the verify fix-up's indexed pass: scattered datagrams, and its kernel has
        // no SGPRs to spare for it)
        if (WTP_PC_TAILCLAMP && !Prov::kIndexed && spec != kNoSpan && hi - p0 <= 64u) {  // wave-uniform: the wave's last packets are all in view
            // end of the bytes any packet still to do can need (lanes from the round's last
            // packet on: a superset of p0n .. hi-1)
            const uint32_t pend = have && lane >= last_pk ? uint32_t(off) + len : 0u;
            dma.issue_below(rs, spec, lane, int32_t(wave_max_u32(pend)));
        } else if (spec != kNoSpan) {
            dma.issue(rs, spec, lane);  // wave-uniform branch
        }

        // rotate left by a>>2 dwords with bit-selects (v_bfi_b32), then funnel by a&3
        const uint32_t a = uint32_t(ws) & 15u;
        const uint32_t m2 = 0u - ((a >> 3) & 1u), m1 = 0u - ((a >> 2) & 1u), sb = a & 3u;
        uint32_t e[kPcWords + 2];
#pragma unroll
        for (int i = 0; i < int(kPcWords) + 2; ++i) e[i] = d[i] ^ ((d[i] ^ d[i + 2]) & m2);
#pragma unroll
        for (int i = 0; i < int(kPcWords) + 1; ++i) e[i] = e[i] ^ ((e[i] ^ e[i + 1]) & m1);

        // one slice-by-4 chain over the window's 16 words.  (Two interleaved chains per
        // window were 2% slower on C5, profiles/r06e: the loop is bound by VALU issue, not
        // by its LDS chain latency.)
        // The chain register is a one-element array indexed through the loop variable, as it
        // was when the loop could run two chains: a plain scalar compiles to the same
        // instructions with the operands of 16 v_xor_b32 swapped, and retiring the build
        // switches kept every kernel byte-identical (profiles/kernelsplit).  The next change
        // to this kernel's code may make it a scalar.
        uint32_t cc[1];
        cc[0] = (lane == 0u) ? carry : 0u;  // carry is 0 unless packet p0 continues
        const int32_t vf8 = 8 * vf;
#pragma unroll
        for (int i = 0; i < int(kPcWords); ++i) {
            uint32_t &cj = cc[i % 1];
            const uint32_t wd = __builtin_amdgcn_alignbyte(e[i + 1], e[i], sb);
            // keep the bytes at window offset >= vf: the low s = clamp(8 vf - 32 i, 0, 32)
            // bits of word i go.  One v_med3 + one v_lshlrev_b64 (the shift unit reads 6
            // bits: word 2j takes the low half of 0xFFFFFFFF << s, word 2j+1 the high half
            // of 0xFFFFFFFF << (s + 32), and s = 32 wraps to a zero high half)
            const int32_t t = vf8 < 32 * i ? 32 * i : (vf8 > 32 * i + 32 ? 32 * i + 32 : vf8);
            const uint64_t k64 = uint64_t(0xFFFFFFFFu) << (uint32_t(t) & 63u);
            const uint32_t keep = (i & 1) ? uint32_t(k64 >> 32) : uint32_t(k64);
            cj = stag_apply3<0>(lds, K.kA, K.sel, __builtin_amdgcn_bitop3_b32(cj, wd, keep, 0x78));  // cj ^ (wd & keep)
        }
        uint32_t c = cc[0];
        // head piece: R_~0(head) = R_0(0^vf || head) ^ shift(~0, S - vf)
        const uint32_t hw = lds_rd(lds, kPcHinit + 4u * uint32_t(kPieceS - (vf < 0 ? 0 : vf)));
        c ^= gp == 0u ? hw : 0u;

        // --- segmented inclusive scan: W_i <- W_{i-d} * x^(8*64*d) ^ W_i ---------------
        uint32_t W = c;
        {
            const uint32_t u = __shfl_up(W, 1);  // x^(8*64) is the staggered set 1
            if (lp >= 1u && lane >= 1u) W = stag_apply3x<128>(lds, K.kA, K.sel, u, W);
        }
        // levels no lane needs (every packet of the round has < dd pieces in it) are
        // skipped with a wave-uniform branch on the ballot (SGPRs): small-packet rounds
        // stop early
#pragma unroll
        for (uint32_t dd = 2, o = 0; dd < 64; dd <<= 1, ++o) {
            const bool need = lp >= dd && lane >= dd;
            if (__builtin_amdgcn_ballot_w64(need) == 0) break;
            const uint32_t u = __shfl_up(W, dd);
            if (need) W = op_apply_fold(lds, kPcOps + o * kOpBytes, u, W);  // exec-masked: idle lanes issue no lookups
        }
        epi.put(pout, W ^ 0xFFFFFFFFu, pvalid, paux, active && gp == pkk - 1);
        carry = partial ? __builtin_amdgcn_readlane(W, tl) : 0u;
        skip = partial ? last_gp + 1 : 0u;
        p0 = uniform64(p0n);  // keeps the loop-carried packet index in SGPRs
        if (WTP_PROBE && nrounds == 0) PC_PROBE(4, __builtin_amdgcn_s_memrealtime());
        ++nrounds;
        if constexpr (Prov::kVarLen) {
            // The SIMD arbiter serves the oldest of equal-priority waves first, so with a
            // fixed rotation the youngest waves still ended ~8 us after the oldest
            // (tools/pprobe.py).  Priority = how many of the SIMD's four waves have less
            // work left than this one (stale reads only blur the ranking).
            done += total;
            const uint32_t left = wpieces > done ? wpieces - done : 0u;
            const uint32_t simd = wave & 3u;
            typedef __attribute__((address_space(3))) uint32_t lu32w;
            if (lane == 0) *(lu32w *)((lchar *)lds + kPcRem + 4u * (4u * simd + (wave >> 2))) = left;
            // lanes 0..3 read the SIMD's four entries; the rank is one ballot's popcount
            const uint32_t other = *(const lu32w *)((lchar *)lds + kPcRem + 16u * simd + 4u * (lane & 3u));
            rotate_prio(uint32_t(__popcll(__builtin_amdgcn_ballot_w64(lane < kPcWaves / 4u && other < left))));
        } else {
            rotate_prio(nrounds + (wave >> 2));
        }
    }
    PC_PROBE(5, __builtin_amdgcn_s_memrealtime());
    PC_PROBE(6, nrounds);
    PC_PROBE(7, hi - lo);
}

// LDS tables of the piece loop: the two staggered sets (slice-by-4, x^(8*64)), the plain
// scan operators x^(8*64*d), d = 2..32, and the head-init table.  load() issues every
// global load (ahead of the caller's other prologue loads: vmcnt completes in order),
// store() writes LDS; a barrier must follow before pieces_loop.
template <int THREADS>
struct PcTables {
    static constexpr uint32_t kOpQ = kPcNOps * 256, kOpPer = (kOpQ + THREADS - 1) / THREADS;
    StagFill<2, THREADS> fill;
    u32x4 q[kOpPer];
    uint32_t hv;
    __device__ __forceinline__ static void sets(const uint32_t *gtab, StagSet (&s)[2]) {
        s[0] = {gtab + OFF_S4, 0u};
        s[1] = {gtab + OFF_FWD, 128u};  // x^(8*64)
    }
    __device__ __forceinline__ void load(const uint32_t *gtab) {
        StagSet ss[2];
        sets(gtab, ss);
        fill.load(ss);
        const u32x4 *src = reinterpret_cast<const u32x4 *>(gtab + OFF_FWD + 1024 * (6 - kPcNOps));  // the last 5 of 6
#pragma unroll
        for (uint32_t k = 0; k < kOpPer; ++k) {
            const uint32_t i = threadIdx.x + k * THREADS;
            q[k] = src[i < kOpQ ? i : 0];
        }
        hv = gtab[OFF_HINIT + (threadIdx.x <= kPieceS ? threadIdx.x : 0)];
    }
    __device__ __forceinline__ void store(char *lds, const uint32_t *gtab) const {
        StagSet ss[2];
        sets(gtab, ss);
        fill.store(lds, ss);
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds + kPcOps);
#pragma unroll
        for (uint32_t k = 0; k < kOpPer; ++k) {
            const uint32_t i = threadIdx.x + k * THREADS;
            if (i < kOpQ) dst[i] = q[k];
        }
        if (threadIdx.x <= kPieceS) reinterpret_cast<uint32_t *>(lds + kPcHinit)[threadIdx.x] = hv;
    }
};

template <class Prov, class Epi>
__global__ __launch_bounds__(kPcThreads) void k_pieces(const uint8_t *__restrict__ base_in, uint32_t nbytes_in,
                                                 Prov prov_in, uint64_t n_in, Epi epi_in,
                                                 const uint32_t *__restrict__ gtab, uint32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint32_t lds_w[kPcLdsWords];
    char *lds = reinterpret_cast<char *>(lds_w);
    Prov prov = prov_in;
    Epi epi = epi_in;
    const uint8_t *base = base_in;
    uint32_t nbytes = nbytes_in;
    uint64_t n = n_in;
    if constexpr (kDevRange<Prov>) {
        if (!prov.bind(base, nbytes, n, epi)) return;  // this sub-launch's range is empty
    }
    const uint32_t nw = blockDim.x >> 6;
    const uint64_t tw = uint64_t(gridDim.x) * nw, w0 = uint64_t(blockIdx.x) * nw;
    const uint64_t g0 = n * w0 / tw, g1 = n * (w0 + nw) / tw;  // this workgroup's packets
    if (g0 == g1) return;  // no packets for this block
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(base, nbytes);
    PC_PROBE(0, __builtin_amdgcn_s_memrealtime());
    WaveSplit split;
    PcTables<kPcThreads> tb;
    // every table load first (one memory latency, and ahead of the length loads of the
    // wave split, since vmcnt completes in order; see StagFill).  (Lengths first, tables
    // behind them, the first round's metadata issued before the table stores wait:
    // neutral on C5, 53.4 vs 52.9 us back to back, profiles/r03f/abc5.log.)
    tb.load(gtab);
    if constexpr (Prov::kVarLen) split.load(prov, g0, g1);
    PC_PROBE(1, __builtin_amdgcn_s_memrealtime());
    tb.store(lds, gtab);
    uint64_t lo, hi;
    uint32_t wpieces = 0;  // pieces of this wave's range (variable-length providers)
    if constexpr (Prov::kVarLen) {
        split.finish(prov, g0, g1, lds, wave, lane, lo, hi, wpieces);  // two barriers; LDS outside the tables
    } else {
        lo = n * (w0 + wave) / tw;
        hi = n * (w0 + wave + 1) / tw;
    }
    MetaRaw raw{};
    if (lo < hi) pieces_meta(prov, lo, hi, lane, raw, rs);
    __syncthreads();  // the tables are visible to every wave
    PC_PROBE(2, __builtin_amdgcn_s_memrealtime());

    pieces_loop(lds, rs, prov, epi, lo, hi, wpieces, status, wave, lane, raw);
}

// ------------------------------------------------------------------------------------
// 2a. verify fix-up phase (end of k_fixed_braid<VerifyBEpi>)
// ------------------------------------------------------------------------------------
// The braided verify decides the datagrams of the ring's full length; every other one
// (short, empty, runt, 1473-1500 B in a 1504-B slot, oversize) was given ok = 0, crc = 0
// and counted by its wave's flush (nfix).  Once all waves of the workgroup are past their
// braided rounds, a workgroup that counted none returns (one barrier: the common case
// costs nothing).  Otherwise it rebuilds its LDS for the piece loop (PcTables), rescans
// its own packets in passes of kVfPass, compacts the listed ones into an LDS index list
// and finishes them with pieces_loop (DgramProvL semantics: CRC over [16, recv_len),
// Receiver.cpp:25-35,203-206).  Nothing lives outside the caller's buffers and the
// kernel: no list in global memory, no counters, no second launch, so any number of
// concurrent calls, streams and graph replays are independent.  A rescan that finds a
// different number of datagrams than the flushes counted (the recv_len array changed
// under the kernel) sets status bit 2.
//
// LDS after the braided rounds (the piece layout for 8 waves): tables [0, kPcStage),
// staging slots of waves 0..7, the index list where slots 8..15 of k_pieces would be,
// flags at kPcFlags, control words (per-wave counts, list length) past kPcLdsWords.
constexpr uint32_t kVfWaves = 8;  // the verify launch's 512 threads (VerifyBEpi::kThreads)
constexpr uint32_t kVfList = kPcStage + kVfWaves * kPcSlot;
constexpr uint32_t kVfCap = (kPcFlags - kVfList) / 4;
constexpr uint32_t kVfCtl = (kPcLdsWords * 4 + 15) & ~15u;
constexpr uint32_t kVfPer = 8;                          // packets rescanned per thread and pass
constexpr uint32_t kVfPass = kVfWaves * 64 * kVfPer;   // packets rescanned per pass
// A layout that leaves the fix-up list no room (a larger piece or slot, say) must not
// compile, rather than overwrite the flags with indices.
static_assert(kVfPass <= kVfCap && kVfCtl + 64 <= kBraidLdsWords * 4, "verify fix-up LDS");

typedef __attribute__((address_space(3))) uint32_t lu32;

// Datagram list[p] of the ring (lead 0: the ring is 16-B aligned); aux = ntohl(checksum).
struct LdsIdxDgramProv {
    static constexpr const char *kName = "LdsIdxDgramProv";  // wtp_last_kernel()
    static constexpr bool kVarLen = false;
    static constexpr bool kIndexed = true;
    static constexpr bool kGroupLoad = false;
    uint64_t stride;
    const uint32_t *__restrict__ rl;
    const lu32 *list;
    __device__ __forceinline__ void load(uint64_t p, MetaRaw &r, __amdgpu_buffer_rsrc_t rs) const {
        const uint32_t idx = list[p];
        const uint32_t h = uint32_t(uint64_t(idx) * stride + 12);  // 4-B aligned, the view is < 2 GiB
        r.a = idx;
        r.b = rl[idx];
        const u32x2 w = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, int(h), 0, 0));
        r.c = w.x;
        r.d = w.y;
    }
    __device__ __forceinline__ void decode(const MetaRaw &r, uint64_t &off, uint32_t &l, bool &ok, uint32_t &want,
                                           uint32_t &slot) const {
        const uint64_t d = r.a * stride;
        want = bswap32(r.c);  // d + 12 is 4-B aligned
        off = d + 16;
        ok = r.b >= 16 && r.b <= stride;
        l = ok ? r.b - 16 : 0;
        slot = uint32_t(r.a);
    }
};

// VEpi is VerifyBEpi (crc32_braid.hpp, included after this file): the ring, its recv_len
// array and the outputs come from the epilogue of the kernel that calls this.
template <class VEpi>
__device__ __forceinline__ void verify_fixup(char *lds, const VEpi &epi, const uint32_t *gtab, uint32_t nfix,
                                             uint64_t rstep, uint32_t wave, uint32_t lane) {
    lu32 *const ctl = (lu32 *)((lchar *)lds + kVfCtl);  // [w] = wave w's count, [8] = list length
    const uint32_t nwave = blockDim.x >> 6;
    if (lane == 0) ctl[wave] = nfix;
    __syncthreads();  // every wave is past its braided rounds and flushes
    uint32_t total = 0;
    for (uint32_t w = 0; w < nwave; ++w) total += ctl[w];
    total = __builtin_amdgcn_readfirstlane(total);
    if (total == 0) return;
    typedef __attribute__((address_space(1))) uint32_t gmu32;
    gmu32 *const st = (gmu32 *)epi.status;
    if (nwave != kVfWaves) {  // the host launches 512 threads; anything else cannot hold the list
        if (threadIdx.x == 0) __hip_atomic_fetch_or(st, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    {
        PcTables<kVfWaves * 64> tb;  // overwrites the braid tables: no wave reads them any more
        tb.load(gtab);
        tb.store(lds, gtab);
    }
    const uint64_t n = epi.n;
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(epi.ring, uint32_t((n * epi.stride + 15) & ~uint64_t(15)));
    const __amdgpu_buffer_rsrc_t rr = make_rsrc(epi.rl, uint32_t(4 * n));
    lu32 *const list = (lu32 *)((lchar *)lds + kVfList);
    const LdsIdxDgramProv prov{epi.stride, epi.rl, list};
    const VerifyEpi vepi{epi.ok, epi.crc, uint32_t(n)};
    const uint64_t g0 = uint64_t(blockIdx.x) * nwave;  // the workgroup's first round
    uint32_t found = 0;
    // the workgroup's packets in braided order: enumeration index e <-> packet
    // 4 (g0 + (e >> 5) rstep) + (e & 31) (wave (e & 31) >> 2's round of group e >> 5)
    for (uint64_t e0 = 0; 4 * (g0 + (e0 >> 5) * rstep) < n; e0 += kVfPass) {
        if (threadIdx.x == 0) ctl[8] = 0;
        __syncthreads();  // publishes the tables (first pass) and the reset list length
        uint64_t pv[kVfPer];
        uint32_t rv[kVfPer];
#pragma unroll
        for (uint32_t k = 0; k < kVfPer; ++k) {
            const uint64_t e = e0 + k * (kVfWaves * 64) + threadIdx.x;
            pv[k] = 4 * (g0 + (e >> 5) * rstep) + (e & 31u);
            rv[k] = __builtin_amdgcn_raw_buffer_load_b32(rr, pv[k] < n ? int(4 * pv[k]) : int(0x80000000u), 0, 0);
        }
#pragma unroll
        for (uint32_t k = 0; k < kVfPer; ++k) {
            const bool need = pv[k] < n && rv[k] != epi.full;
            const uint64_t m = __ballot(need);
            if (m == 0) continue;  // wave-uniform
            uint32_t b = 0;
            if (lane == 0) b = __hip_atomic_fetch_add(&ctl[8], uint32_t(__popcll(m)), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP);
            b = __builtin_amdgcn_readfirstlane(b);
            const uint32_t pos = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
            if (need) list[b + pos] = uint32_t(pv[k]);
        }
        __syncthreads();
        const uint32_t c = __builtin_amdgcn_readfirstlane(ctl[8]);
        found += c;
        const uint64_t lo = uint64_t(c) * wave / kVfWaves, hi = uint64_t(c) * (wave + 1) / kVfWaves;
        MetaRaw raw{};
        if (lo < hi) pieces_meta(prov, lo, hi, lane, raw, rs);
        pieces_loop(lds, rs, prov, vepi, lo, hi, 0u, epi.status, wave, lane, raw);
        __syncthreads();  // the next pass rebuilds the list
    }
    if (threadIdx.x == 0 && found != total) __hip_atomic_fetch_or(st, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace dev
}  // namespace wtp
