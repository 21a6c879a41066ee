// crc32_dev.hpp — what every kernel of crc32_kernels.hip shares: the layout of the device
// constant tables (OFF_*, filled by host_tables() in crc32_launch.hpp), the LDS layout
// constants of the braided kernel, address-space typedefs, PC_PROBE, and the device helpers
// (make_rsrc, the staggered tables' StagKeys / stag_apply* / StagFill, op_apply_fold,
// nib_apply, rotate_prio).  A part of the one translation unit crc32_kernels.hip, included
// there first, after the build switches; not a header for other units.
#pragma once

namespace wtp {

// ------------------------------------------------------------------------------------
// Device constant tables (one block per device, built once on the host)
// ------------------------------------------------------------------------------------
constexpr int kG = 16;                       // lanes per packet in the braided kernel
constexpr int kBraids = 4 * kG;              // 64 braids x 4-byte words
constexpr uint32_t kBraidBlock = 4 * kBraids;  // one row = 256 bytes
constexpr int kPieceS = 64;                  // piece bytes in the general kernel
constexpr uint32_t kHinitWords = (kPieceS + 4) & ~3;  // shift(~0, h), h = 0..kPieceS, padded
constexpr uint32_t kMaxVarLen = 4096;        // 64 pieces x 64 B: a packet fills one wave at most
constexpr uint64_t kSubBatch = 1ull << 28;   // packets per general-kernel launch (32-bit store offsets)

constexpr uint32_t OFF_BRAID = 0;            // 4x256 braid word tables (advance 256 B)
constexpr uint32_t OFF_INV = 1024;           // 6 ops: x^-32, x^-64, x^-128, x^-256, x^-512, x^-1024
constexpr uint32_t OFF_S4 = OFF_INV + 6 * 1024;   // 4x256 slice-by-4 word tables
constexpr uint32_t OFF_FWD = OFF_S4 + 1024;       // 6 ops: x^(8*S*d), d = 1..32 (S = kPieceS)
constexpr uint32_t OFF_HINIT = OFF_FWD + 6 * 1024;  // shift(~0, h), h = 0..S (head-piece init)
// k_stream (packed mixed lengths): T256 = shift by one 32-B block; 38 nibble operators
// (8 tables x 16 words each): shift by 128 * 2^k B (k = 0..5, the lane scan), then the
// payload-length shift in four 3-bit levels (level k, digit j: shift by j * 8^k B).
constexpr uint32_t OFF_T256 = OFF_HINIT + kHinitWords;
constexpr uint32_t kStNibOps = 6 + 32;
constexpr uint32_t OFF_NIB = OFF_T256 + 1024;
constexpr uint32_t TAB_WORDS = OFF_NIB + kStNibOps * 128;

// LDS images (staggered table sets are described at StagKeys below).
constexpr uint32_t kOpBytes = 4096;  // a plain operator: 4 byte tables x 256 words
// k_fixed_braid: region A = {braid tables, x^-32}, region B = {x^-128, x^-1024} (staggered,
// conflict-free), then the 16 waves' 2 KiB transposition slots.
constexpr uint32_t kBraidXpose = 131072;
constexpr uint32_t kBraidLdsWords = (kBraidXpose + 16 * 2048) / 4;  // 163,840 B

namespace dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
// Explicit global (address space 1) pointers for the streaming loads: a select between
// two generic pointers defeats address-space inference and degrades to flat_load, which
// also counts on lgkmcnt and serialises with the LDS lookups.
typedef const __attribute__((address_space(1))) uint8_t gu8;
typedef const __attribute__((address_space(1))) u32x4 gu32x4;
// Explicit LDS (address space 3) pointers for the general kernel's staging slots and
// flags: the accesses are ds_* by construction, never flat.
typedef __attribute__((address_space(3))) char lchar;
typedef __attribute__((address_space(3))) u32x4 lu32x4;
typedef __attribute__((address_space(3))) u32x2 lu32x2;
typedef __attribute__((address_space(3))) uint8_t lu8;

// Per-wave phase timestamps for tools/pprobe.hip (built with -DWTP_PROBE=1 there and
// compiled out of the product): slot k of wave (block, wave) gets value v, e.g. a
// 100 MHz s_memrealtime stamp.
#if WTP_PROBE
__device__ uint64_t *g_probe;
#define PC_PROBE(k, v)                                                                                  \
    do {                                                                                                \
        if (lane == 0u) g_probe[(uint64_t(blockIdx.x) * 16u + wave) * 8u + (k)] = (v);                 \
    } while (0)
#else
#define PC_PROBE(k, v) \
    do {               \
    } while (0)
#endif

__device__ __forceinline__ uint32_t lds_rd(const char *lds, uint32_t byte_addr) {
    return *reinterpret_cast<const uint32_t *>(lds + byte_addr);
}

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// the first active lane's v as a wave-uniform value in SGPRs (each half widened as unsigned)
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))))) |
           (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))))) << 32);
}

// Buffer resource over [base, base + nbytes) (nbytes rounded up to 16 by the host, so
// every 16-B block that holds a valid byte is in range); out-of-range loads return 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, uint32_t nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, (int)nbytes, 0x00020000);
}
__device__ __forceinline__ u32x4 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// w ^ f(v) for a linear operator f stored as 4 byte tables (256 words each) at LDS byte
// offset base: each byte address is one v_bfe + one v_lshl_or, the five-way XOR two
// v_bitop3 (the piece kernel's scan levels)
__device__ __forceinline__ uint32_t op_apply_fold(const char *lds, uint32_t base, uint32_t v, uint32_t w) {
    const uint32_t a0 = (__builtin_amdgcn_ubfe(v, 0, 8) << 2) | base;
    const uint32_t a1 = (__builtin_amdgcn_ubfe(v, 8, 8) << 2) | (base + 1024u);
    const uint32_t a2 = (__builtin_amdgcn_ubfe(v, 16, 8) << 2) | (base + 2048u);
    const uint32_t a3 = ((v >> 24) << 2) | (base + 3072u);
    return xor3(xor3(lds_rd(lds, a0), lds_rd(lds, a1), lds_rd(lds, a2)), lds_rd(lds, a3), w);
}

// ---- staggered 8-copy tables (conflict-free with a quarter of the replication) ------
// A "table set" is 4 byte-tables (256 u32 each) of one linear map.  Each 32-lane half of
// a wave is split into 4 groups of 8 lanes; in lookup instruction s, group g reads table
// (s + g) & 3, so the 4 groups always hit 4 different tables, and copy c = lane & 7 of
// table t lives in bank 8t + c: all 32 lanes touch distinct banks whatever the bytes.
// Every lane still XORs one entry of each of the 4 tables, just in a lane-dependent
// order.  Layout: 256-B rows, one per byte value e; two table sets per 64 KiB region:
//   byte address = region*65536 + e*256 + set*128 + t*32 + c*4.
// The per-lane key holds everything but e; v_perm_b32 with a per-lane selector drops the
// data byte t into bits 8..15, so each lookup is one v_perm + one ds_read_b32 (the set
// bit is the instruction's immediate offset).
struct StagKeys {
    uint32_t kA[4], kB[4], sel[4];
    __device__ __forceinline__ explicit StagKeys(uint32_t lane) {
        const uint32_t h = lane & 31u, g = (h >> 3) & 3u, c = h & 7u;
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) {
            const uint32_t t = (s + g) & 3u;
            kA[s] = (t << 5) | (c << 2);
            kB[s] = kA[s] | (1u << 16);
            sel[s] = 0x0C020000u | ((4u + t) << 8);
        }
    }
};

template <uint32_t OFF>
__device__ __forceinline__ uint32_t stag_apply(const char *lds, const uint32_t (&key)[4], const uint32_t (&sel)[4],
                                               uint32_t x) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, key[0], sel[0]);
    const uint32_t a1 = __builtin_amdgcn_perm(x, key[1], sel[1]);
    const uint32_t a2 = __builtin_amdgcn_perm(x, key[2], sel[2]);
    const uint32_t a3 = __builtin_amdgcn_perm(x, key[3], sel[3]);
    return (lds_rd(lds, a0 + OFF) ^ lds_rd(lds, a1 + OFF)) ^ (lds_rd(lds, a2 + OFF) ^ lds_rd(lds, a3 + OFF));
}

// Fill one table set (1024 words from global: table t at g[256 t]) into the staggered image.
// Store j (of 2048) writes the 16-B half h = j & 1 of table t = (j >> 1) & 3's 8 copies of
// entry e = j >> 3, so each 8-lane ds_write_b128 group covers 128 contiguous bytes (one
// entry per 32 B, lanes 256 B apart, was 8-way bank-conflicted: 3.4 us per launch).
__device__ __forceinline__ uint32_t stag_fill_word(uint32_t j) { return ((j >> 1) & 3u) * 256u + (j >> 3); }
__device__ __forceinline__ uint32_t stag_fill_off(uint32_t j) { return (j >> 3) * 256u + ((j >> 1) & 3u) * 32u + (j & 1u) * 16u; }
__device__ __forceinline__ void fill_stag(char *lds, uint32_t region, uint32_t set, const uint32_t *__restrict__ g) {
    for (uint32_t j = threadIdx.x; j < 2048; j += blockDim.x) {
        const uint32_t v = g[stag_fill_word(j)];
        *reinterpret_cast<u32x4 *>(lds + region * 65536u + set * 128u + stag_fill_off(j)) = u32x4{v, v, v, v};
    }
}

// Staggered fill of NS table sets with every global load of a thread issued before any
// LDS write.  The tables are usually evicted from L2 by the stream between launches, and
// the load-write loop of fill_stag paid one memory latency per word: entry to first
// round took 5.9 us in every braided launch (tools/bprobe.py), a third of a C2 launch.
struct StagSet {
    const uint32_t *g;  // 4 byte tables (1024 words)
    uint32_t off;       // region * 65536 + set * 128
};
// load() issues the loads, store() writes LDS: a kernel issues the table loads before
// its first data loads, since vmcnt completes in order and the table writes would
// otherwise wait for the first round's data (the fill ended 4.4 us after entry).
template <int NS, int THREADS>
struct StagFill {
    static_assert(THREADS <= 1024 && (NS * 512) % THREADS == 0 && (THREADS > 512 || 512 % THREADS == 0), "StagFill");
    // Load slot s of a set (512 per set) covers table t = (s >> 1) & 3, entries
    // 4g .. 4g+3 (g = s >> 3), half h = s & 1 of their 8 copies: one 16-B global load, four
    // 16-B LDS stores (each 8-lane group still writes 128 contiguous bytes of one row).
    // A quarter of the vector memory instructions of one dword load per store: C2 (64 K
    // packets) 15.46 -> 14.29 us from a graph, 16 K 7.03 -> 5.98, 1 M 216.5 -> 214.9
    // (interleaved, profiles/r04fx).  The piece kernel's 1024-thread fill too since round 6
    // (7 -> 4 loads per thread): C5 1 M 47.4 -> 47.0-47.2 us median, 64 K mixed 19.2 ->
    // 18.6-18.7 (interleaved, both library orders, profiles/r06c).
    static constexpr int PER = NS * 512 / THREADS;  // loads per thread
    u32x4 v[PER];
    __device__ __forceinline__ void load(const StagSet (&sets)[NS]) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t sidx = (uint32_t(k * THREADS) + threadIdx.x) & 511u;
            if constexpr (THREADS <= 512) {  // one set per k
                v[k] = *reinterpret_cast<const u32x4 *>(sets[(k * THREADS) >> 9].g + ((sidx >> 1) & 3u) * 256u +
                                                        4u * (sidx >> 3));
            } else {  // the set as an offset from set 0 (a select between pointers would be flat)
                const uint32_t si = (uint32_t(k * THREADS) + threadIdx.x) >> 9;
                ptrdiff_t gofs = 0;
#pragma unroll
                for (int i = 1; i < NS; ++i) gofs = si == uint32_t(i) ? sets[i].g - sets[0].g : gofs;
                v[k] = *reinterpret_cast<const u32x4 *>(sets[0].g + gofs + ((sidx >> 1) & 3u) * 256u + 4u * (sidx >> 3));
            }
        }
    }
    __device__ __forceinline__ void store(char *lds, const StagSet (&sets)[NS]) const {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint32_t sidx = (uint32_t(k * THREADS) + threadIdx.x) & 511u;
            uint32_t soff;
            if constexpr (THREADS <= 512) {
                soff = sets[(k * THREADS) >> 9].off;
            } else {
                const uint32_t si = (uint32_t(k * THREADS) + threadIdx.x) >> 9;
                soff = sets[0].off;
#pragma unroll
                for (int i = 1; i < NS; ++i) soff = si == uint32_t(i) ? sets[i].off : soff;
            }
            const uint32_t base = soff + (sidx >> 3) * 1024u + ((sidx >> 1) & 3u) * 32u + (sidx & 1u) * 16u;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                *reinterpret_cast<u32x4 *>(lds + base + i * 256u) = u32x4{v[k][i], v[k][i], v[k][i], v[k][i]};
        }
    }
};

// x ^ apply(set, x) folded with the next data word w: xor3(xor3(l0, l1, l2), l3, w).
template <uint32_t OFF>
__device__ __forceinline__ uint32_t stag_apply3x(const char *lds, const uint32_t (&key)[4], const uint32_t (&sel)[4],
                                                 uint32_t x, uint32_t w) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, key[0], sel[0]);
    const uint32_t a1 = __builtin_amdgcn_perm(x, key[1], sel[1]);
    const uint32_t a2 = __builtin_amdgcn_perm(x, key[2], sel[2]);
    const uint32_t a3 = __builtin_amdgcn_perm(x, key[3], sel[3]);
    return xor3(xor3(lds_rd(lds, a0 + OFF), lds_rd(lds, a1 + OFF), lds_rd(lds, a2 + OFF)), lds_rd(lds, a3 + OFF), w);
}

template <uint32_t OFF>
__device__ __forceinline__ uint32_t stag_apply3(const char *lds, const uint32_t (&key)[4], const uint32_t (&sel)[4],
                                                uint32_t x) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, key[0], sel[0]);
    const uint32_t a1 = __builtin_amdgcn_perm(x, key[1], sel[1]);
    const uint32_t a2 = __builtin_amdgcn_perm(x, key[2], sel[2]);
    const uint32_t a3 = __builtin_amdgcn_perm(x, key[3], sel[3]);
    return xor3(lds_rd(lds, a0 + OFF), lds_rd(lds, a1 + OFF), lds_rd(lds, a2 + OFF)) ^ lds_rd(lds, a3 + OFF);
}

// Operator stored as 8 nibble tables of 16 words at LDS byte address `base` (which may
// differ per lane): f(v) = XOR_i N_i[(v >> 4i) & 15].  A table's 16 words sit in 16
// consecutive banks, so a wave-uniform operator never conflicts.
__device__ __forceinline__ uint32_t nib_apply(const char *lds, uint32_t base, uint32_t v) {
    uint32_t l[8];
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) l[i] = lds_rd(lds, base + 64u * i + 4u * __builtin_amdgcn_ubfe(v, 4 * i, 4));
    return xor3(xor3(l[0], l[1], l[2]), xor3(l[3], l[4], l[5]), l[6] ^ l[7]);
}

// Wave issue priority, rotated (general kernel).  The SIMD arbiter favours the oldest of
// equal-priority waves: with static per-wave work, the four waves sharing a SIMD ran at
// unequal speeds (k_pieces on C5: 2.8 us per round for the oldest, 4.2 us for the
// youngest; tools/pprobe.py) and the launch waited for the youngest while its SIMD ran
// nearly empty.  Each wave steps its priority through 0..3 per round (x = round counter
// + the wave's age rank), so each spends a quarter of its rounds at every level: C5
// 57.6 -> 54.6 us (interleaved A/B, tools/ab_c5.py).  The braided kernel, at the read
// ceiling, lost 1% with it (and 2.5% with dynamic per-workgroup group claims).
__device__ __forceinline__ void rotate_prio(uint32_t x) {
    switch (x & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

}  // namespace dev
}  // namespace wtp
