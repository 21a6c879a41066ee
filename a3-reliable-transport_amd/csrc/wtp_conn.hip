// wtp_conn.hip — the device-side connection table (include/wtp_crc32.h: wtp_flows_classify,
// wtp_flows_control): a caller-owned table from a datagram's 16-byte source address to its
// flow, one call that classifies a batch by address and one that applies the batch's START
// and END datagrams: opens flows, closes flows and writes the control ACKs.
//
// The table is nbuckets buckets of kConnWays entries; a bucket is 16 tag words followed by 16
// keys of 16 bytes (320 B).  A tag is 0xFFFFFFFF (empty, d_slot_len's convention), a flow id, or,
// inside wtp_flows_control only, a claim 0x80000000 | i of datagram i (k_accept_claim's
// encoding); occupancy lives in the tag, so every 16-byte value is a key.  A key belongs to
// bucket conn_hash(key) & (nbuckets - 1), on the host and on the device alike.
//
//   classify  k_conn_classify  one lane per datagram: the key's bucket, its 16 tags, and the
//                              key of every entry that holds a flow id
//   control   1. k_conn_mark   one lane per datagram: the verdicts that need no contention;
//                              a START of a new key scans its bucket in order and claims the
//                              first empty entry (atomicCAS) or joins the claim that holds its
//                              key (atomicMin: the lowest index stays).  Tags only go from
//                              empty to occupied in this launch and an occupied entry's key
//                              is fixed (the key behind a claim is d_keys[i] of the batch), so
//                              all datagrams of one key meet in one entry.  Lanes [0, nflows)
//                              initialise the per-flow scratch words.
//             2. k_conn_count  the claim that is still in its entry is the key's opener;
//                              count per 1024 datagrams.  END candidates atomicMin their
//                              index into their flow's scratch word.
//             3. k_conn_open   ranks the openers in arrival order: rank r below the free ids
//                              takes d_free[(head + r) mod nflows], writes key, tag and the
//                              per-flow words; a higher rank releases its entry.  The first
//                              END candidate of a flow is its closer; count per 1024.
//             4. k_conn_close  ranks the closers: free the entry, push the id.  Same-key
//                              followers read what their opener left in the entry.  Every
//                              verdict is final; count the answered per 1024.
//             5. k_conn_emit   ranks the answered: ACKs, d_verdict; one lane writes d_counts
//                              and d_free_pos.
//             6. k_conn_reset  one lane per global slot: EMPTY where the flow was opened now.
//
// The three ordered rankings share block_count / block_rank below, which stay in this unit
// (DESIGN.md 3.8).  A separate translation unit: see wtp_common.hpp.
#include <algorithm>

#include "wtp_common.hpp"

namespace wtp {

// The bucket hash over the key's four little-endian dwords; the host function and the
// kernels share this one body.
__host__ __device__ inline uint32_t conn_hash(uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
    uint32_t h = k0 * 0x9E3779B1u;
    h = ((h << 13) | (h >> 19)) ^ k1;
    h *= 0x85EBCA77u;
    h = ((h << 13) | (h >> 19)) ^ k2;
    h *= 0xC2B2AE3Du;
    h = ((h << 13) | (h >> 19)) ^ k3;
    h *= 0x27D4EB2Fu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}

inline bool conn_buckets_ok(uint32_t nbuckets) {
    return nbuckets != 0 && (nbuckets & (nbuckets - 1)) == 0 && nbuckets <= WTP_CONN_MAX_BUCKETS;
}

namespace dev {

constexpr uint32_t kConnEmpty = 0xFFFFFFFFu;  // an empty tag; also "no END candidate yet"
constexpr uint32_t kConnClaim = 0x80000000u;  // claim of datagram i = kConnClaim | i (n < 2^31)
constexpr uint32_t kConnWays = WTP_CONN_WAYS;
constexpr uint32_t kConnBucketWords = kConnWays + kConnWays * (WTP_CONN_KEY_BYTES / 4);  // 16 tags, 16 keys
constexpr uint32_t kConnBlock = 1024;  // datagrams per block of the ranking kernels
constexpr uint32_t kConnWaves = kConnBlock / 64;

// st[i], a datagram's word of scratch: bits 0 .. 3 its verdict (WTP_CTL_*) or, until the
// kernel that settles it, its role; bits 4 .. 27 its table entry, bucket * 16 + way.
constexpr uint32_t kRoleClaim = 10;   // a new-key START with an entry: opener or follower
constexpr uint32_t kRoleOpener = 11;  // ... whose claim stayed in the entry
constexpr uint32_t kRoleEnd = 12;     // an END that may close its flow
constexpr uint32_t kRoleCloser = 13;  // ... the first of its flow
constexpr uint32_t kConnHdr = 4;      // scratch words {openers, closers, refused full, refused bucket}

__device__ __forceinline__ uint32_t tag_load(const uint32_t *tag) {
    return __hip_atomic_load(tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 16 bytes at p as four little-endian dwords: one 16-B load where aligned, dwords where
// 4-B aligned, bytes otherwise (no access wider than the key's alignment).
__device__ __forceinline__ u32x4 load_key(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15u) == 0) return *reinterpret_cast<const u32x4 *>(p);
    u32x4 k;
    if ((a & 3u) == 0) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
        k.x = w[0], k.y = w[1], k.z = w[2], k.w = w[3];
        return k;
    }
    k.x = __builtin_bswap32(be32(p)), k.y = __builtin_bswap32(be32(p + 4));
    k.z = __builtin_bswap32(be32(p + 8)), k.w = __builtin_bswap32(be32(p + 12));
    return k;
}

__device__ __forceinline__ bool key_eq(u32x4 a, u32x4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

__device__ __forceinline__ uint32_t key_bucket(u32x4 k, uint32_t nbuckets) {
    return conn_hash(k.x, k.y, k.z, k.w) & (nbuckets - 1);
}

__device__ __forceinline__ const u32x4 *bucket_keys(const uint32_t *tags) {
    return reinterpret_cast<const u32x4 *>(tags + kConnWays);  // 64 B past a 16-B aligned bucket
}

__global__ void __launch_bounds__(256)
k_conn_classify(const uint8_t *__restrict__ keys, uint64_t key_stride, uint32_t n, const uint32_t *__restrict__ table,
                uint32_t nbuckets, uint32_t *__restrict__ flow) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32x4 key = load_key(keys + uint64_t(i) * key_stride);
    const uint32_t *tags = table + uint64_t(key_bucket(key, nbuckets)) * kConnBucketWords;
    const u32x4 *bkeys = bucket_keys(tags);
    uint32_t f = WTP_NO_FLOW;
    for (uint32_t e = 0; e < kConnWays; ++e) {
        const uint32_t t = tags[e];
        if (t < kConnClaim && key_eq(bkeys[e], key)) {  // a flow id; no claim outlives wtp_flows_control
            f = t;
            break;
        }
    }
    flow[i] = f;
}

// Is datagram i a control datagram?  The header is read only where ok says it is there.
__device__ __forceinline__ bool control_header(const uint8_t *__restrict__ ring, uint64_t stride,
                                               const uint8_t *__restrict__ ok, uint32_t i, uint32_t &type, uint32_t &seq) {
    if (ok[i] == 0) return false;
    const Header hd = load_header(ring + uint64_t(i) * stride);  // type, seq
    type = hd.type;
    seq = hd.seq;
    return type == WTP_TYPE_START || type == WTP_TYPE_END;
}

__global__ void __launch_bounds__(256)
k_conn_mark(const uint8_t *__restrict__ ring, uint64_t stride, const uint8_t *__restrict__ keys, uint64_t key_stride,
            const uint32_t *__restrict__ flow, const uint8_t *__restrict__ ok, uint32_t n, uint32_t *table,
            uint32_t nbuckets, uint32_t nflows, uint32_t window, const uint32_t *__restrict__ flow_start,
            const uint32_t *__restrict__ slot_len, uint32_t *__restrict__ hdr, uint32_t *__restrict__ end_min,
            uint32_t *__restrict__ opened_now, uint32_t *__restrict__ st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nflows) {
        end_min[i] = kConnEmpty;
        opened_now[i] = 0;
    }
    if (i < kConnHdr) hdr[i] = 0;
    if (i >= n) return;
    uint32_t type = 0, seq = 0;
    if (!control_header(ring, stride, ok, i, type, seq)) {
        st[i] = WTP_CTL_NONE;
        return;
    }
    const uint32_t f = flow[i];
    if (type == WTP_TYPE_START && f < nflows) {
        st[i] = seq == flow_start[f] ? WTP_CTL_START_DUP : WTP_CTL_START_OTHER;
        return;
    }
    if (type == WTP_TYPE_END && f >= nflows) {
        st[i] = WTP_CTL_END_STALE;
        return;
    }
    if (type == WTP_TYPE_END) {
        if (seq != flow_start[f]) {
            st[i] = WTP_CTL_END_OTHER;
            return;
        }
        if (window > 0 && slot_len[uint64_t(f) * window] != WTP_SLOT_EMPTY) {
            st[i] = WTP_CTL_END_BUSY;
            return;
        }
    } else if (nflows == 0) {  // no id can be free; the table may be NULL
        st[i] = WTP_CTL_REFUSED_FULL;
        return;
    }
    const u32x4 key = load_key(keys + uint64_t(i) * key_stride);
    const uint32_t b = key_bucket(key, nbuckets);
    uint32_t *tags = table + uint64_t(b) * kConnBucketWords;
    if (type == WTP_TYPE_END) {
        // the entry of flow f; with d_flow from wtp_flows_classify on this table it is there
        uint32_t v = WTP_CTL_END_OTHER;
        for (uint32_t e = 0; e < kConnWays; ++e)
            if (tag_load(&tags[e]) == f) {
                v = kRoleEnd | ((b * kConnWays + e) << 4);
                break;
            }
        st[i] = v;
        return;
    }
    const uint32_t mine = kConnClaim | i;
    uint32_t v = WTP_CTL_REFUSED_BUCKET;
    for (uint32_t e = 0; e < kConnWays; ++e) {
        uint32_t t = tag_load(&tags[e]);
        if (t == kConnEmpty) {  // a stale "empty" is harmless: the CAS returns the truth
            t = atomicCAS(&tags[e], kConnEmpty, mine);
            if (t == kConnEmpty) t = mine;
        }
        if (t == mine) {
            v = kRoleClaim | ((b * kConnWays + e) << 4);
            break;
        }
        if (t >= kConnClaim) {  // another datagram's claim: the same key?
            const uint32_t j = t & ~kConnClaim;
            if (j < n && key_eq(load_key(keys + uint64_t(j) * key_stride), key)) {
                atomicMin(&tags[e], mine);  // still a claim of this key: the lowest index stays
                v = kRoleClaim | ((b * kConnWays + e) << 4);
                break;
            }
        }
    }
    st[i] = v;
}

// blk[blockIdx.x] = the number of this block's lanes with `flag`.
__device__ __forceinline__ void block_count(bool flag, uint32_t *__restrict__ blk) {
    __shared__ uint32_t part[kConnWaves];
    const uint32_t t = threadIdx.x;
    const uint64_t b = __ballot(flag);
    if ((t & 63u) == 0) part[t / 64] = uint32_t(__popcll(b));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kConnWaves; ++w) sum += part[w];
        blk[blockIdx.x] = sum;
    }
}

// The number of lanes with `flag` in front of this one, over the whole grid in index order,
// from the per-block counts; total = all of them.  Every lane of the block calls it.
__device__ __forceinline__ uint32_t block_rank(bool flag, const uint32_t *__restrict__ blk, uint32_t nblk, uint32_t &total) {
    __shared__ uint32_t before[kConnWaves], all[kConnWaves], wave_n[kConnWaves];
    const uint32_t t = threadIdx.x, w = t / 64, lane = t & 63u;
    uint32_t c_before = 0, c_all = 0;
    for (uint32_t b = t; b < nblk; b += kConnBlock) {
        const uint32_t c = blk[b];
        c_all += c;
        c_before += b < blockIdx.x ? c : 0u;
    }
    c_before = wave_sum(c_before);
    c_all = wave_sum(c_all);
    const uint64_t ballot = __ballot(flag);
    if (lane == 0) {
        before[w] = c_before;
        all[w] = c_all;
        wave_n[w] = uint32_t(__popcll(ballot));
    }
    __syncthreads();
    uint32_t rank = 0;
    total = 0;
    for (uint32_t k = 0; k < kConnWaves; ++k) {
        rank += before[k] + (k < w ? wave_n[k] : 0u);
        total += all[k];
    }
    return rank + __builtin_amdgcn_mbcnt_hi(uint32_t(ballot >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(ballot), 0u));
}

__global__ void __launch_bounds__(kConnBlock)
k_conn_count(const uint32_t *__restrict__ flow, uint32_t n, const uint32_t *table, uint32_t *__restrict__ end_min,
             uint32_t *__restrict__ st, uint32_t *__restrict__ blk_open) {
    const uint32_t i = blockIdx.x * kConnBlock + threadIdx.x;
    bool opener = false;
    if (i < n) {
        const uint32_t s = st[i], role = s & 15u;
        if (role == kRoleClaim) {
            const uint32_t e = s >> 4;
            opener = table[uint64_t(e / kConnWays) * kConnBucketWords + e % kConnWays] == (kConnClaim | i);
            if (opener) st[i] = kRoleOpener | (e << 4);
        } else if (role == kRoleEnd) {
            atomicMin(&end_min[flow[i]], i);  // kRoleEnd: flow[i] < nflows
        }
    }
    block_count(opener, blk_open);
}

__global__ void __launch_bounds__(kConnBlock)
k_conn_open(const uint8_t *__restrict__ ring, uint64_t stride, const uint8_t *__restrict__ keys, uint64_t key_stride,
            const uint32_t *__restrict__ flow, uint32_t n, uint32_t *table, uint32_t nflows,
            uint32_t *__restrict__ flow_start, uint32_t *__restrict__ seq0, const uint32_t *__restrict__ free_ids,
            const uint32_t *__restrict__ free_pos, uint32_t *__restrict__ opened, uint32_t *__restrict__ opened_src,
            uint32_t *__restrict__ hdr, const uint32_t *__restrict__ end_min, uint32_t *__restrict__ opened_now,
            uint32_t *__restrict__ st, const uint32_t *__restrict__ blk_open, uint32_t nblk,
            uint32_t *__restrict__ blk_close) {
    const uint32_t i = blockIdx.x * kConnBlock + threadIdx.x;
    const uint32_t s = i < n ? st[i] : 0u, role = s & 15u;
    uint32_t total = 0;
    const uint32_t r = block_rank(role == kRoleOpener, blk_open, nblk, total);
    if (i == 0) hdr[0] = total;
    if (role == kRoleOpener) {
        const uint32_t e = s >> 4;
        uint32_t *tags = table + uint64_t(e / kConnWays) * kConnBucketWords;
        const uint32_t head = free_pos[0] % nflows, avail = min(free_pos[1], nflows);  // an opener: nflows > 0
        const uint32_t g = r < avail ? free_ids[(head + r) % nflows] : WTP_NO_FLOW;
        if (g < nflows) {
            reinterpret_cast<u32x4 *>(tags + kConnWays)[e % kConnWays] = load_key(keys + uint64_t(i) * key_stride);
            tags[e % kConnWays] = g;
            flow_start[g] = load_header(ring + uint64_t(i) * stride).seq;
            seq0[g] = 0;
            opened_now[g] = 1;
            opened[r] = g;
            if (opened_src) opened_src[r] = i;
            st[i] = WTP_CTL_OPENED;
        } else {  // no free id (or a ring cell that holds none): the entry is released
            tags[e % kConnWays] = kConnEmpty;
            st[i] = WTP_CTL_REFUSED_FULL;
        }
    }
    const bool closer = role == kRoleEnd && end_min[flow[i]] == i;
    if (closer) st[i] = kRoleCloser | (s & ~15u);
    block_count(closer, blk_close);
}

__global__ void __launch_bounds__(kConnBlock)
k_conn_close(const uint8_t *__restrict__ ring, uint64_t stride, const uint32_t *__restrict__ flow, uint32_t n,
             uint32_t *table, uint32_t nflows, const uint32_t *__restrict__ flow_start, uint32_t *__restrict__ free_ids,
             const uint32_t *__restrict__ free_pos, uint32_t *__restrict__ closed, uint32_t *__restrict__ hdr,
             uint32_t *__restrict__ st, const uint32_t *__restrict__ blk_close, uint32_t nblk,
             uint32_t *__restrict__ blk_ans) {
    const uint32_t i = blockIdx.x * kConnBlock + threadIdx.x;
    const uint32_t s = i < n ? st[i] : 0u, role = s & 15u;
    uint32_t total = 0;
    const uint32_t q = block_rank(role == kRoleCloser, blk_close, nblk, total);
    if (i == 0) hdr[1] = total;
    uint32_t v = role;
    if (role == kRoleCloser) {
        const uint32_t e = s >> 4, f = flow[i];
        table[uint64_t(e / kConnWays) * kConnBucketWords + e % kConnWays] = kConnEmpty;
        const uint32_t head = free_pos[0] % nflows, have = min(free_pos[1], nflows);
        free_ids[(head + have + q) % nflows] = f;  // behind the cells that hold ids: none of them is popped
        closed[q] = f;
        v = WTP_CTL_CLOSED;
    } else if (role == kRoleEnd) {  // a later END of a flow closed in this call
        v = WTP_CTL_END_STALE;
    } else if (role == kRoleClaim) {  // a follower: what the key's opener left in the entry
        const uint32_t e = s >> 4;
        const uint32_t g = table[uint64_t(e / kConnWays) * kConnBucketWords + e % kConnWays];
        if (g < nflows)
            v = load_header(ring + uint64_t(i) * stride).seq == flow_start[g] ? WTP_CTL_START_DUP : WTP_CTL_START_OTHER;
        else
            v = WTP_CTL_REFUSED_FULL;
    }
    if (i < n && v != s) st[i] = v;
    const uint64_t full = __ballot(i < n && v == WTP_CTL_REFUSED_FULL);
    const uint64_t bucket = __ballot(i < n && v == WTP_CTL_REFUSED_BUCKET);
    if ((threadIdx.x & 63u) == 0) {
        if (full) atomicAdd(&hdr[2], uint32_t(__popcll(full)));
        if (bucket) atomicAdd(&hdr[3], uint32_t(__popcll(bucket)));
    }
    const bool ans = i < n && (v == WTP_CTL_OPENED || v == WTP_CTL_START_DUP || v == WTP_CTL_CLOSED || v == WTP_CTL_END_STALE);
    block_count(ans, blk_ans);
}

// hdr == NULL: n == 0, and one lane only writes d_counts.
__global__ void __launch_bounds__(kConnBlock)
k_conn_emit(const uint8_t *__restrict__ ring, uint64_t stride, uint32_t n, uint32_t nflows,
            uint32_t *__restrict__ free_pos, uint8_t *__restrict__ wire, uint64_t ack_stride, uint32_t max_acks,
            uint32_t *__restrict__ src, uint32_t *__restrict__ verdict, uint32_t *__restrict__ counts,
            const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ st, const uint32_t *__restrict__ blk_ans,
            uint32_t nblk) {
    const uint32_t i = blockIdx.x * kConnBlock + threadIdx.x;
    const uint32_t v = i < n ? st[i] : 0u;
    const bool ans = v == WTP_CTL_OPENED || v == WTP_CTL_START_DUP || v == WTP_CTL_CLOSED || v == WTP_CTL_END_STALE;
    uint32_t total = 0;
    const uint32_t k = block_rank(ans, blk_ans, nblk, total);
    if (i == 0) {
        uint32_t opened = 0, closed = 0;
        if (hdr && nflows > 0) {
            const uint32_t head = free_pos[0] % nflows, have = min(free_pos[1], nflows);
            opened = min(hdr[0], have);
            closed = hdr[1];
            free_pos[0] = (head + opened) % nflows;
            free_pos[1] = have - opened + closed;
        }
        counts[0] = min(total, max_acks);
        counts[1] = total;
        counts[2] = opened;
        counts[3] = closed;
        counts[4] = hdr ? hdr[2] : 0u;
        counts[5] = hdr ? hdr[3] : 0u;
    }
    if (i >= n) return;
    if (verdict) verdict[i] = v;
    if (!ans || k >= max_acks) return;
    const uint32_t seq = load_header(ring + uint64_t(i) * stride).seq;
    store_ack(wire + uint64_t(k) * ack_stride, seq);  // the datagram's own seqNum
    if (src) src[k] = i;
}

__global__ void __launch_bounds__(256)
k_conn_reset(const uint32_t *__restrict__ opened_now, uint32_t window, uint32_t slots, uint32_t *__restrict__ slot_len) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < slots && opened_now[g / window]) slot_len[g] = WTP_SLOT_EMPTY;
}

}  // namespace dev
}  // namespace wtp

namespace {

// d_work of wtp_flows_control: hdr[4], end_min[nflows], opened_now[nflows], st[n] and three
// count arrays of ceil(n / 1024).
struct ConnWork {
    uint32_t *hdr, *end_min, *opened_now, *st, *blk_open, *blk_close, *blk_ans;
    size_t bytes;
};

ConnWork conn_layout(void *d_work, size_t n, uint32_t nflows) {
    wtp::Work l(d_work, 4);
    ConnWork w;
    const size_t nblk = (n + wtp::dev::kConnBlock - 1) / wtp::dev::kConnBlock;
    w.hdr = l.take<uint32_t>(wtp::dev::kConnHdr);
    w.end_min = l.take<uint32_t>(nflows);
    w.opened_now = l.take<uint32_t>(nflows);
    w.st = l.take<uint32_t>(n);
    w.blk_open = l.take<uint32_t>(nblk);
    w.blk_close = l.take<uint32_t>(nblk);
    w.blk_ans = l.take<uint32_t>(nblk);
    w.bytes = l.bytes();
    return w;
}

int check_buckets(uint32_t nbuckets) {
    if (wtp::conn_buckets_ok(nbuckets)) return WTP_OK;
    return wtp::fail(WTP_EINVAL, "nbuckets %u is not a power of two in [1, %u]", nbuckets, WTP_CONN_MAX_BUCKETS);
}

int check_table_align(const void *d_table) {
    if ((reinterpret_cast<uintptr_t>(d_table) & 15u) == 0) return WTP_OK;
    return wtp::fail(WTP_EINVAL, "d_table %p is not 16-byte aligned", d_table);
}

}  // namespace

extern "C" size_t wtp_conn_table_bytes(uint32_t nbuckets) {
    return wtp::conn_buckets_ok(nbuckets) ? size_t(nbuckets) * wtp::dev::kConnBucketWords * 4 : 0;
}

extern "C" uint32_t wtp_conn_bucket(const void *key16, uint32_t nbuckets) {
    if (!key16 || !wtp::conn_buckets_ok(nbuckets)) return WTP_NO_FLOW;
    const uint8_t *p = static_cast<const uint8_t *>(key16);
    uint32_t k[4];
    for (int w = 0; w < 4; ++w)
        k[w] = uint32_t(p[4 * w]) | (uint32_t(p[4 * w + 1]) << 8) | (uint32_t(p[4 * w + 2]) << 16) | (uint32_t(p[4 * w + 3]) << 24);
    return wtp::conn_hash(k[0], k[1], k[2], k[3]) & (nbuckets - 1);
}

extern "C" int wtp_flows_classify(const void *d_keys, size_t key_stride, size_t n, const void *d_table, uint32_t nbuckets,
                                  uint32_t *d_flow, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if (key_stride < WTP_CONN_KEY_BYTES) return fail(WTP_EINVAL, "key_stride %zu < 16", key_stride);
    if ((rc = check_buckets(nbuckets))) return rc;
    if (n == 0) return WTP_OK;
    if (!d_keys) return null_arg("d_keys");
    if (!d_table) return null_arg("d_table");
    if (!d_flow) return null_arg("d_flow");
    if ((rc = check_table_align(d_table))) return rc;
    return launch("k_conn_classify", dev::k_conn_classify, dim3(unsigned((n + 255) / 256)), dim3(256),
                  static_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_keys), uint64_t(key_stride), uint32_t(n),
                  static_cast<const uint32_t *>(d_table), nbuckets, d_flow);
}

extern "C" size_t wtp_conn_scratch_bytes(size_t n, uint32_t nflows) {
    return conn_layout(nullptr, std::min<size_t>(n, (size_t(1) << 31) - 1), std::min(nflows, WTP_RX_MAX_FLOWS)).bytes;
}

extern "C" int wtp_flows_control(const void *d_dgrams, size_t stride, const uint32_t *d_recv_len, const void *d_keys,
                                 size_t key_stride, const uint32_t *d_flow, const uint8_t *d_ok, size_t n, void *d_table,
                                 uint32_t nbuckets, uint32_t nflows, uint32_t window, uint32_t *d_flow_start,
                                 uint32_t *d_seq0, uint32_t *d_slot_len, uint32_t *d_free, uint32_t *d_free_pos,
                                 void *d_ack_wire, size_t ack_stride, uint32_t max_acks, uint32_t *d_ack_src,
                                 uint32_t *d_opened, uint32_t *d_opened_src, uint32_t *d_closed, uint32_t *d_verdict,
                                 uint32_t *d_counts, void *d_work, size_t work_bytes, void *stream) {
    using namespace wtp;
    int rc = check_batch(n);
    if (rc) return rc;
    if ((rc = check_stride(stride))) return rc;
    if (key_stride < WTP_CONN_KEY_BYTES) return fail(WTP_EINVAL, "key_stride %zu < 16", key_stride);
    if (ack_stride < 16) return fail(WTP_EINVAL, "ack_stride %zu < 16", ack_stride);
    if ((rc = check_buckets(nbuckets))) return rc;
    if ((rc = check_flows(nflows, window))) return rc;
    const ConnWork w = conn_layout(d_work, n, nflows);
    if ((rc = check_work_bytes(work_bytes, w.bytes))) return rc;
    if (!d_counts) return null_arg("d_counts");
    if (!d_work) return null_arg("d_work");
    const uint32_t slots = nflows * window;  // <= WTP_RX_MAX_FLOW_SLOTS
    if (nflows > 0) {
        if (!d_table) return null_arg("d_table");
        if (!d_flow_start) return null_arg("d_flow_start");
        if (!d_seq0) return null_arg("d_seq0");
        if (!d_free) return null_arg("d_free");
        if (!d_free_pos) return null_arg("d_free_pos");
        if (!d_opened) return null_arg("d_opened");
        if (!d_closed) return null_arg("d_closed");
    }
    if (slots > 0 && !d_slot_len) return null_arg("d_slot_len");
    if (n > 0) {
        if (!d_dgrams) return null_arg("d_dgrams");
        if (!d_recv_len) return null_arg("d_recv_len");
        if (!d_ok) return null_arg("d_ok");
        if (!d_keys) return null_arg("d_keys");
        if (!d_flow) return null_arg("d_flow");
        if (max_acks > 0 && !d_ack_wire) return null_arg("d_ack_wire");
    }
    if ((rc = check_table_align(d_table))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint8_t *ring = static_cast<const uint8_t *>(d_dgrams), *keys = static_cast<const uint8_t *>(d_keys);
    uint32_t *table = static_cast<uint32_t *>(d_table);
    uint8_t *wire = static_cast<uint8_t *>(d_ack_wire);
    const uint32_t n32 = uint32_t(n), nblk = uint32_t((n + dev::kConnBlock - 1) / dev::kConnBlock);
    const dim3 ranked(std::max(nblk, 1u)), block(dev::kConnBlock);
    if (n == 0)  // nothing can change: one block, which only writes d_counts
        return launch("k_conn_emit", dev::k_conn_emit, ranked, block, st, ring, uint64_t(stride), 0u, nflows, d_free_pos, wire,
                      uint64_t(ack_stride), max_acks, d_ack_src, d_verdict, d_counts, nullptr, w.st, w.blk_ans, 0u);
    rc = launch("k_conn_mark", dev::k_conn_mark, dim3((std::max(n32, nflows) + 255) / 256), dim3(256), st, ring,
                uint64_t(stride), keys, uint64_t(key_stride), d_flow, d_ok, n32, table, nbuckets, nflows, window, d_flow_start,
                d_slot_len, w.hdr, w.end_min, w.opened_now, w.st);
    if (rc) return rc;
    rc = launch("k_conn_count", dev::k_conn_count, ranked, block, st, d_flow, n32, table, w.end_min, w.st, w.blk_open);
    if (rc) return rc;
    rc = launch("k_conn_open", dev::k_conn_open, ranked, block, st, ring, uint64_t(stride), keys, uint64_t(key_stride), d_flow,
                n32, table, nflows, d_flow_start, d_seq0, d_free, d_free_pos, d_opened, d_opened_src, w.hdr, w.end_min,
                w.opened_now, w.st, w.blk_open, nblk, w.blk_close);
    if (rc) return rc;
    rc = launch("k_conn_close", dev::k_conn_close, ranked, block, st, ring, uint64_t(stride), d_flow, n32, table, nflows,
                d_flow_start, d_free, d_free_pos, d_closed, w.hdr, w.st, w.blk_close, nblk, w.blk_ans);
    if (rc) return rc;
    rc = launch("k_conn_emit", dev::k_conn_emit, ranked, block, st, ring, uint64_t(stride), n32, nflows, d_free_pos, wire,
                uint64_t(ack_stride), max_acks, d_ack_src, d_verdict, d_counts, w.hdr, w.st, w.blk_ans, nblk);
    if (rc || slots == 0) return rc;
    return launch("k_conn_reset", dev::k_conn_reset, dim3((slots + 255) / 256), dim3(256), st, w.opened_now, window, slots,
                  d_slot_len);
}
