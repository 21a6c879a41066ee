// wtp_concat.hip — whole-buffer CRC-32 on the device (include/wtp_crc32.h:
// wtp_crc32_concat, wtp_crc32_buffer): the fold of per-payload CRCs into the CRC of their
// concatenation, zlib crc32_combine semantics (crc32_combine.hpp),
//
//   crc32(p_0 || .. || p_{n-1}) = XOR_i crc_i * x^(8 S_i) mod P,   S_i = bytes after payload i.
//
// Fixed lengths (k_concat_fold).  Payloads 0 .. n-2 all have `len` bytes, so their fold is
// a Horner scheme in one constant m = x^(8 len).  A thread walks `run` consecutive CRCs,
// acc = acc * m ^ crc, with m as the 4 x 256 byte-table operator (built in LDS by each
// workgroup: 4 entries per thread); the 256 thread values are then folded by a tree whose
// level j multiplies by the constant m^(run 2^j).  Every constant is computed on the host
// (square and multiply, nanoseconds) and arrives as a kernel argument, so on the device a
// multiplication is always by a wave-uniform value: the 32-step shift/xor loop.  The
// tree's constants arrive as their whole chains c x^i, which takes the chain off the
// scalar unit (the tree was the larger part of both launches).  The element count is padded to groups * 256 * run
// with virtual elements IN FRONT: a leading zero CRC contributes nothing whatever its
// length, so every thread and every workgroup is uniform and no step needs an inverse.
// A second launch of the same kernel (one workgroup, elements = the first launch's
// partials, constant m^(256 run)) folds the partials and applies the three terms that are
// not of the common length: * x^(8 last_len) ^ crc_{n-1}, and for the buffer call
// ^ crc_head * x^(8 (nbytes - head)).  Up to 256 * 16 + 1 CRCs take one launch.
//
// Variable lengths (k_concat_var).  The reduction with the associative operator
// (a, la) o (b, lb) = (a x^(8 lb) ^ b, la + lb), lengths carried mod 2^32 - 1 (the order
// of x divides it).  x^(8 e) for a per-lane e is X0[e & 255] X1[..] X2[..] X3[e >> 24]
// with Xk[b] = x^(8 b 2^(8k)), four 256-entry tables each workgroup builds in LDS by
// doubling from the 32 constants x^(8 2^k).  A thread folds `run` consecutive payloads,
// the workgroup scans the thread lengths into suffix sums, multiplies each thread value
// by x^(8 suffix) and XORs; the partial (value, length) pairs are payloads again, so the
// second launch is the same kernel on one workgroup.
//
// The buffer call composes the braided kernel (wtp_crc32_batch_fixed over the 16-B aligned
// interior in 1456-B chunks) with k_concat_fold; the misaligned head (<= 15 B) and the
// tail (< 1456 B) are hashed by two extra workgroups of the first fold launch (a byte run
// per thread from a zero register, then the same uniform tree), so a misaligned base costs
// nothing but them.
//
// All scratch is the caller's d_work; nothing is allocated, no state is kept, every word
// of d_work that is read was written earlier in the same call.  A separate translation
// unit: see wtp_common.hpp.
#include <algorithm>

#include "crc32_combine.hpp"
#include "wtp_common.hpp"

namespace wtp {
namespace dev {

constexpr uint32_t kCcThreads = 256;    // one workgroup; the tree below has log2 = 8 levels
constexpr uint32_t kCcLevels = 8;
constexpr uint32_t kCcMaxGroups = 1024; // partials of a first launch (d_work holds them)
constexpr uint32_t kCcRun = 16;         // CRCs per thread while fewer than kCcMaxGroups groups are needed

// d_work, in 32-bit words: partial values, partial lengths (var), the two edge CRCs
constexpr uint32_t kCcWorkLen = kCcMaxGroups;
constexpr uint32_t kCcWorkEdge = 2 * kCcMaxGroups;
constexpr size_t kCcWorkBytes = 16384;
static_assert((kCcWorkEdge + 2) * 4 <= kCcWorkBytes && kCcWorkBytes <= 65536, "work buffer");
static_assert(kCcThreads == 1u << kCcLevels, "tree levels");

// Uniform-length elements src[0 .. n): thread (group, t) folds the `run` virtual elements
// from (group * 256 + t) * run on, virtual v = real index + pad.
struct FoldArgs {
    const uint32_t *src;
    uint64_t n, pad, run;
    uint32_t groups;
    uint32_t m;                  // x^(8 len)
    uint32_t lv[kCcLevels][32];  // the chain of m^(run 2^j): lv[j][i] = m^(run 2^j) x^i
};

// One edge of the buffer call: bytes p[0 .. len), a run of `run` bytes per thread, `pad`
// virtual zero bytes in front (256 * run = pad + len).
struct EdgeArgs {
    const uint8_t *p;
    uint32_t len, pad, run;
    uint32_t lv[kCcLevels];  // x^(8 run 2^j)
    uint32_t initc;          // crc32(M) = R_0(M) ^ initc for |M| = len
};

static_assert(sizeof(FoldArgs) + 2 * sizeof(EdgeArgs) <= 2048, "kernel arguments");

// What the last launch adds to the folded body B: B * mlast ^ *last ^ *head * mhead.
struct FinalArgs {
    const uint32_t *last, *head;  // either may be NULL (term absent)
    uint32_t mlast, mhead;
    uint32_t *out;                // NULL: not the last launch
};

// a * c for a uniform c.  Plain: the 32-step loop, the chain c x^i running on the scalar unit
// between the vector steps (7 to 8 instructions a step).  Chain: the same with the chain
// computed on the host and read from the kernel arguments (3 instructions a step); the
// workgroup tree of the CRC fold, eight dependent multiplications per launch, uses it.
struct PlainConst {
    uint32_t c;
    __device__ __forceinline__ uint32_t times(uint32_t a) const { return gf::mul(a, c); }
};
struct ChainConst {
    const uint32_t (&ch)[32];
    __device__ __forceinline__ uint32_t times(uint32_t a) const {
        uint32_t p = 0;
#pragma unroll
        for (uint32_t i = 0; i < 32; ++i) p ^= (0u - ((a >> (31 - i)) & 1u)) & ch[i];
        return p;
    }
};
__device__ __forceinline__ PlainConst level_const(const uint32_t (&lv)[kCcLevels], uint32_t j) { return {lv[j]}; }
__device__ __forceinline__ ChainConst level_const(const uint32_t (&lv)[kCcLevels][32], uint32_t j) { return {lv[j]}; }

// Thread t holds a; thread t's elements precede thread t+1's.  Level j folds blocks of 2^j
// threads pairwise: left * (level j's constant) ^ right.  Every thread reaches every barrier.
template <class Levels>
__device__ __forceinline__ uint32_t wg_fold(uint32_t a, const Levels &lv, uint32_t *s) {
    const uint32_t t = threadIdx.x;
    s[t] = a;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kCcLevels; ++j) {
        const uint32_t h = 1u << j;
        if ((t & (2 * h - 1)) == 0) s[t] = level_const(lv, j).times(s[t]) ^ s[t + h];
        __syncthreads();
    }
    return s[0];
}

// The byte-table operator of a uniform constant c: tab[256 k + b] = (b << 8k) * c.  One pass
// over the chain c x^i (step i is the image of input bit 31 - i) fills a thread's four
// entries, so the build costs one multiplication, not four.
__device__ __forceinline__ void build_operator(uint32_t *tab, uint32_t c) {
    const uint32_t t = threadIdx.x;
    uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 32; ++i) {
        const uint32_t bit = 31 - i;
        r[bit >> 3] ^= (0u - ((t >> (bit & 7u)) & 1u)) & c;
        c = (c >> 1) ^ ((0u - (c & 1u)) & gf::kP);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tab[256 * k + t] = r[k];
}

constexpr uint32_t kCcBatch = 16;    // CRCs a thread has in flight before it folds them
constexpr uint32_t kCcEdgeBytes = 8; // bytes per thread of an edge, all loaded up front
static_assert((WTP_MAX_PAYLOAD - 1 + kCcThreads - 1) / kCcThreads <= kCcEdgeBytes, "edge run");

__global__ void __launch_bounds__(kCcThreads)
k_concat_fold(const FoldArgs f, const EdgeArgs e0, const EdgeArgs e1, uint32_t *work, const FinalArgs fin) {
    __shared__ uint32_t tab[1024];
    __shared__ uint32_t s[kCcThreads];
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    if (g < f.groups) {  // block-uniform
        const uint64_t v0 = (uint64_t(g) * kCcThreads + t) * f.run;
        uint32_t acc = 0;
        if (f.run == 1) {  // uniform: nothing to multiply, no table (the fold of <= 256 partials)
            acc = v0 >= f.pad ? f.src[v0 - f.pad] : 0u;
        } else {
            build_operator(tab, f.m);
            __syncthreads();
            // a batch of loads is in flight at once: one memory latency per 16 CRCs, not 16
            for (uint64_t b = 0; b < f.run; b += kCcBatch) {
                uint32_t c[kCcBatch];
#pragma unroll
                for (uint32_t k = 0; k < kCcBatch; ++k) {
                    const uint64_t v = v0 + b + k;
                    c[k] = b + k < f.run && v >= f.pad ? f.src[v - f.pad] : 0u;  // v - pad < n
                }
#pragma unroll
                for (uint32_t k = 0; k < kCcBatch; ++k)
                    if (b + k < f.run)  // uniform
                        acc = tab[acc & 255u] ^ tab[256 + ((acc >> 8) & 255u)] ^ tab[512 + ((acc >> 16) & 255u)] ^
                              tab[768 + (acc >> 24)] ^ c[k];
            }
        }
        const uint32_t body = wg_fold(acc, f.lv, s);
        if (t == 0) {
            if (fin.out) {
                uint32_t r = fin.mlast == gf::kOne ? body : gf::mul(body, fin.mlast);
                if (fin.last) r ^= *fin.last;
                if (fin.head) r ^= gf::mul(*fin.head, fin.mhead);
                *fin.out = r;
            } else {
                work[g] = body;
            }
        }
    } else {
        const EdgeArgs &e = g == f.groups ? e0 : e1;
        const uint32_t v0 = t * e.run;
        uint32_t byte[kCcEdgeBytes];
#pragma unroll
        for (uint32_t k = 0; k < kCcEdgeBytes; ++k) {
            const uint32_t v = v0 + k;
            byte[k] = k < e.run && v >= e.pad ? uint32_t(e.p[v - e.pad]) : 0u;  // v - pad < len
        }
        uint32_t reg = 0;
#pragma unroll
        for (uint32_t k = 0; k < kCcEdgeBytes; ++k) {
            if (k < e.run) {  // uniform
                reg ^= byte[k];
#pragma unroll
                for (int b = 0; b < 8; ++b) reg = (reg >> 1) ^ ((0u - (reg & 1u)) & gf::kP);
            }
        }
        const uint32_t raw = wg_fold(reg, e.lv, s);
        if (t == 0) work[kCcWorkEdge + (g - f.groups)] = raw ^ e.initc;
    }
}

// a * x^(8 e), e per lane, from the four byte tables of powers
__device__ __forceinline__ uint32_t mul_pow8(uint32_t a, uint32_t e, const uint32_t *X) {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b = (e >> (8 * k)) & 255u;
        if (b) a = gf::mul(a, X[256 * k + b]);
    }
    return a;
}

__global__ void __launch_bounds__(kCcThreads)
k_concat_var(const uint32_t *crc, const uint32_t *len, uint64_t n, uint64_t run,
             const gf::Pow8 pw, uint32_t *pcrc, uint32_t *plen, uint32_t *out) {
    __shared__ uint32_t X[1024];
    __shared__ uint32_t s[kCcThreads];
    __shared__ uint64_t sl[kCcThreads];
    const uint32_t t = threadIdx.x;
    {  // Xk[b] = prod over the set bits j of b of x^(8 2^(8k + j)): wave k builds table k by doubling
        const uint32_t k = __builtin_amdgcn_readfirstlane(t >> 6), r = t & 63u;
        if (r == 0) X[256 * k] = gf::kOne;
        __syncthreads();
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t h = 1u << j, gj = pw.v[8 * k + j];
            for (uint32_t q = r; q < h; q += 64) X[256 * k + h + q] = gf::mul(X[256 * k + q], gj);
            __syncthreads();
        }
    }
    const uint64_t i0 = (uint64_t(blockIdx.x) * kCcThreads + t) * run;
    uint32_t acc = 0;
    uint64_t L = 0;
    for (uint64_t e = 0; e < run; ++e) {
        const uint64_t i = i0 + e;
        if (i < n) {
            const uint32_t l = len[i];
            acc = mul_pow8(acc, l, X) ^ crc[i];
            L += l;
            if (L >> 63) L %= gf::kOrder;
        }
    }
    // suffix sums of the thread lengths (each < 2^32 after the reduction: no overflow)
    const uint64_t mine = L % gf::kOrder;
    sl[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < kCcThreads; d <<= 1) {
        const uint64_t v = t + d < kCcThreads ? sl[t + d] : 0;
        __syncthreads();
        sl[t] += v;
        __syncthreads();
    }
    s[t] = mul_pow8(acc, uint32_t((sl[t] - mine) % gf::kOrder), X);
    __syncthreads();
    for (uint32_t h = kCcThreads / 2; h > 0; h >>= 1) {
        if (t < h) s[t] ^= s[t + h];
        __syncthreads();
    }
    if (t == 0) {
        if (out) {
            *out = s[0];
        } else {
            pcrc[blockIdx.x] = s[0];
            plen[blockIdx.x] = uint32_t(sl[0] % gf::kOrder);
        }
    }
}

}  // namespace dev
}  // namespace wtp

namespace {

using namespace wtp;

uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// x^(8 * len * count) for a reduced len
uint32_t xpow8_times(uint32_t len_r, uint64_t count) { return gf::xpow8(uint64_t(len_r) * gf::reduce(count)); }

// Grid of a fold over n uniform elements of (reduced) length len_r each.
dev::FoldArgs plan_fold(const uint32_t *src, uint64_t n, uint32_t len_r) {
    dev::FoldArgs f{};
    f.src = src;
    f.n = n;
    if (n <= uint64_t(dev::kCcThreads) * dev::kCcRun) {
        f.run = std::max<uint64_t>(1, ceil_div(n, dev::kCcThreads));
        f.groups = 1;
    } else {
        f.run = std::max<uint64_t>(dev::kCcRun, ceil_div(n, uint64_t(dev::kCcThreads) * dev::kCcMaxGroups));
        f.groups = uint32_t(ceil_div(n, dev::kCcThreads * f.run));
    }
    f.pad = uint64_t(f.groups) * dev::kCcThreads * f.run - n;
    f.m = gf::xpow8(len_r);
    for (uint32_t j = 0; j < dev::kCcLevels; ++j) {
        uint32_t c = xpow8_times(len_r, f.run << j);
        for (uint32_t i = 0; i < 32; ++i) {
            f.lv[j][i] = c;
            c = (c >> 1) ^ ((0u - (c & 1u)) & gf::kP);
        }
    }
    return f;
}

dev::EdgeArgs plan_edge(const uint8_t *p, uint32_t len) {
    dev::EdgeArgs e{};
    e.p = p;
    e.len = len;
    e.run = uint32_t(std::max<uint64_t>(1, ceil_div(len, dev::kCcThreads)));
    e.pad = dev::kCcThreads * e.run - len;
    for (uint32_t j = 0; j < dev::kCcLevels; ++j) e.lv[j] = gf::xpow8(uint64_t(e.run) << j);
    e.initc = gf::mul(0xFFFFFFFFu, gf::xpow8(len)) ^ 0xFFFFFFFFu;
    return e;
}

// body = fold of src[0 .. n) (uniform reduced length len_r), then fin; edges, if any, are
// hashed by extra workgroups of the first launch into work[kCcWorkEdge ..].
int launch_fold(const uint32_t *src, uint64_t n, uint32_t len_r, const dev::EdgeArgs *edges, uint32_t nedge,
                uint32_t *work, const dev::FinalArgs &fin, hipStream_t st) {
    const dev::FoldArgs f = plan_fold(src, n, len_r);
    const dev::EdgeArgs none{};
    const dev::EdgeArgs &e0 = nedge > 0 ? edges[0] : none, &e1 = nedge > 1 ? edges[1] : none;
    if (f.groups == 1 && nedge == 0)
        return launch("k_concat_fold", dev::k_concat_fold, dim3(1), dim3(dev::kCcThreads), st, f, none, none, work, fin);
    int rc = launch("k_concat_fold", dev::k_concat_fold, dim3(f.groups + nedge), dim3(dev::kCcThreads), st, f, e0, e1, work,
                    dev::FinalArgs{});
    if (rc) return rc;
    // the partials: f.groups elements of 256 * run payloads each
    const uint32_t len2 = gf::reduce(uint64_t(len_r) * gf::reduce(dev::kCcThreads * f.run));
    const dev::FoldArgs f2 = plan_fold(work, f.groups, len2);  // <= 1024 elements: one workgroup
    return launch("k_concat_fold", dev::k_concat_fold, dim3(1), dim3(dev::kCcThreads), st, f2, none, none, work, fin);
}

int check_work(const void *d_work, size_t work_bytes, size_t need) {
    if (work_bytes < need) return fail(WTP_EINVAL, "work_bytes %zu < %zu required", work_bytes, need);
    if (need && !d_work) return fail(WTP_EINVAL, "d_work is null");
    return WTP_OK;
}

}  // namespace

extern "C" size_t wtp_crc32_concat_work_bytes(size_t) { return wtp::dev::kCcWorkBytes; }

extern "C" size_t wtp_crc32_buffer_work_bytes(size_t nbytes) {
    return wtp::dev::kCcWorkBytes + 4 * (nbytes / WTP_MAX_PAYLOAD + (nbytes % WTP_MAX_PAYLOAD != 0));
}

extern "C" int wtp_crc32_concat(const uint32_t *d_crc, const uint32_t *d_len, uint64_t len, uint64_t last_len, size_t n,
                                void *d_work, size_t work_bytes, uint32_t *d_out, void *stream) {
    if (!d_out) return fail(WTP_EINVAL, "d_out is null");
    if (n > 0 && !d_crc) return fail(WTP_EINVAL, "d_crc is null");
    int rc = check_work(d_work, work_bytes, wtp_crc32_concat_work_bytes(n));
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {  // the empty message
        hipError_t e = hipMemsetAsync(d_out, 0, 4, st);
        if (e != hipSuccess) return fail(WTP_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        return WTP_OK;
    }
    uint32_t *work = static_cast<uint32_t *>(d_work);
    if (!d_len) {
        dev::FinalArgs fin{};
        fin.last = d_crc + (n - 1);
        fin.mlast = gf::xpow8(last_len);
        fin.out = d_out;
        return launch_fold(d_crc, n - 1, gf::reduce(len), nullptr, 0, work, fin, st);
    }
    const gf::Pow8 pw{};
    uint64_t run = std::max<uint64_t>(1, ceil_div(n, dev::kCcThreads));
    uint32_t groups = 1;
    if (run > dev::kCcRun) {
        run = std::max<uint64_t>(dev::kCcRun, ceil_div(n, uint64_t(dev::kCcThreads) * dev::kCcMaxGroups));
        groups = uint32_t(ceil_div(n, dev::kCcThreads * run));
    }
    if (groups == 1)
        return launch("k_concat_var", dev::k_concat_var, dim3(1), dim3(dev::kCcThreads), st, d_crc, d_len, uint64_t(n), run, pw,
                      work, work + dev::kCcWorkLen, d_out);
    rc = launch("k_concat_var", dev::k_concat_var, dim3(groups), dim3(dev::kCcThreads), st, d_crc, d_len, uint64_t(n), run, pw,
                work, work + dev::kCcWorkLen, static_cast<uint32_t *>(nullptr));
    if (rc) return rc;
    return launch("k_concat_var", dev::k_concat_var, dim3(1), dim3(dev::kCcThreads), st, static_cast<const uint32_t *>(work),
                  static_cast<const uint32_t *>(work + dev::kCcWorkLen), uint64_t(groups), ceil_div(groups, dev::kCcThreads),
                  pw, work, work + dev::kCcWorkLen, d_out);
}

extern "C" int wtp_crc32_buffer(const void *d_buf, size_t nbytes, void *d_work, size_t work_bytes, uint32_t *d_out,
                                void *stream) {
    if (!d_out) return fail(WTP_EINVAL, "d_out is null");
    if (nbytes > 0 && !d_buf) return fail(WTP_EINVAL, "d_buf is null");
    int rc = check_work(d_work, work_bytes, wtp_crc32_buffer_work_bytes(nbytes));
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nbytes == 0) {
        hipError_t e = hipMemsetAsync(d_out, 0, 4, st);
        if (e != hipSuccess) return fail(WTP_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        return WTP_OK;
    }
    // head (to the first 16-B boundary) | nfull chunks of 1456 B | tail
    const uint8_t *p = static_cast<const uint8_t *>(d_buf);
    const uint64_t head = std::min<uint64_t>(nbytes, (16 - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
    const uint64_t nfull = (nbytes - head) / WTP_MAX_PAYLOAD;
    const uint64_t tail = nbytes - head - nfull * WTP_MAX_PAYLOAD;
    uint32_t *work = static_cast<uint32_t *>(d_work);
    uint32_t *crcs = work + dev::kCcWorkBytes / 4;  // nfull <= ceil(nbytes / 1456) words
    if (nfull > 0) {
        rc = wtp_crc32_batch_fixed(p + head, WTP_MAX_PAYLOAD, WTP_MAX_PAYLOAD, nfull, crcs, stream);
        if (rc) return rc;
    }
    dev::EdgeArgs edges[2];
    uint32_t nedge = 0;
    dev::FinalArgs fin{};
    fin.mlast = gf::xpow8(tail);
    fin.out = d_out;
    if (head) {
        fin.head = work + dev::kCcWorkEdge + nedge;
        fin.mhead = gf::xpow8(nbytes - head);
        edges[nedge++] = plan_edge(p, uint32_t(head));
    }
    if (tail) {
        fin.last = work + dev::kCcWorkEdge + nedge;
        edges[nedge++] = plan_edge(p + head + nfull * WTP_MAX_PAYLOAD, uint32_t(tail));
    }
    return launch_fold(crcs, nfull, gf::reduce(WTP_MAX_PAYLOAD), edges, nedge, work, fin, st);
}
