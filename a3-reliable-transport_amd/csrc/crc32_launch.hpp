// crc32_launch.hpp — the host side of crc32_kernels.hip: error and kernel-name state,
// the per-device state (DevState, host_tables, init_device, stream_scratch), the launchers
// (launch_fixed_braid, launch_pieces, launch_stream, launch_packed_ranges), and the
// metadata providers the C-ABI entry points hand to k_pieces (FixedProvL, ArrayProvL,
// RangeArrayProvL with k_cut_ranges, DgramProvL).  A part of the one translation unit
// crc32_kernels.hip, included there last, before the C-ABI entry points; not a header for
// other units.
#pragma once

namespace wtp {

// ------------------------------------------------------------------------------------
// host side: per-device state, error handling, launchers
// ------------------------------------------------------------------------------------
namespace {

thread_local std::string g_err;
thread_local std::string g_kernel;  // wtp_last_kernel(): the calling thread's last launch

void note_kernel(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void note_kernel(const char *fmt, ...) {
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_kernel = buf;
}

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define WTP_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail(WTP_EHIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr size_t kStreamScratch = 32768;  // launch_packed_ranges' descriptors (one call)
constexpr unsigned kCaptureSlots = 64;     // descriptor buffers for calls captured into graphs
struct DevState {
    std::once_flag once;
    int rc = WTP_OK;
    std::string err;
    uint32_t *tabs = nullptr;
    uint32_t *status = nullptr;
    int cus = 0;
    std::atomic<int> reserve{0};  // CUs left free of the persistent kernels (wtp_reserve_cus)
    unsigned grid_cus() const { return unsigned(std::max(1, cus - reserve.load(std::memory_order_relaxed))); }
    hipMemPool_t pool = nullptr;  // library-owned stream-ordered pool, never trimmed (builder scratch)
    // Device scratch of fixed size for launch_packed_ranges' descriptors.  Outside graph
    // capture: one buffer per stream, made on the stream's first use and kept (calls on one
    // stream are ordered, so they may share it).  During capture: a slot of `cap`, taken
    // by that one captured call for the life of the process, so two graphs captured on one
    // stream (torch's shared capture stream) never share descriptors when replayed at
    // once; with every slot taken, a captured call takes k_stream instead (exact, no
    // scratch).  Both kinds are plain hipMalloc memory made outside any capture, so a graph
    // bakes in a buffer that outlives it.  (Stream-ordered pool allocations inside a
    // capture replayed wrongly when one graph held several calls: the sub-launches read
    // zeroed descriptors and did nothing; profiles/r05)
    std::mutex smu;
    std::unordered_map<hipStream_t, void *> sbuf;
    uint8_t *cap = nullptr;  // kCaptureSlots x kStreamScratch, made at init
    unsigned cap_used = 0;
};
constexpr int kMaxDev = 64;
DevState g_dev[kMaxDev];

std::vector<uint32_t> host_tables() {
    std::vector<uint32_t> t(TAB_WORDS, 0);
    make_word_tables(&t[OFF_BRAID], kBraidBlock);
    const uint32_t inv_bytes[6] = {4, 8, 16, 32, 64, 128};
    for (int o = 0; o < 6; ++o)
        make_operator(&t[OFF_INV + 1024 * o], [&](uint32_t v) { return unshift_bytes(v, inv_bytes[o]); });
    make_word_tables(&t[OFF_S4], 4);
    for (int o = 0; o < 6; ++o) {
        const uint64_t nb = uint64_t(kPieceS) << o;
        make_operator(&t[OFF_FWD + 1024 * o], [&](uint32_t v) { return shift_bytes(v, nb); });
    }
    for (uint32_t h = 0; h <= uint32_t(kPieceS); ++h) t[OFF_HINIT + h] = shift_bytes(0xFFFFFFFFu, h);
    make_operator(&t[OFF_T256], [](uint32_t v) { return shift_bytes(v, 32); });
    auto nib = [&](uint32_t op, uint64_t nbytes) {
        for (uint32_t i = 0; i < 8; ++i)
            for (uint32_t e = 0; e < 16; ++e) t[OFF_NIB + 128 * op + 16 * i + e] = shift_bytes(e << (4 * i), nbytes);
    };
    for (uint32_t k = 0; k < 6; ++k) nib(k, uint64_t(128) << k);
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t j = 0; j < 8; ++j) nib(6 + 8 * k + j, uint64_t(j) << (3 * k));
    return t;
}

int init_device(int dev) {
    if (dev < 0 || dev >= kMaxDev) return fail(WTP_EINVAL, "device %d out of range", dev);
    DevState &s = g_dev[dev];
    std::call_once(s.once, [&] {
        auto setfail = [&](int code, const std::string &m) {
            s.rc = code;
            s.err = m;
        };
        int prev = 0;
        (void)hipGetDevice(&prev);
        auto setup = [&]() {
            if (hipSetDevice(dev) != hipSuccess) return setfail(WTP_ENODEV, "hipSetDevice failed");
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return setfail(WTP_ENODEV, "hipGetDeviceProperties failed");
            if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
                return setfail(WTP_ENODEV, std::string("device is ") + prop.gcnArchName + ", library built for gfx950");
            s.cus = prop.multiProcessorCount;
            std::vector<uint32_t> t = host_tables();
            if (hipMalloc(&s.tabs, t.size() * 4) != hipSuccess) return setfail(WTP_ENOMEM, "hipMalloc(tables) failed");
            if (hipMemcpy(s.tabs, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
                return setfail(WTP_EHIP, "hipMemcpy(tables) failed");
            if (hipMalloc(&s.status, 4) != hipSuccess) return setfail(WTP_ENOMEM, "hipMalloc(status) failed");
            if (hipMemset(s.status, 0, 4) != hipSuccess) return setfail(WTP_EHIP, "hipMemset(status) failed");
            // Scratch of async entry points (the builder's CRCs on its slow path) comes from a
            // library-owned pool whose memory is kept across calls (release threshold max):
            // the default threshold returns it at every synchronisation, and re-mapping it
            // cost ~1 ms per small host-verify call.
            hipMemPoolProps pp{};
            pp.allocType = hipMemAllocationTypePinned;
            pp.location.type = hipMemLocationTypeDevice;
            pp.location.id = dev;
            if (hipMalloc(&s.cap, kCaptureSlots * kStreamScratch) != hipSuccess)
                return setfail(WTP_ENOMEM, "hipMalloc(capture scratch) failed");
            if (hipMemPoolCreate(&s.pool, &pp) != hipSuccess) return setfail(WTP_EHIP, "hipMemPoolCreate failed");
            uint64_t keep = UINT64_MAX;
            if (hipMemPoolSetAttribute(s.pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess)
                return setfail(WTP_EHIP, "hipMemPoolSetAttribute failed");
        };
        setup();
        (void)hipSetDevice(prev);  // the caller's current device, on success and on failure
        (void)hipGetLastError();
    });
    if (s.rc != WTP_OK) return fail(s.rc, "wtp init(device %d): %s", dev, s.err.c_str());
    return WTP_OK;
}

int current(DevState *&s) {
    int dev = 0;
    WTP_HIP(hipGetDevice(&dev));
    int rc = init_device(dev);
    if (rc) return rc;
    s = &g_dev[dev];
    return WTP_OK;
}

// Descriptor scratch (kStreamScratch bytes) for one launch_packed_ranges call on `st`
// (DevState::sbuf / cap).  *out = nullptr: the call is being captured and every capture
// slot is taken; the caller then takes the scratch-free k_stream route.
int stream_scratch(DevState &s, hipStream_t st, void **out) {
    std::lock_guard<std::mutex> g(s.smu);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    WTP_HIP(hipStreamIsCapturing(st, &cs));
    if (cs != hipStreamCaptureStatusNone) {
        *out = s.cap_used < kCaptureSlots ? s.cap + kStreamScratch * s.cap_used++ : nullptr;
        return WTP_OK;
    }
    auto it = s.sbuf.find(st);
    if (it != s.sbuf.end()) {
        *out = it->second;
        return WTP_OK;
    }
    void *p = nullptr;
    WTP_HIP(hipMalloc(&p, kStreamScratch));
    s.sbuf.emplace(st, p);
    *out = p;
    return WTP_OK;
}

int launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WTP_EHIP, "launch %s: %s", what, hipGetErrorString(e));
    return WTP_OK;
}

// Workgroup size of the braided kernel (one workgroup per CU: its LDS tables take the
// CU's 160 KiB).  Interleaved A/B on one box (profiles/r01i/ab_braid_threads.txt):
//   CRC / verify, 1 M x 1456 B: 1024 threads 0.2325 ms, 768 0.2334, 640 0.2286,
//     576 0.2271, 512 0.2219 (86% of HBM peak), 448 0.2289, 384 0.2353, 256 0.2720;
//   fused builder (reads + wire writes): 1024 0.769 ms, 512 0.745, 256 0.680,
//     192 0.667, 128 0.653, 64 1.052.
// Fewer waves per CU keep fewer rows in flight; HBM serves the stream with less
// queueing (and, for the builder, fewer read/write turnarounds) while 8 resp. 2 waves,
// two rounds each, still cover its latency.
// (the sizes are each epilogue's kThreads: CrcBEpi and VerifyBEpi 512, BuildBEpi 128)
static_assert(dev::VerifyBEpi::kThreads == dev::CrcBEpi::kThreads, "one braided grid rule");
static_assert(dev::VerifyBEpi::kThreads == 64 * dev::kVfWaves, "verify fix-up LDS layout");

template <int ROWS, class BEpi>
void launch_braid_rows(dim3 grid, unsigned threads, hipStream_t st, const uint8_t *b, uint64_t stride, uint32_t len,
                       uint64_t n, BEpi epi, const uint32_t *tabs) {
    note_kernel("k_fixed_braid<%d, %d, %s>", ROWS, BEpi::kDiag, BEpi::kName);
    hipLaunchKernelGGL((dev::k_fixed_braid<ROWS, BEpi::kDiag, BEpi>), grid, dim3(threads), 0, st, b,
                       uint32_t(stride), len, n, epi, tabs);
}

template <class BEpi>
int launch_fixed_braid_rows(DevState &s, const uint8_t *base, uint64_t stride, uint32_t len, uint64_t n, BEpi epi,
                            hipStream_t st, unsigned grid, unsigned threads, int rows) {
    switch (rows) {
        case 1: launch_braid_rows<1>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        case 2: launch_braid_rows<2>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        case 3: launch_braid_rows<3>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        case 4: launch_braid_rows<4>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        case 5: launch_braid_rows<5>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        case 6: launch_braid_rows<6>(grid, threads, st, base, stride, len, n, epi, s.tabs); break;
        default: return fail(WTP_EINVAL, "braid rows %d", rows);
    }
    return launch_check("k_fixed_braid");
}

constexpr uint64_t kHoldRounds = 64;  // rounds per wave from which the CRC holds its results (CrcHoldBEpi)

// Braided kernel over n packets base[p*stride, +len): base, stride, len multiples of 16,
// 16 <= len <= 1536, stride <= 16 KiB.  The epilogue's cinit is filled in here.
template <class BEpi>
int launch_fixed_braid(DevState &s, const uint8_t *base, uint64_t stride, uint32_t len, uint64_t n, BEpi epi,
                       hipStream_t st) {
    const int rows = int((len + 255) / 256);
    const unsigned threads = BEpi::kThreads;
    const uint64_t rounds = (n + 3) / 4;
    const uint64_t want = (rounds + threads / 64 - 1) / (threads / 64);
    uint64_t cap = s.grid_cus();
    // Long streaming batches (>= 64 rounds per wave) run one workgroup per XCD fewer than
    // CUs: fewer rows in flight queue less at HBM.  Interleaved A/B, 8 reps
    // (profiles/r02h/ab_reserve2.log): 1 M x 1456 B 220.6 us at 256 workgroups, 218.7 at
    // 252, 217.4 at 248, 217.5-217.7 at 244-232; 2 M 460.6 vs 452.2 us at 248.  Short
    // batches keep every CU (C2: 8 rounds per wave, a ninth would be its tail).
    if (!BEpi::kCopy && s.reserve.load(std::memory_order_relaxed) == 0 && rounds >= 64 * cap * (threads / 64))
        cap -= cap / 32;
    const unsigned grid = unsigned(want < cap ? want : cap);
    epi.cinit = init_const(len);
    if constexpr (std::is_same_v<BEpi, dev::CrcBEpi>) {
        // long batches hold their results in LDS (k_fixed_braid, kDump): short ones store
        // directly, the held form's code was 1.4-1.7% slower on 16 K-64 K packets even with
        // nothing held (profiles/r04u).  The held form's bursts are 16-B stores at
        // out + 16 k: only a 16-B aligned `out` takes it (a torch slice out[1:] is only
        // 4-B aligned; it keeps the direct dword stores).
        if (rounds >= kHoldRounds * grid * (threads / 64) &&
            (reinterpret_cast<uintptr_t>(epi.out) & 15u) == 0) {
            dev::CrcHoldBEpi h;
            static_cast<dev::CrcBEpi &>(h) = epi;
            return launch_fixed_braid_rows(s, base, stride, len, n, h, st, grid, threads, rows);
        }
    }
    return launch_fixed_braid_rows(s, base, stride, len, n, epi, st, grid, threads, rows);
}

template <class Prov, class Epi>
int launch_pieces(DevState &s, const uint8_t *base, uint64_t nbytes, Prov prov, uint64_t n, Epi epi,
                  hipStream_t st) {
    // Align the buffer view down to 16 B and round its size up: every 16-B block holding
    // a valid byte is then fully inside the resource (and inside one page).
    const uintptr_t ub = reinterpret_cast<uintptr_t>(base);
    const uint64_t lead = ub & 15u;
    const uint8_t *b16 = base - lead;
    const uint64_t span = (lead + nbytes + 15) & ~uint64_t(15);
    if (span >= (1ull << 31)) return fail(WTP_EINVAL, "general kernel span %llu B >= 2 GiB (split the batch)", (unsigned long long)span);
    const uint64_t waves_want = (n + 63) / 64;
    uint64_t grid = (waves_want + dev::kPcThreads / 64 - 1) / (dev::kPcThreads / 64);
    if (grid > uint64_t(s.grid_cus())) grid = uint64_t(s.grid_cus());
    if (grid == 0) grid = 1;
    note_kernel("k_pieces<%s, %s>", Prov::kName, Epi::kName);
    hipLaunchKernelGGL((dev::k_pieces<Prov, Epi>), dim3(unsigned(grid)), dim3(dev::kPcThreads), 0, st, b16, uint32_t(span),
                       prov, n, epi, s.tabs, s.status);
    return launch_check("k_pieces");
}

// Packed mixed lengths (k_stream): one launch for any n and any buffer size (64-bit
// offsets, per-round buffer resources); the kernel finds its own workgroup ranges.
int launch_stream(DevState &s, const uint8_t *base, uint64_t nbytes, const uint64_t *offs, const uint32_t *lens,
                  uint64_t n, uint32_t *out, hipStream_t st, const dev::RangeDesc *gate = nullptr, uint32_t ngate = 0) {
    const uint64_t lead = reinterpret_cast<uintptr_t>(base) & 15u;
    uint64_t grid = (n + dev::kStWaves * 64 - 1) / (dev::kStWaves * 64);  // >= 64 payloads per wave
    if (grid > uint64_t(s.grid_cus())) grid = uint64_t(s.grid_cus());
    if (grid == 0) grid = 1;
    note_kernel("k_stream");
    hipLaunchKernelGGL((dev::k_stream<0>), dim3(unsigned(grid)), dim3(dev::kStThreads), 0, st, base - lead,
                       lead + nbytes, offs, lens, lead, n, out, s.tabs, s.status, gate, ngate);
    return launch_check("k_stream");
}

}  // namespace

// Offsets handed to k_pieces must be relative to the 16-B aligned view.  The providers
// below add `lead` back.
namespace dev {
// Providers split metadata access in two: load() only issues loads (its results are
// consumed a round later, so no arithmetic may touch them there) and decode() turns the
// raw words into (offset in the view, length, valid, aux, output slot) when the round
// uses them.  (The fix-up pass's provider, LdsIdxDgramProv, is in crc32_pieces.hpp.)
struct FixedProvL {
    static constexpr const char *kName = "FixedProvL";  // wtp_last_kernel()
    static constexpr bool kVarLen = false;  // wave ranges balanced by pieces
    static constexpr bool kIndexed = false;
    static constexpr bool kGroupLoad = false;
    uint64_t stride, lead;
    uint32_t len;
    __device__ __forceinline__ void load(uint64_t p, MetaRaw &r, __amdgpu_buffer_rsrc_t) const { r.a = p; }
    __device__ __forceinline__ void decode(const MetaRaw &r, uint64_t &off, uint32_t &l, bool &ok, uint32_t &,
                                           uint32_t &) const {
        off = lead + r.a * stride;
        l = len;
        ok = true;
    }
};
struct ArrayProvL {
    static constexpr const char *kName = "ArrayProvL";  // wtp_last_kernel()
    static constexpr bool kVarLen = true;  // wave ranges balanced by pieces
    static constexpr bool kIndexed = false;
    static constexpr bool kGroupLoad = true;  // load_group: 32-bit buffer offsets, no clamp
    const uint64_t *__restrict__ offs;
    const uint32_t *__restrict__ lens;
    uint64_t lead;
    uint32_t n;  // packets of this launch (< 2^28: the arrays' byte extents fit 32 bits)
    __device__ __forceinline__ void load(uint64_t p, MetaRaw &r, __amdgpu_buffer_rsrc_t) const {
        r.a = reinterpret_cast<const uint32_t *>(offs)[2 * p];  // low dword: the view is < 2 GiB
        r.b = lens[p];
    }
    // packets q0 + lane: one VALU address per array; past n the loads return 0 (the range
    // check covers voffset, so the whole offset goes there, none in soffset)
    __device__ __forceinline__ void load_group(uint64_t q0, uint32_t lane, MetaRaw &r) const {
        const uint32_t pi = uint32_t(q0) + lane;
        r.a = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(offs, n * 8u), int(pi * 8u), 0, 0);
        r.b = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(lens, n * 4u), int(pi * 4u), 0, 0);
    }
    __device__ __forceinline__ const uint32_t *len_array() const { return lens; }
    __device__ __forceinline__ uint32_t len_of(uint32_t w) const { return w; }
    __device__ __forceinline__ void decode(const MetaRaw &r, uint64_t &off, uint32_t &l, bool &ok, uint32_t &,
                                           uint32_t &) const {
        off = lead + r.a;
        l = r.b;
        ok = true;
    }
};
// Packed batches >= 2 GiB (launch_packed_ranges): ArrayProvL over one device-bound
// sub-range of the arrays (RangeDesc), 64-bit offsets rebased onto the sub-launch's
// < 2 GiB view.  A packet outside the view (offsets not packed) is flagged, not read.
struct RangeArrayProvL {
    static constexpr const char *kName = "RangeArrayProvL";  // wtp_last_kernel()
    static constexpr bool kVarLen = true;
    static constexpr bool kIndexed = false;
    static constexpr bool kGroupLoad = true;
    static constexpr bool kDevRange = true;
    const uint64_t *__restrict__ offs;  // the caller's arrays (bind() moves them to the range)
    const uint32_t *__restrict__ lens;
    RangeDesc *desc;
    uint64_t lead;        // the caller's base mod 16
    uint64_t rebase = 0;  // bind(): view offset of this launch's resource base
    uint32_t n = 0, vbytes = 0;
    template <class E>
    __device__ __forceinline__ bool bind(const uint8_t *&base, uint32_t &nbytes, uint64_t &nn, E &e) {
        const uint64_t b = desc->begin, en = desc->end;
        // only the cut-time flag: kRunBad may be set by another workgroup mid-launch, and
        // reading it here could let some waves of a block leave before a barrier
        if (b >= en || (desc->bad & kCutBad)) return false;
        rebase = desc->rebase;
        vbytes = desc->nbytes;
        offs += b;
        lens += b;
        n = uint32_t(en - b);  // <= kSubBatch
        base += rebase;
        nbytes = vbytes;
        nn = en - b;
        e.rebase(b, n);
        return true;
    }
    __device__ __forceinline__ void flag_outside() const { atomicOr(&desc->bad, kRunBad); }
    __device__ __forceinline__ void load(uint64_t p, MetaRaw &r, __amdgpu_buffer_rsrc_t) const {
        r.a = offs[p];
        r.b = lens[p];
    }
    __device__ __forceinline__ void load_group(uint64_t q0, uint32_t lane, MetaRaw &r) const {
        const uint32_t pi = uint32_t(q0) + lane;  // past n: 0
        const u32x2 w = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(make_rsrc(offs, n * 8u),
                                                                                        int(pi * 8u), 0, 0));
        r.a = uint64_t(w.x) | (uint64_t(w.y) << 32);
        r.b = __builtin_amdgcn_raw_buffer_load_b32(make_rsrc(lens, n * 4u), int(pi * 4u), 0, 0);
    }
    __device__ __forceinline__ const uint32_t *len_array() const { return lens; }
    __device__ __forceinline__ uint32_t len_of(uint32_t w) const { return w; }
    __device__ __forceinline__ void decode(const MetaRaw &r, uint64_t &off, uint32_t &l, bool &ok, uint32_t &,
                                           uint32_t &) const {
        const uint64_t o = r.a + lead - rebase;  // offset in this launch's view (mod 2^64)
        const bool in = o <= uint64_t(vbytes) && uint64_t(r.b) <= uint64_t(vbytes) - o;
        off = in ? o : 0u;
        l = in ? r.b : 0u;
        ok = in;
    }
};

// Sub-ranges of a packed batch for launch_packed_ranges: cuts where the view offset
// reaches k * G (binary search over the offsets; a prefix max keeps them monotone for
// any offsets) merged with the count cuts j * sb, so every range holds <= sb packets
// and, if packed, its bytes lie within G + 4 KiB < 2 GiB of its first offset.
constexpr uint32_t kMaxRanges = 1024;
__global__ __launch_bounds__(256) void k_cut_ranges(const uint64_t *__restrict__ offs, uint64_t n, uint64_t lead,
                                                    uint64_t vspan, uint64_t G, uint32_t kb, uint64_t sb,
                                                    RangeDesc *__restrict__ desc, uint32_t nd) {
    __shared__ uint64_t bcut[kMaxRanges];
    __shared__ uint64_t cuts[kMaxRanges + 1];
    for (uint32_t k = threadIdx.x + 1; k < kb; k += blockDim.x) {
        const uint64_t t = uint64_t(k) * G;
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t m = lo + (hi - lo) / 2;
            if (offs[m] + lead < t) lo = m + 1;
            else hi = m;
        }
        bcut[k] = lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t pb = 0, jc = sb;
        uint32_t k = 1, m = 1;
        cuts[0] = 0;
        while (m < nd) {
            const uint64_t b = k < kb ? (bcut[k] > pb ? bcut[k] : pb) : ~0ull;
            const uint64_t c = jc < n ? jc : ~0ull;
            if (b == ~0ull && c == ~0ull) {  // both lists used up (cannot happen for nd = kb + nc - 1): pad
                cuts[m++] = n;
                continue;
            }
            if (b <= c) {
                cuts[m++] = b;
                pb = b;
                ++k;
            } else {
                cuts[m++] = c;
                jc += sb;
            }
        }
        cuts[nd] = n;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nd; j += blockDim.x) {
        RangeDesc d{};
        d.begin = cuts[j];
        d.end = cuts[j + 1] > cuts[j] ? cuts[j + 1] : cuts[j];
        d.nbytes = 16;
        if (d.begin < d.end) {
            const uint64_t r = (offs[d.begin] + lead) & ~uint64_t(15);
            if (r < vspan) {
                d.rebase = r;
                d.nbytes = uint32_t(vspan - r < (1ull << 31) - 16 ? vspan - r : (1ull << 31) - 16);
            } else {
                d.bad = kCutBad;  // an offset past the buffer: not a packed batch
            }
        }
        desc[j] = d;
    }
}

// Datagram p = view[lead + p*stride, +recv_len[p]): header (16 B) + payload.  aux =
// ntohl(header.checksum): the two dwords covering header bytes 12..15 ride with the
// metadata prefetch (through the view's buffer resource: the second dword may lie past
// the last datagram, reads there return 0 and are never selected) and are
// funnel-shifted at decode.
struct DgramProvL {
    static constexpr const char *kName = "DgramProvL";  // wtp_last_kernel()
    static constexpr bool kVarLen = true;  // wave ranges balanced by pieces
    static constexpr bool kIndexed = false;
    static constexpr bool kGroupLoad = false;
    uint64_t stride, lead;
    const uint32_t *__restrict__ rl;
    __device__ __forceinline__ void load(uint64_t p, MetaRaw &r, __amdgpu_buffer_rsrc_t rs) const {
        const uint32_t h = uint32_t(lead + p * stride + 12) & ~3u;  // the view is < 2 GiB
        r.a = p;
        r.b = rl[p];
        const u32x2 w = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, int(h), 0, 0));
        r.c = w.x;
        r.d = w.y;
    }
    __device__ __forceinline__ const uint32_t *len_array() const { return rl; }
    __device__ __forceinline__ uint32_t len_of(uint32_t r) const { return r >= 16 && r <= stride ? r - 16 : 0u; }
    __device__ __forceinline__ void decode(const MetaRaw &r, uint64_t &off, uint32_t &l, bool &ok, uint32_t &want,
                                           uint32_t &) const {
        const uint64_t d = lead + r.a * stride;
        want = bswap32(__builtin_amdgcn_alignbyte(r.d, r.c, uint32_t(d + 12) & 3u));
        off = d + 16;
        ok = r.b >= 16 && r.b <= stride;
        l = ok ? r.b - 16 : 0;
    }
};
}  // namespace dev

namespace {
// Packed mixed lengths in a buffer >= 2 GiB (wtp_crc32_batch_packed): the piece kernel in
// sub-launches over < 2 GiB views instead of k_stream (C5-like data: 43 vs 57 us per 1 M
// packets).  The host knows neither offsets nor lengths, so the cuts are
// made on the device (k_cut_ranges: view offsets at multiples of G, packet counts at
// multiples of kSubBatch) and each k_pieces sub-launch binds its range from its
// descriptor (RangeArrayProvL); the host launches an upper bound of kb + nc - 1 of them
// (empty ones return at once).  Exact for any offsets: a sub-launch that meets a packet
// outside its view flags its descriptor, and the gated k_stream launch at the end then
// recomputes the whole batch (it returns at once otherwise).  Asynchronous on `st`; the
// descriptors live in the stream's scratch (stream_scratch: calls on one stream are
// ordered, so they may share it).
int launch_packed_ranges(DevState &s, const uint8_t *b, uint64_t base_bytes, const uint64_t *offs,
                         const uint32_t *lens, uint64_t n, uint32_t *out, hipStream_t st) {
    const uint64_t lead = reinterpret_cast<uintptr_t>(b) & 15u;
    const uint8_t *view = b - lead;
    const uint64_t vspan = (lead + base_bytes + 15) & ~uint64_t(15);
    constexpr uint64_t G = (1ull << 31) - (1ull << 16);  // packed: a range spans <= G + 4111 B < 2 GiB - 16
    const uint64_t kb = (vspan + G - 1) / G, nc = (n + kSubBatch - 1) / kSubBatch;
    const uint64_t nd = kb + nc - 1;
    if (nd > dev::kMaxRanges) return launch_stream(s, b, base_bytes, offs, lens, n, out, st);
    static_assert(dev::kMaxRanges * sizeof(dev::RangeDesc) <= kStreamScratch, "descriptor scratch");
    dev::RangeDesc *d = nullptr;
    int rc = stream_scratch(s, st, reinterpret_cast<void **>(&d));
    if (rc) return rc;
    if (!d) return launch_stream(s, b, base_bytes, offs, lens, n, out, st);  // captured, no slot left
    hipLaunchKernelGGL(dev::k_cut_ranges, dim3(1), dim3(256), 0, st, offs, n, lead, vspan, G, uint32_t(kb),
                       uint64_t(kSubBatch), d, uint32_t(nd));
    rc = launch_check("k_cut_ranges");
    const uint64_t per = n < kSubBatch ? n : kSubBatch;  // packets of the largest range: the grid
    uint64_t grid = ((per + 63) / 64 + dev::kPcThreads / 64 - 1) / (dev::kPcThreads / 64);
    if (grid > uint64_t(s.grid_cus())) grid = uint64_t(s.grid_cus());
    for (uint64_t j = 0; j < nd && !rc; ++j) {
        hipLaunchKernelGGL((dev::k_pieces<dev::RangeArrayProvL, dev::CrcEpi>), dim3(unsigned(grid)),
                           dim3(dev::kPcThreads), 0, st, view, uint32_t(0),
                           dev::RangeArrayProvL{offs, lens, d + j, lead}, per, dev::CrcEpi{out, 0}, s.tabs, s.status);
        rc = launch_check("k_pieces");
    }
    if (!rc) rc = launch_stream(s, b, base_bytes, offs, lens, n, out, st, d, uint32_t(nd));
    note_kernel("k_pieces<RangeArrayProvL, CrcEpi> x %llu (+ k_stream if not packed)", (unsigned long long)nd);
    return rc;
}
}  // namespace

}  // namespace wtp
