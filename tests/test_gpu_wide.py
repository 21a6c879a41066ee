"""Addressing past 2 GiB and 4 GiB: every device call of include/wtp_crc32.h on a ring, wire
buffer, image or stream whose extent passes 2^32 bytes, with work on both sides of byte
offsets 2^31 and 2^32 measured from the pointer the caller passes.

The extents are large, the work is not.  A ring with a stride near 1 MiB spans 4.3 GB in about
4100 entries; a ring of the braided paths (stride <= 16384) takes 262,209 entries or more, gathered
on the device from a small pool of datagrams or chunks made on the host.  Expected values come
from the oracle on the pool and numpy / torch arithmetic per index (ok[i] = pool_ok[idx[i]]), or
from the tests' sequential models run on a compact host copy of the same entries (the same bytes
in slots of 1504 or 1472 bytes): never from a library call.  Every output buffer starts from a
sentinel and is compared whole, on the device in pieces of at most 512 MiB where it is large:
slot tails, entries past the count, the bytes behind the last slot and the bytes just below
2^31 and 2^32 that belong to no entry keep the sentinel.  Each test asserts its own boundary
conditions (gpu_support.assert_straddles): an entry that ends within one stride below each
boundary, one that begins at or above it and, where the stride can be chosen, one that
contains it."""
import time

import numpy as np
import pytest

import accept_model
import ack_model
import buildvar_model
import deliver_model
import flows_flush_model as FM
import flows_model as F
import oracle as O
import retx_model as R
import retxvar_model
from gpu_support import (BOUNDS, GUARD_WORD, MAXP, ODD_STRIDE, PIECE, WIDE_N, WIDE_STRIDE, Batch, Bytes, DevWindow, SparseRing, W, Words,  # noqa: F401
                         assert_filled, assert_no_data_error, assert_straddles, be_words, dev_s32, periodic, periodic_crc, s32,
                         slots, straddling_stride, torch, u32)

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF
FILL = 0xEE          # the sentinel of every large buffer
CW = 1504            # slot of the compact host copy of a datagram ring: the longest datagram is 1500 bytes
DW = 16 + MAXP       # 1472, the longest DATA datagram a builder writes
BRAID_STRIDE = 16384  # the largest stride of the braided paths
BRAID_N = (1 << 32) // BRAID_STRIDE + 1 + 155  # 262,300 >= 262,145 + 64 slots: the ring ends 2.5 MB past 2^32
GIB = 1 << 30
LIMIT = 16 * GIB     # no test holds more device memory than this


@pytest.fixture(autouse=True)
def accounted(request):
    """Peak device memory and wall time of every test, printed for the record and held to the
    limit; the cache is emptied so that the next test starts from nothing."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"\nWIDE {request.node.name}: peak {peak / GIB:.2f} GiB, {wall:.2f} s")
    assert peak <= LIMIT
    assert torch.cuda.memory_allocated() < GIB // 4, "a test kept its buffers"


def need(nbytes):
    """Skip only when the device has less free memory than the test allocates."""
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes + GIB // 2:
        pytest.skip(f"{free / GIB:.1f} GiB free, the test needs {nbytes / GIB:.1f}")


def misaligned(nbytes, by=3):
    """Scratch of nbytes at an address that is `by` past a 16-B boundary."""
    return torch.empty(nbytes + by, dtype=torch.uint8, device="cuda")[by:]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the pool of datagrams --------------------------------------------------------------------
class Pool:
    """A few dozen datagrams of type `ptype` and seqNum 0 in rows of CW bytes (random bytes
    behind each datagram): full 1456-byte payloads, the short and empty ones, 1473-1500-byte
    datagrams, runts (recv_len < 16 over a good datagram), corrupt payloads and wrong checksums;
    with the oracle's verdicts.  `full` / `long` / `odd` name rows by kind."""

    def __init__(self, ptype, seed):
        rng = np.random.default_rng(seed)
        plens = [MAXP] * 6 + [0, 1, 15, 16, 17, 255, 1440, 1455, 1457, 1460, 1484, 1484]
        kinds = ["full"] * 6 + ["short"] * 8 + ["long"] * 4
        spoil = [("flip", MAXP), ("flip", 100), ("flip", 1484), ("sum", MAXP), ("sum", 0), ("runt", 0), ("runt", 8), ("runt", 15)]
        self.rows = rng.integers(0, 256, (len(plens) + len(spoil), CW), dtype=np.uint8)
        self.rl = np.zeros(self.rows.shape[0], dtype=np.uint32)
        for k, ln in enumerate(plens + [MAXP if s[0] == "runt" else s[1] for s in spoil]):
            d = np.frombuffer(O.build_datagram(0, O.synth_fill_np(ln, start_byte=1009 * k, seed=seed).tobytes(), ptype), np.uint8)
            self.rows[k, :d.size] = d
            self.rl[k] = d.size
        for k, (how, v) in enumerate(spoil, len(plens)):
            kinds.append(how)
            if how == "flip":
                self.rows[k, 16 + int(rng.integers(0, v))] ^= 0x20
            elif how == "sum":
                self.rows[k, 15] ^= 1
            else:
                self.rl[k] = v
        self.kinds = np.array(kinds)
        self.ok, self.crc = R.verify_limited(self.rows.reshape(-1), CW, self.rl)
        assert self.ok[self.kinds == "full"].all() and self.ok[self.kinds == "long"].all() and self.ok[self.kinds == "short"].all()
        assert not self.ok[np.isin(self.kinds, ("flip", "sum", "runt"))].any()
        self.full = np.flatnonzero(self.kinds == "full")
        self.long = np.flatnonzero((self.rl == 1500) & (self.ok == 1))
        self.odd = np.flatnonzero(self.kinds != "full")
        self.good = np.flatnonzero(np.isin(self.kinds, ("full", "short")))   # placeable DATA, plain ACKs
        self.dev = dev(self.rows)

    def pick(self, n, stride, seed, cuts=(), mostly_good=False):
        """A pool row for each of n ring slots: random (nine in ten of them `good` with
        mostly_good), every kind of odd datagram in the three slots on either side of each
        boundary and of each sub-batch cut (index multiples of `cuts`), a 1500-byte datagram in
        the slot that ends below a boundary and a full one in the slot that contains it or
        begins at it."""
        rng = np.random.default_rng(seed)
        idx = rng.integers(0, self.rl.size, n)
        if mostly_good:
            idx = np.where(rng.random(n) < 0.9, self.good[rng.integers(0, self.good.size, n)], idx)
        centres = [b // stride for b in BOUNDS] + [m for c in cuts for m in range(c, n, c)]
        k = 0
        for c in sorted(set(centres)):
            for j in range(max(c - 3, 0), min(c + 4, n)):
                idx[j] = self.odd[k % self.odd.size]
                k += 1
        for b in BOUNDS:
            idx[b // stride - 1], idx[b // stride] = self.long[0], self.full[b % 5]
        assert b // stride + 1 < n
        return idx


@pytest.fixture(scope="module")
def data_pool():
    return Pool(2, 0xDA7A)


@pytest.fixture(scope="module")
def ack_pool():
    return Pool(3, 0xACC)


def ring_straddles(idx_rl, stride, contains=True):
    n = idx_rl.size
    assert n * stride > BOUNDS[1]
    assert_straddles(np.arange(n, dtype=np.int64) * stride, idx_rl, stride, contains=contains)


# ---- wtp_crc32_verify_batch -------------------------------------------------------------------
GENERAL_16K = straddling_stride(BRAID_STRIDE + 1, 1025)  # a stride the braided paths do not take, entries contain the boundaries


@pytest.mark.parametrize("stride,off", [(WIDE_STRIDE, 0), (WIDE_STRIDE, 5), (BRAID_STRIDE, 0), (GENERAL_16K, 5)])
def test_verify_ring_past_4_gib(W, data_pool, stride, off):
    """Wide stride: the general path on an aligned and a misaligned ring.  Stride 16384 on an
    aligned ring: the braided path with its fix-ups in four sub-launches, cut at index
    multiples of 131071.  A stride just above 16384 on a misaligned ring: the general path in
    six sub-launches.  Each ring is long enough for its last sub-launch to begin above byte 2^32
    (5.4 to 6.5 GB).  Every ok and crc against the oracle's verdict on the entry's pool row."""
    P = data_pool
    braided = stride == BRAID_STRIDE
    cuts = (((1 << 31) - 4096) // stride,) if braided else ((1 << 30) // stride,)
    n = -(-BOUNDS[1] // (cuts[0] * stride)) * cuts[0] + 300  # the last sub-launch begins above 2^32
    assert n // cuts[0] * cuts[0] * stride >= BOUNDS[1]
    need(n * stride + n * CW)
    idx = P.pick(n, stride, 7 + off, cuts)
    ring_straddles(P.rl[idx], stride, contains=not braided)
    ring = rl = ok = crc = None
    try:
        ring = SparseRing(n, stride, P.dev[dev(idx)], FILL, off)
        rl, ok, crc = Words(P.rl[idx]), Bytes(fill=7, size=n, front=16), Words(0x0BAD0BAD, n)
        W.verify_batch(ring.t, stride, rl.t, n, ok.t, crc.t)
        torch.cuda.synchronize()
        assert ("VerifyBEpi" in W.LIB.wtp_last_kernel().decode()) == braided
        got_ok, got_crc = ok.get(), crc.get()
        bad = np.flatnonzero((got_ok != P.ok[idx]) | (got_crc != P.crc[idx]))
        assert bad.size == 0, f"{bad.size} verdicts differ, first at entries {bad[:5]} (kinds {P.kinds[idx[bad[:5]]]})"
        assert_no_data_error(W)
        assert np.array_equal(rl.get(), P.rl[idx])
    finally:
        del ring, rl, ok, crc
        torch.cuda.empty_cache()


# ---- wtp_crc32_batch_fixed --------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_pool():
    """64 chunks of 1456 bytes and the oracle's CRC of each."""
    rows = O.synth_fill_np(64 * MAXP, start_byte=0xC0FFEE).reshape(64, MAXP)
    return rows, np.array([O.crc32(r) for r in rows], dtype=np.uint32)


@pytest.mark.parametrize("stride,off", [(BRAID_STRIDE, 0), (GENERAL_16K, 5)])
def test_fixed_payload_buffer_past_4_gib(W, chunk_pool, stride, off):
    """The braided fast path at stride 16384, and the general path on a misaligned base in its
    1 GiB sub-batches: every CRC against the oracle's for the entry's pool chunk."""
    rows, crcs = chunk_pool
    n = (1 << 32) // stride + 220
    if off:  # the general path's sub-batches: the last one begins above byte 2^32
        per = ((1 << 30) - 4096) // stride
        n = -(-BOUNDS[1] // (per * stride)) * per + 300
        assert n // per * per * stride >= BOUNDS[1]
    need(n * stride + n * MAXP)
    idx = np.random.default_rng(11 + off).integers(0, 64, n)
    ring_straddles(np.full(n, MAXP), stride, contains=off != 0)
    ring = out = None
    try:
        ring = SparseRing(n, stride, dev(rows)[dev(idx)], FILL, off)
        out = Words(0x0BAD0BAD, n)
        W.crc32_batch_fixed(ring.t, stride, MAXP, n, out.t)
        torch.cuda.synchronize()
        assert W.LIB.wtp_last_kernel().decode().startswith("k_fixed_braid" if off == 0 else "k_pieces")
        bad = np.flatnonzero(out.get() != crcs[idx])
        assert bad.size == 0, f"{bad.size} CRCs differ, first at entries {bad[:5]}"
        assert_no_data_error(W)
    finally:
        del ring, out
        torch.cuda.empty_cache()


# ---- wtp_crc32_buffer -------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("off", [0, 5])
def test_buffer_crc_just_past_the_boundaries(W, bound, off):
    """nbytes just above 2^31 and 2^32 on an aligned and a misaligned base, with a tail that is
    neither empty nor a multiple of 16: the CRC against the host fold of the period's oracle CRC."""
    period = O.synth_fill_np(1_000_003, start_byte=off)
    nbytes = bound + 3 * MAXP + 777
    assert (nbytes - (16 - off) % 16) % MAXP % 16 != 0
    need(nbytes + W.buffer_work_bytes(nbytes))
    mem = out = work = None
    try:
        mem, out = periodic(period, nbytes, off), Words(0x0BAD0BAD, 1)
        work = torch.empty(W.buffer_work_bytes(nbytes), dtype=torch.uint8, device="cuda")
        W.crc32_buffer(mem.t, nbytes, out.t, work=work)
        torch.cuda.synchronize()
        assert int(out.get()[0]) == periodic_crc(period, nbytes)
        mem.check_guards()
        assert_no_data_error(W)
    finally:
        del mem, out, work
        torch.cuda.empty_cache()


# ---- wtp_build_data_packets -------------------------------------------------------------------
def header_rows(seq, length, crc):
    """(n, 16) header bytes of DATA datagrams from int64 device tensors."""
    return be_words([torch.full_like(seq, 2), seq & M32, length, crc])


THREE_STEP = straddling_stride(16400, 1025, step=16)  # above the fused path's largest stride; entries contain the boundaries


@pytest.mark.parametrize("wire_stride,pay_off", [(BRAID_STRIDE, 0), (16400, 3), (THREE_STEP, 3)])
def test_build_fixed_wire_ring_past_4_gib(W, chunk_pool, wire_stride, pay_off):
    """More than 262,209 full chunks and a short tail into a wire ring of 4.3 GB: the fused
    path at wire_stride 16384, the three-step path at 16400 and at a stride whose slots contain
    the boundaries, from a misaligned payload.  seqNum, length and d_wire_len by arithmetic, the checksum from the pool chunks'
    oracle CRCs, the payload bytes and every sentinel byte by device compare."""
    rows, crcs = chunk_pool
    nfull, tail, seq0 = (1 << 32) // wire_stride + 220, 333, 0xFFFFF000
    n, total = nfull + 1, nfull * MAXP + tail
    need(n * wire_stride + 3 * n * DW)
    idx = np.random.default_rng(13 + pay_off).integers(0, 64, n)
    lens = np.full(n, MAXP)
    lens[-1] = tail
    ring_straddles(16 + lens, wire_stride, contains=wire_stride == THREE_STEP)
    crc = crcs[idx].copy()
    crc[-1] = O.crc32(rows[idx[-1], :tail])
    pay = wire = wlen = want = None
    try:
        chunks = dev(rows)[dev(idx)]
        pay = Bytes(fill=0, size=total, off=pay_off)
        pay.payload[:nfull * MAXP].view(nfull, MAXP).copy_(chunks[:nfull])
        pay.payload[nfull * MAXP:].copy_(chunks[nfull, :tail])
        want = torch.cat([header_rows(seq0 + torch.arange(n, device="cuda"), dev(lens), dev(crc.astype(np.int64))), chunks], dim=1)
        want[nfull, 16 + tail:] = FILL
        del chunks
        wire, wlen = SparseRing(n, wire_stride, None, FILL), Words(0x0BAD0BAD, n)
        W.build_data_packets(pay.t, total, seq0, wire.t, wire_stride, wlen.t)
        torch.cuda.synchronize()
        wire.assert_rows(want)
        assert np.array_equal(wlen.get(), 16 + lens)
        pay.check_guards()
    finally:
        del pay, wire, wlen, want
        torch.cuda.empty_cache()


def test_build_fixed_source_past_4_gib(W, chunk_pool):
    """total_bytes above 2^32 at wire_stride 1472 from a periodic payload (the 64 pool chunks
    repeated): chunk i is pool chunk i mod 64, so its checksum is that chunk's oracle CRC; the
    source and the wire ring both pass 2^32.  Rows are generated and compared in pieces."""
    rows, crcs = chunk_pool
    total, seq0 = (1 << 32) + 100 * MAXP + 333, 0xFFF00000
    n, tail = -(-total // MAXP), total % MAXP
    need(total + n * DW + 3 * PIECE)
    ring_straddles(np.full(n, DW), DW)        # the wire ring
    ring_straddles(np.full(n, MAXP), MAXP)    # the source
    pool, dcrc = dev(rows), dev(crcs.astype(np.int64))

    def want(a, b):
        i = torch.arange(a, b, device="cuda")
        r = torch.cat([header_rows(seq0 + i, torch.where(i == n - 1, tail, MAXP), dcrc[i % 64]), pool[i % 64]], dim=1)
        if b == n:
            r[-1, :16] = header_rows(seq0 + i[-1:], i[-1:] * 0 + tail, i[-1:] * 0 + O.crc32(rows[(n - 1) % 64, :tail]))[0]
            r[-1, 16 + tail:] = FILL
        return r

    pay = wire = wlen = None
    try:
        pay = periodic(rows.reshape(-1), total)
        wire, wlen = SparseRing(n, DW, None, FILL), Words(0x0BAD0BAD, n)
        W.build_data_packets(pay.t, total, seq0, wire.t, DW, wlen.t)
        torch.cuda.synchronize()
        wire.assert_rows(want, DW)
        got = wlen.get()
        assert (got[:-1] == DW).all() and got[-1] == 16 + tail
        pay.check_guards()
    finally:
        del pay, wire, wlen
        torch.cuda.empty_cache()


# ---- wtp_build_data_packets_var ---------------------------------------------------------------
EDGE_LENS = (0, 1, 15, 16, 17, 255, 1440, 1455, 1456)


def edge_records(n, seed, invalid_at):
    """A Batch of n packed records whose lengths cycle through the edge lengths, full-length ones
    in the slots that end below, contain and follow each boundary of a WIDE_STRIDE ring, and
    invalid records (a length above 1456, an offset past the buffer) at `invalid_at`."""
    lens = np.array([EDGE_LENS[i % len(EDGE_LENS)] for i in range(n)], dtype=np.uint32)
    for b in BOUNDS:
        lens[b // WIDE_STRIDE - 1:b // WIDE_STRIDE + 2] = MAXP
    offs = buildvar_model.packed_offsets(lens)
    base = O.synth_fill_np(int(lens.sum()), start_byte=seed)
    for k, i in enumerate(invalid_at):
        if k % 2:
            offs[i] = base.size + 1 + k
        else:
            lens[i] = (MAXP + 1, 4097, 0xFFFFFFFF)[k // 2 % 3]
    return base, offs, lens


def rows_of(wire, n, stride=DW):
    return dev(wire[:n * stride].reshape(n, stride))


@pytest.mark.parametrize("off", [0, 5])
def test_build_var_wire_ring_past_4_gib(W, off):
    """About 4100 records of the edge lengths into a wire ring of stride ~1 MiB, aligned (vector
    stores) and misaligned (bytewise), with invalid records on both sides of each boundary, whose
    slots keep the sentinel: the model's datagrams on a compact image, slot by slot."""
    n, seq0 = WIDE_N, 0xFFFFF800
    inv = [b // WIDE_STRIDE + d for b in BOUNDS for d in (-3, -2, 2, 3)]
    base, offs, lens = edge_records(n, 0xB1D, inv)
    need(n * WIDE_STRIDE)
    want_wire, want_len, want_crc = buildvar_model.build(base, base.size, offs, lens, seq0, np.full(n * DW, FILL, np.uint8), DW)
    assert (want_len[inv] == 0).all() and (want_len > 0).sum() == n - len(inv)
    ring_straddles(want_len, WIDE_STRIDE)
    b = wire = wlen = crc = None
    try:
        b = Batch(base, offs, lens, base_off=off)
        wire, wlen, crc = SparseRing(n, WIDE_STRIDE, None, FILL, off), Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, n)
        W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, wire.t, WIDE_STRIDE, wlen.t, crc.t)
        torch.cuda.synchronize()
        wire.assert_rows(rows_of(want_wire, n))
        assert np.array_equal(wlen.get(), want_len) and np.array_equal(crc.get(), want_crc)
        b.check_untouched()
    finally:
        del b, wire, wlen, crc
        torch.cuda.empty_cache()


# ---- wtp_tx_build_retransmit, wtp_tx_build_retransmit_var ---------------------------------------
INFLIGHT, NOW, TIMEOUT = 3 * 4200, 20, 50


def sparse_window():
    """acked / sent_ms of a window whose due slots are s % 3 == 1 (4200 of them): s % 3 == 0 is
    ACKed, s % 3 == 2 is un-ACKed but young; the clock wrapped between send and now."""
    s = np.arange(INFLIGHT)
    acked = (s % 3 == 0).astype(np.uint32)
    sent = np.where(s % 3 == 1, (NOW - TIMEOUT - 1 - s % 7) & M32, (NOW - TIMEOUT + s % 5) & M32).astype(np.uint32)
    return acked, sent


@pytest.mark.parametrize("off", [0, 5])
def test_retransmit_wire_ring_past_4_gib(W, off):
    """max_sel 4104 entries of stride ~1 MiB and 4200 due slots, every third one, so d_sel[k] =
    3k + 1: wire, d_sel, d_wire_len, the timers and the counts against the model."""
    total, seq0, max_sel = INFLIGHT * MAXP - 456, 0xFFFFE000, WIDE_N
    need(max_sel * WIDE_STRIDE)
    payloads = O.synth_fill_np(total, start_byte=0x7E7)
    acked, sent = sparse_window()
    sel, dgrams, want_sent, counts = R.retransmit(payloads, total, seq0, INFLIGHT, acked, sent, NOW, TIMEOUT, 0, max_sel, vectorised=True)
    assert counts == (max_sel, 4200) and sel[:3].tolist() == [1, 4, 7]
    want = np.full((max_sel, DW), FILL, np.uint8)
    for k, d in enumerate(dgrams):
        want[k, :len(d)] = np.frombuffer(d, np.uint8)
    ring_straddles(np.array([len(d) for d in dgrams]), WIDE_STRIDE)
    pay = wire = outs = d_acked = d_sent = d_sel = d_wlen = d_counts = None
    try:
        pay, wire = Bytes(payloads, off=off), SparseRing(max_sel, WIDE_STRIDE, None, FILL, off)
        outs = [Words(acked), Words(sent), Words(0x0BAD0BAD, max_sel), Words(0x0BAD0BAD, max_sel), Words(0x0BAD0BAD, 2)]
        d_acked, d_sent, d_sel, d_wlen, d_counts = outs
        W.tx_build_retransmit(pay.t, total, seq0, INFLIGHT, d_acked.t, d_sent.t, NOW, TIMEOUT, 0, wire.t, WIDE_STRIDE, max_sel,
                              d_sel.t, d_wlen.t, d_counts.t, work=misaligned(W.tx_work_bytes(INFLIGHT, max_sel)))
        torch.cuda.synchronize()
        wire.assert_rows(dev(want))
        assert d_counts.get().tolist() == list(counts) and np.array_equal(d_sel.get(), sel)
        assert np.array_equal(d_wlen.get(), [len(d) for d in dgrams]) and np.array_equal(d_sent.get(), want_sent)
        assert np.array_equal(d_acked.get(), acked) and np.array_equal(pay.get(), payloads)
    finally:
        del pay, wire, outs, d_acked, d_sent, d_sel, d_wlen, d_counts
        torch.cuda.empty_cache()


@pytest.mark.parametrize("off", [0, 5])
def test_retransmit_var_wire_ring_past_4_gib(W, off):
    """The same window over records of the edge lengths, some of them invalid: every output of
    wtp_tx_build_retransmit_var against the model on a compact image."""
    seq0, max_sel = 0xFFFFE000, WIDE_N
    need(max_sel * WIDE_STRIDE)
    inv = [3 * (b // WIDE_STRIDE + d) + 1 for b in BOUNDS for d in (-3, -2, 2, 3)]  # the slots of entries k = boundary +- 2, 3
    base, offs, lens = edge_records(INFLIGHT, 0x7E8, inv)
    for b in BOUNDS:  # entry k holds slot 3k + 1: full-length records in the entries around each boundary
        for k in range(b // WIDE_STRIDE - 1, b // WIDE_STRIDE + 2):
            lens[3 * k + 1], offs[3 * k + 1] = MAXP, 0
    acked, sent = sparse_window()
    prior = np.full(max_sel, 0x0BAD0BAD, np.uint32)
    want_wire, sel, want_len, want_crc, want_sent, counts = retxvar_model.retransmit_var(
        base, base.size, offs, lens, seq0, INFLIGHT, acked, sent, NOW, TIMEOUT, 0, np.full(max_sel * DW, FILL, np.uint8), DW, max_sel,
        prior, prior, prior, vectorised=True)
    assert counts == (max_sel, 4200) and sel[:3].tolist() == [1, 4, 7] and (want_len == 0).sum() == len(inv)
    ring_straddles(want_len, WIDE_STRIDE)
    b = wire = outs = d_acked = d_sent = d_sel = d_wlen = d_crc = d_counts = None
    try:
        b, wire = Batch(base, offs, lens, base_off=off), SparseRing(max_sel, WIDE_STRIDE, None, FILL, off)
        outs = [Words(acked), Words(sent), Words(prior), Words(prior), Words(prior), Words(0x0BAD0BAD, 2)]
        d_acked, d_sent, d_sel, d_wlen, d_crc, d_counts = outs
        W.tx_build_retransmit_var(b.base, b.base_bytes, b.o, b.l.t, seq0, INFLIGHT, d_acked.t, d_sent.t, NOW, TIMEOUT, 0, wire.t,
                                  WIDE_STRIDE, max_sel, d_sel.t, d_wlen.t, d_crc.t, d_counts.t,
                                  work=misaligned(W.tx_work_bytes(INFLIGHT, max_sel)))
        torch.cuda.synchronize()
        wire.assert_rows(rows_of(want_wire, max_sel))
        assert d_counts.get().tolist() == list(counts) and np.array_equal(d_sel.get(), sel)
        assert np.array_equal(d_wlen.get(), want_len) and np.array_equal(d_crc.get(), want_crc)
        assert np.array_equal(d_sent.get(), want_sent) and np.array_equal(d_acked.get(), acked)
        b.check_untouched()
    finally:
        del b, wire, outs, d_acked, d_sent, d_sel, d_wlen, d_crc, d_counts
        torch.cuda.empty_cache()


# ---- wtp_accept_data_packets, wtp_rx_build_acks, wtp_tx_ingest_acks -----------------------------
def with_seqs(P, idx, seqs):
    """The compact host ring of pool rows idx with these seqNums (the CRC covers the payload
    only, so the verdicts stay the pool's)."""
    rows = P.rows[idx].copy()
    rows[:, 4:8] = np.asarray(seqs, dtype=np.uint32).astype(">u4").view(np.uint8).reshape(-1, 4)
    return rows


def window_seqs(n, window, seq0, seed):
    """A seqNum per datagram: most once each inside the window, some twice, some at and above
    its end, some below it."""
    rng = np.random.default_rng(seed)
    s = np.resize(rng.permutation(window), n).astype(np.int64)
    dup = rng.random(n) < 0.03
    s[dup] = s[rng.integers(0, n, int(dup.sum()))]
    s = np.where(rng.random(n) < 0.02, window + rng.integers(0, 3, n), s)
    s = np.where(rng.random(n) < 0.02, -1 - rng.integers(0, 1000, n), s)
    return (seq0 + s) & M32


@pytest.mark.parametrize("off", [0, 5])
def test_accept_and_acks_rings_past_4_gib(W, data_pool, off):
    """5000 datagrams in a ring of stride ~1 MiB (5.2 GB) into a window of 5100 slots whose
    sequence numbers wrap: all five outputs of accept against the model on the compact ring;
    then wtp_rx_build_acks in both modes from the model's verdicts into an ACK ring that passes
    4 GiB too (stride ~1 MiB; an odd stride on the misaligned run, so that ACKs contain the
    boundaries): every ACK, d_src, the counts and every sentinel byte."""
    P, n, window, seq0 = data_pool, 5000, 5100, 0xFFFFF000
    ack_stride = WIDE_STRIDE if off == 0 else ODD_STRIDE
    need(n * WIDE_STRIDE + n * ack_stride)
    idx = P.pick(n, WIDE_STRIDE, 17 + off, mostly_good=True)
    rl = P.rl[idx]
    ring_straddles(rl, WIDE_STRIDE)
    compact = with_seqs(P, idx, window_seqs(n, window, seq0, 19 + off)).reshape(-1)
    win = ring = d_rl = ok = place = ack = acks = src = counts = None
    want = accept_model.accept(compact, CW, rl, seq0, window, np.full(window * MAXP, 0xA5, np.uint8),
                               np.full(window, accept_model.EMPTY, np.uint32))
    assert (want[1] != accept_model.NOT_PLACED).sum() > 3500
    try:
        win = DevWindow(window, out_off=off and 4)
        ring = SparseRing(n, WIDE_STRIDE, dev(compact.reshape(n, CW)), FILL, off)
        d_rl, ok = Words(rl), Bytes(fill=7, size=n, front=16)
        place, ack = Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, 1)
        W.accept_data_packets(ring.t, WIDE_STRIDE, d_rl.t, n, seq0, window, win.out, win.slot_len, ok.t, place.t, ack.t)
        torch.cuda.synchronize()
        assert np.array_equal(ok.get(), want[0]) and np.array_equal(place.get(), want[1])
        assert np.array_equal(win.sl.get(), want[3]) and int(ack.get()[0]) == want[4]
        assert np.array_equal(win.img.get(), want[2])
        assert_no_data_error(W)
        ring.assert_rows(dev(compact.reshape(n, CW)))  # the ring is only read
        # the ACKs, from the model's verdicts
        d_ok, d_place, d_sl = dev(want[0]), dev_s32(want[1]), dev_s32(want[3])
        for mode in (R.SELECTIVE, R.CUMULATIVE):
            seqs, want_src, want_counts = ack_model.build_acks(compact, CW, rl, mode, seq0, window, want[1], want[3], want[0])
            k = want_counts[0]
            assert k == want_counts[1] >= 4100 and k * ack_stride > BOUNDS[1]
            assert_straddles(np.arange(k) * ack_stride, np.full(k, 16), ack_stride, contains=off != 0)
            rows = np.full((n, 16), FILL, np.uint8)
            rows[:k] = ack_model.ack_bytes(seqs)
            acks, src, counts = SparseRing(n, ack_stride, None, FILL, off), Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, 2)
            W.rx_build_acks(ring.t, WIDE_STRIDE, d_rl.t, n, mode, seq0, window, d_ok, d_place, d_sl, acks.t, ack_stride, 0, n,
                            src.t, counts.t, work=misaligned(W.rx_ack_work_bytes(n, window, mode)))
            torch.cuda.synchronize()
            acks.assert_rows(dev(rows))
            assert counts.get().tolist() == list(want_counts) and np.array_equal(src.get()[:k], want_src)
            assert (src.get()[k:] == 0x0BAD0BAD).all()
            acks = None
            torch.cuda.empty_cache()
    finally:
        del win, ring, d_rl, ok, place, ack, acks, src, counts
        torch.cuda.empty_cache()


def test_accept_vector_path_ring_past_4_gib(W, data_pool):
    """262,300 placeable datagrams at stride 16384 (the 16-B vector copy) into a window of 2^20
    slots, every seqNum once: the pool rows are gathered on the device and the seqNums written
    into their headers there.  ok = the pool's verdict, place = seqNum - seq0, the image and
    slot_len by scatter of the pool payloads, the ACK from the leading run."""
    P, n, window, seq0 = data_pool, BRAID_N, 1 << 20, 0xFFFF0000
    need(n * BRAID_STRIDE + 2 * window * MAXP + 2 * n * CW)
    rng = np.random.default_rng(23)
    idx = P.good[rng.integers(0, P.good.size, n)]
    slot = rng.permutation(window)[:n]
    slot[slot < 100] += 100                   # may collide: a first-wins race in the batch...
    slot[:50] = np.arange(50)                 # ...and a leading run of 50 slots
    first = np.zeros(n, bool)
    first[np.unique(slot, return_index=True)[1]] = True
    rl = P.rl[idx]
    ring_straddles(rl, BRAID_STRIDE, contains=False)
    want_place = np.where(first, slot, accept_model.NOT_PLACED).astype(np.uint32)
    want_sl = np.full(window, accept_model.EMPTY, np.uint32)
    want_sl[slot[first]] = rl[first] - 16
    lead = int(np.flatnonzero(want_sl == accept_model.EMPTY)[0])
    assert lead == 50 and (~first).sum() > 0
    ring = rows = img = want_img = sl = d_rl = ok = place = ack = None
    try:
        rows = P.dev[dev(idx)]
        rows[:, 4:8] = be_words([dev((seq0 + slot) & M32)])
        ring = SparseRing(n, BRAID_STRIDE, rows, FILL)
        img = Bytes(fill=0xA5, size=window * MAXP, front=64, back=64)
        want_img = torch.full((window, MAXP), 0xA5, dtype=torch.uint8, device="cuda")
        f = dev(np.flatnonzero(first))
        keep = torch.arange(MAXP, device="cuda")[None, :] < (dev(rl.astype(np.int64))[f, None] - 16)
        want_img[dev(slot)[f]] = torch.where(keep, rows[f, 16:DW], torch.tensor(0xA5, dtype=torch.uint8, device="cuda"))
        sl, d_rl, ok = Words(accept_model.EMPTY, window), Words(rl), Bytes(fill=7, size=n, front=16)
        place, ack = Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, 1)
        W.accept_data_packets(ring.t, BRAID_STRIDE, d_rl.t, n, seq0, window, img.t, sl.t, ok.t, place.t, ack.t)
        torch.cuda.synchronize()
        assert (ok.get() == 1).all() and np.array_equal(place.get(), want_place)
        assert np.array_equal(sl.get(), want_sl) and int(ack.get()[0]) == (seq0 + lead) & M32
        for a in range(0, window, PIECE // MAXP):
            assert torch.equal(img.payload.view(window, MAXP)[a:a + PIECE // MAXP], want_img[a:a + PIECE // MAXP])
        img.check_guards()
        assert_no_data_error(W)
    finally:
        del ring, rows, img, want_img, sl, d_rl, ok, place, ack
        torch.cuda.empty_cache()


@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("mode", [R.SELECTIVE, R.CUMULATIVE])
def test_ingest_ring_past_4_gib(W, ack_pool, off, mode):
    """About 4100 ACK datagrams (plain, with a hashed payload, corrupt, runts) in a ring of stride
    ~1 MiB into a window of 5000 slots: d_ok, d_hit, d_acked and the counts against the model on
    the compact ring."""
    P, n, inflight, seq0 = ack_pool, WIDE_N, 5000, 0xFFFFF000
    need(n * WIDE_STRIDE)
    idx = P.pick(n, WIDE_STRIDE, 29 + off, mostly_good=True)
    rl = P.rl[idx]
    ring_straddles(rl, WIDE_STRIDE)
    seqs = window_seqs(n, inflight if mode == R.SELECTIVE else inflight // 2, seq0, 31 + off)
    compact = with_seqs(P, idx, seqs).reshape(-1)
    acked0 = (np.random.default_rng(37).random(inflight) < 0.2).astype(np.uint32)
    want_ok, want_hit, want_acked, want_counts = R.ingest(compact, CW, rl, mode, seq0, inflight, acked0, vectorised=True)
    assert (want_hit != R.NOT_PLACED).sum() > 3000 and want_counts[1] > 1000
    ring = outs = d_rl = d_acked = ok = hit = counts = None
    try:
        ring = SparseRing(n, WIDE_STRIDE, dev(compact.reshape(n, CW)), FILL, off)
        outs = [Words(rl), Words(acked0), Bytes(fill=7, size=n, front=16), Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, 2)]
        d_rl, d_acked, ok, hit, counts = outs
        W.tx_ingest_acks(ring.t, WIDE_STRIDE, d_rl.t, n, mode, seq0, inflight, d_acked.t, ok.t, hit.t, counts.t)
        torch.cuda.synchronize()
        assert np.array_equal(ok.get(), want_ok) and np.array_equal(hit.get(), want_hit)
        assert np.array_equal(d_acked.get(), want_acked) and counts.get().tolist() == list(want_counts)
    finally:
        del ring, outs, d_rl, d_acked, ok, hit, counts
        torch.cuda.empty_cache()


# ---- wtp_rx_deliver ---------------------------------------------------------------------------
@pytest.mark.parametrize("stream_off,cut", [(BOUNDS[0] - 5000, False), (BOUNDS[1] - 5000, True), (BOUNDS[1] + 4099, False)])
def test_deliver_stream_past_4_gib(W, stream_off, cut):
    """A small window flushed into a stream of more than 2^32 bytes at offsets around 2^31 and
    2^32 (with `cut`, the capacity ends inside the run, so k is decided by a 64-bit compare):
    the stream bytes, the 64-bit offsets, the lengths and the counts against the model, which
    runs on the part of the stream from 8192 bytes before stream_off on; the rest of the 4.3 GB
    keeps its sentinel."""
    window = 600
    lens = [EDGE_LENS[(7 * i) % len(EDGE_LENS)] for i in range(500)]
    img, sl = deliver_model.slot_image([O.synth_fill_np(ln, start_byte=977 * i).tobytes() for i, ln in enumerate(lens)], window)
    room = sum(lens) - (3000 if cut else -3000)
    stream_bytes, origin = stream_off + room, stream_off - 8192
    total = max(stream_bytes, BOUNDS[1] + 4096) + 4096
    need(total)
    local = np.full(8192 + room, FILL, np.uint8)
    want, offs, wl, counts = deliver_model.deliver(img, sl, window, window, local, local.size, 8192, np.full(window, 0x7E7E, np.uint64),
                                                   np.full(window, 0x0BAD0BAD, np.uint32))
    k = int(counts[0])
    offs[:k] += np.uint64(origin)
    assert (k < 500) == cut and int(offs[k - 1]) > stream_off
    assert_straddles(offs[:k].astype(np.int64), wl[:k], MAXP, bounds=[b for b in BOUNDS if stream_off < b < stream_off + room])
    stream = outs = d_img = d_sl = d_offs = d_lens = d_counts = None
    try:
        stream = Bytes(fill=FILL, size=total, guard=FILL)
        outs = [Bytes(img, off=4, front=64, back=64), Words(sl), Words(0x7E7E, window, np.uint64), Words(0x0BAD0BAD, window),
                Words(0x7E7E, 4, np.uint64)]
        d_img, d_sl, d_offs, d_lens, d_counts = outs
        W.rx_deliver(d_img.t, d_sl.t, window, window, stream.t, stream_bytes, stream_off, d_offs.t, d_lens.t, d_counts.t,
                     work=misaligned(W.rx_deliver_work_bytes(window)))
        torch.cuda.synchronize()
        assert np.array_equal(d_counts.get(), counts) and np.array_equal(d_offs.get(), offs) and np.array_equal(d_lens.get(), wl)
        assert np.array_equal(stream.buf[origin:origin + local.size].cpu().numpy(), want)
        assert_filled(stream.buf[:origin], FILL)
        assert_filled(stream.buf[origin + local.size:], FILL)
        assert np.array_equal(d_img.get(), img) and np.array_equal(d_sl.get(), sl)
    finally:
        del stream, outs, d_img, d_sl, d_offs, d_lens, d_counts
        torch.cuda.empty_cache()


# ---- wtp_accept_data_packets_flows, wtp_rx_build_acks_flows -------------------------------------
@pytest.mark.parametrize("off", [0, 5])
def test_flows_accept_and_acks_rings_past_4_gib(W, data_pool, off):
    """The interleaved arrivals of four connections (and of none) in a ring of stride ~1 MiB:
    every output of wtp_accept_data_packets_flows against the model on the compact ring, then
    wtp_rx_build_acks_flows in both modes from the model's verdicts into an ACK ring past 4 GiB."""
    P, n, nflows, window = data_pool, 5000, 4, 1300
    seq0 = np.array([0xFFFFFF00, 5, 0x80000000, 77777], dtype=np.uint32)
    ack_stride = WIDE_STRIDE if off == 0 else ODD_STRIDE
    need(n * WIDE_STRIDE + n * ack_stride)
    rng = np.random.default_rng(43 + off)
    idx = P.pick(n, WIDE_STRIDE, 41 + off, mostly_good=True)
    rl = P.rl[idx]
    ring_straddles(rl, WIDE_STRIDE)
    flow = rng.integers(0, nflows, n).astype(np.uint32)
    seqs = (seq0[flow].astype(np.int64) + window_seqs(n, window, 0, 47 + off)) & M32
    flow[rng.random(n) < 0.03] = F.NO_FLOW
    flow[rng.random(n) < 0.01] = nflows
    compact = with_seqs(P, idx, seqs).reshape(-1)
    out0, sl0 = np.full(nflows * window * MAXP, 0xA5, np.uint8), np.full(nflows * window, F.EMPTY, np.uint32)
    want = F.accept_flows(compact, CW, rl, flow, seq0, nflows, window, out0, sl0)
    assert (want[1] != F.NOT_PLACED).sum() > 2500 and (want[4] != seq0).any()
    ring = img = outs = acks = src = counts = None
    try:
        ring, img = SparseRing(n, WIDE_STRIDE, dev(compact.reshape(n, CW)), FILL, off), Bytes(out0, off=off and 4, front=64, back=64)
        outs = [Words(rl), Words(flow), Words(seq0), Words(sl0), Bytes(fill=7, size=n, front=16), Words(0x0BAD0BAD, n),
                Words(0x0BAD0BAD, nflows)]
        d_rl, d_fl, d_sq, d_sl, ok, place, ack = outs
        W.accept_data_packets_flows(ring.t, WIDE_STRIDE, d_rl.t, d_fl.t, n, d_sq.t, nflows, window, img.t, d_sl.t, ok.t, place.t, ack.t)
        torch.cuda.synchronize()
        assert np.array_equal(ok.get(), want[0]) and np.array_equal(place.get(), want[1])
        assert np.array_equal(d_sl.get(), want[3]) and np.array_equal(ack.get(), want[4])
        assert np.array_equal(img.get(), want[2])
        assert_no_data_error(W)
        d_ok, d_fack = dev(want[0]), dev_s32(want[4])
        for mode in (R.SELECTIVE, R.CUMULATIVE):
            aseq, want_src, want_counts = F.build_acks_flows(compact, CW, rl, flow, mode, seq0, nflows, window, want[0], want[4])
            k = want_counts[0]
            assert k == want_counts[1] >= 4100 and k * ack_stride > BOUNDS[1]
            assert_straddles(np.arange(k) * ack_stride, np.full(k, 16), ack_stride, contains=off != 0)
            rows = np.full((n, 16), FILL, np.uint8)
            rows[:k] = ack_model.ack_bytes(aseq)
            acks, src, counts = SparseRing(n, ack_stride, None, FILL, off), Words(0x0BAD0BAD, n), Words(0x0BAD0BAD, 2)
            W.rx_build_acks_flows(ring.t, WIDE_STRIDE, d_rl.t, d_fl.t, n, mode, d_sq.t, nflows, window, d_ok, d_fack, acks.t, ack_stride,
                                  0, n, src.t, counts.t, work=misaligned(W.rx_ack_flows_work_bytes(n)))
            torch.cuda.synchronize()
            acks.assert_rows(dev(rows))
            assert counts.get().tolist() == list(want_counts) and np.array_equal(src.get()[:k], want_src)
            assert (src.get()[k:] == 0x0BAD0BAD).all()
            acks = None
            torch.cuda.empty_cache()
        ring.assert_rows(dev(compact.reshape(n, CW)))  # the ring is only read
    finally:
        del ring, img, outs, acks, src, counts
        d_rl = d_fl = d_sq = d_sl = ok = place = ack = None
        torch.cuda.empty_cache()


def count_other(t, value):
    """The number of elements of the 1-d tensor `t` that differ from `value`, counted in pieces."""
    return sum(int((t[a:a + PIECE] != value).sum()) for a in range(0, t.numel(), PIECE))


def slot_rows(img, slot, length, fill):
    """(k, 1456) rows: the first length[i] bytes of the image slots slot[i], `fill` behind them."""
    rows = img.view(-1, MAXP)[dev(np.asarray(slot, dtype=np.int64))]
    keep = torch.arange(MAXP, device="cuda")[None, :] < dev(np.asarray(length, dtype=np.int64))[:, None]
    return torch.where(keep, rows, torch.tensor(fill, dtype=torch.uint8, device="cuda"))


def test_flows_accept_image_past_4_gib(W, data_pool):
    """Three flows of 2^20 slots: an image of 4.58 GB.  Datagrams for the global slots around
    byte offsets 2^31 and 2^32 of the image, at the flows' edges, in flow 0's leading run and in
    the last slot, with duplicates, corrupt ones and strangers among them.  Expected by a
    sparse first-wins walk over the pool's verdicts; the placed slots are compared row by row and
    the rest of the image by counting the bytes that left the sentinel."""
    P, nflows, window = data_pool, 3, 1 << 20
    S = nflows * window
    need(S * MAXP + GIB)
    seq0 = np.array([0xFFFFFFF0, 1000, 0xFFF00000], dtype=np.uint32)
    rng = np.random.default_rng(53)
    centres = [b // MAXP for b in BOUNDS]
    g = np.unique(np.concatenate([np.arange(c - 40, c + 41) for c in centres] + [np.arange(S - 40, S), np.arange(30),
                                 np.arange(window - 2, window + 2), np.arange(2 * window - 2, 2 * window + 2), rng.integers(0, S, 300)]))
    g = np.concatenate([rng.permutation(g), rng.choice(g, 60)])  # 60 arrive twice
    n = g.size
    idx = np.where(rng.random(n) < 0.85, P.good[rng.integers(0, P.good.size, n)], rng.integers(0, P.rl.size, n))
    for c in centres:  # the first arrival for the slots below, at and above each boundary is a full datagram
        for slot in (c - 1, c, c + 1):
            idx[np.flatnonzero(g == slot)[0]] = P.full[slot % P.full.size]
    idx[np.flatnonzero(g == S - 1)[0]] = P.full[0]
    rl, flow = P.rl[idx], (g // window).astype(np.uint32)
    seqs = (seq0[flow].astype(np.int64) + g % window) & M32
    flow[rng.random(n) < 0.03] = F.NO_FLOW
    compact = with_seqs(P, idx, seqs)
    want_place, want_sl, owner = np.full(n, F.NOT_PLACED, np.uint32), np.full(S, F.EMPTY, np.uint32), {}
    for i in range(n):  # every datagram is DATA and names a slot inside its flow's window
        if P.ok[idx[i]] and flow[i] < nflows and rl[i] - 16 <= MAXP and int(g[i]) not in owner:
            owner[int(g[i])] = i
            want_place[i], want_sl[g[i]] = g[i] % window, rl[i] - 16
    lead = [int(np.argmax(want_sl[f * window:(f + 1) * window] == F.EMPTY)) for f in range(nflows)]
    assert lead[0] >= 3 and S - 1 in owner and 50 < (~np.isin(np.arange(n), list(owner.values()))).sum()
    slot, who = np.array(sorted(owner)), np.array([owner[s] for s in sorted(owner)])
    assert_straddles(slot * MAXP, want_sl[slot], MAXP)
    ring = img = outs = None
    try:
        ring, img = Bytes(compact.reshape(-1), front=64, back=64), Bytes(fill=0xA5, size=S * MAXP, front=64, back=64)
        outs = [Words(rl), Words(flow), Words(seq0), Words(F.EMPTY, S), Bytes(fill=7, size=n, front=16), Words(0x0BAD0BAD, n),
                Words(0x0BAD0BAD, nflows)]
        d_rl, d_fl, d_sq, d_sl, ok, place, ack = outs
        W.accept_data_packets_flows(ring.t, CW, d_rl.t, d_fl.t, n, d_sq.t, nflows, window, img.t, d_sl.t, ok.t, place.t, ack.t)
        torch.cuda.synchronize()
        assert np.array_equal(ok.get(), P.ok[idx]) and np.array_equal(place.get(), want_place)
        assert np.array_equal(d_sl.get(), want_sl) and np.array_equal(ack.get(), (seq0 + np.array(lead)) & M32)
        want_rows = torch.where(torch.arange(MAXP, device="cuda")[None, :] < dev(want_sl[slot].astype(np.int64))[:, None],
                                dev(compact[who, 16:DW]), torch.tensor(0xA5, dtype=torch.uint8, device="cuda"))
        assert torch.equal(img.payload.view(S, MAXP)[dev(slot)], want_rows)
        assert count_other(img.payload, 0xA5) == int((want_rows != 0xA5).sum())  # nothing outside the placed records
        img.check_guards()
        assert np.array_equal(ring.get(), compact.reshape(-1))
        assert_no_data_error(W)
    finally:
        del ring, img, outs
        d_rl = d_fl = d_sq = d_sl = ok = place = ack = want_rows = None
        torch.cuda.empty_cache()


# ---- wtp_rx_deliver_flows, wtp_rx_advance_flows -------------------------------------------------
SENT32, SENT64 = 0x0BAD0BAD, 0x0BAD0BAD0BAD0BAD


def assert_same(a, b):
    """Two 1-d device tensors of the same size hold the same bytes, compared in pieces."""
    assert a.numel() == b.numel()
    for at in range(0, a.numel(), PIECE):
        assert torch.equal(a[at:at + PIECE], b[at:at + PIECE]), f"the tensors differ in bytes [{at}, {at + PIECE})"


def test_flows_flush_sparse_image_past_4_gib(W, chunk_pool):
    """Six flows of 2^19 slots (an image of 4.58 GB; byte 2^31 lies in flow 2, byte 2^32 in flow
    5): long leading runs of mostly empty records in flows 0, 2 and 5 (flow 5's is its whole
    window, so the image's last slot is delivered), with records of the edge lengths around the
    two boundaries, into a stream at an offset just below 2^32 (so that a full record contains
    byte 2^32 of the stream).  Every output of
    wtp_rx_deliver_flows against the loop-free plan of the model, the stream against the pool
    chunks.  wtp_rx_advance_flows then slides the state by per-flow counts of the test's choice
    into a second image: the lengths and bases against the model, the moved records row by
    row, the rest of the image by counting."""
    rows, _ = chunk_pool
    nflows, window = 6, 1 << 19
    S, adv = nflows * window, np.array([3, 0, 17, 1 << 19, 1, 40], dtype=np.uint64)
    seq0 = np.array([0xFFFFFFFF, 1, 2, 3, 0x7FFFFFFF, 0xFFFFFFD8], dtype=np.uint32)
    need(2 * S * MAXP + GIB)
    centres = [b // MAXP for b in BOUNDS]
    assert [c // window for c in centres] == [2, 5]
    sl = np.full(S, F.EMPTY, np.uint32)
    s = np.arange(window)
    for f, run in ((0, 1000), (2, centres[0] % window + 60), (5, window)):
        sl[f * window:f * window + run] = np.where(s[:run] % 97 == 0, s[:run] % 16 + 1, 0)
        if run < window:
            sl[f * window + run:f * window + run + 5] = (1457, 100, F.EMPTY, 0x80000007, MAXP)  # behind the run
    for c in centres:
        a = int(adv[c // window])
        sl[c - 45:c + 46] = [EDGE_LENS[i % len(EDGE_LENS)] for i in range(91)]
        sl[c - 3:c + 4] = sl[c + a - 3:c + a + 4] = MAXP  # what lies around the boundary before and after the slide
    sl[S - 1] = MAXP
    filled = np.flatnonzero((sl <= MAXP) & (sl > 0))
    g, Q, ln = FM.deliver_flows_plan(sl, nflows, window, window, 1 << 40, 0)[:3]
    stream_off = BOUNDS[1] - int(Q[np.argmax(ln == MAXP)]) - 700   # byte 2^32 of the stream lies in the first full record
    g, Q, ln, w_adv, w_info, w_counts = FM.deliver_flows_plan(sl, nflows, window, window, 1 << 40, stream_off)
    K, total = int(w_counts[0]), int(w_counts[2])
    assert w_adv.tolist() == [1000, 0, centres[0] % window + 60, 0, 0, window] and g[-1] == S - 1
    assert_straddles(g * MAXP, ln, MAXP)                                  # the records in the image
    assert_straddles(stream_off + Q, ln, MAXP, bounds=BOUNDS[1:])         # and in the stream
    want_stream = np.full(total, FILL, np.uint8)
    for r in np.flatnonzero(ln):
        want_stream[Q[r]:Q[r] + ln[r]] = rows[g[r] % 64, :ln[r]]
    _, w_sl, w_sq = FM.advance_flows(None, sl, nflows, window, adv, seq0, None, np.full(S, SENT32, np.uint32),
                                     np.full(nflows, SENT32, np.uint32), fast=True)
    moved = np.flatnonzero((w_sl <= MAXP) & (w_sl > 0))
    src = moved + np.repeat(np.minimum(adv.astype(np.int64), window), window)[moved]
    assert_straddles(moved * MAXP, w_sl[moved], MAXP)
    img = stream = nimg = outs = want_rows = None
    try:
        img = Bytes(fill=0x3C, size=S * MAXP, off=4, front=64, back=64)
        img.payload.view(S, MAXP)[dev(filled)] = dev(rows)[dev(filled % 64)]
        stream = Bytes(fill=FILL, size=stream_off + total + 4096, guard=FILL)
        outs = [Words(sl), Words(77, S + 2, np.uint64), Words(77, S + 2), Words(SENT64, nflows, np.uint64),
                Words(SENT64, 4 * nflows, np.uint64), Words(SENT64, 4, np.uint64)]
        d_sl, offs, lens, d_adv, info, cnt = outs
        W.rx_deliver_flows(img.t, d_sl.t, nflows, window, window, stream.t, stream_off + total + 7, stream_off, offs.t, lens.t,
                           d_adv.t, info.t, cnt.t, work=misaligned(W.rx_deliver_flows_work_bytes(nflows, window)))
        torch.cuda.synchronize()
        assert cnt.get().tolist() == w_counts.tolist() and np.array_equal(d_adv.get(), w_adv)
        assert np.array_equal(info.get().reshape(nflows, 4), w_info)
        assert np.array_equal(offs.get(), np.concatenate([(Q + stream_off).astype(np.uint64), np.full(S + 2 - K, 77, np.uint64)]))
        assert np.array_equal(lens.get(), np.concatenate([ln, np.full(S + 2 - K, 77, np.uint32)]))
        assert np.array_equal(stream.buf[stream_off:stream_off + total].cpu().numpy(), want_stream)
        assert_filled(stream.buf[:stream_off], FILL)
        assert_filled(stream.buf[stream_off + total:], FILL)
        stream = None
        torch.cuda.empty_cache()
        # the slide
        nimg = Bytes(fill=FILL, size=S * MAXP, front=64, back=64)
        outs += [Words(adv, dtype=np.uint64), Words(seq0), Words(SENT32, S), Words(SENT32, nflows)]
        a_adv, d_sq, nsl, nsq = outs[-4:]
        W.rx_advance_flows(img.t, d_sl.t, nflows, window, a_adv.t, d_sq.t, nimg.t, nsl.t, nsq.t)
        torch.cuda.synchronize()
        assert np.array_equal(nsl.get(), w_sl) and np.array_equal(nsq.get(), w_sq)
        want_rows = slot_rows(img.payload, src, w_sl[moved], FILL)
        assert torch.equal(nimg.payload.view(S, MAXP)[dev(moved)], want_rows)
        assert count_other(nimg.payload, FILL) == int((want_rows != FILL).sum())
        nimg.check_guards()
        img.check_guards()
        assert count_other(img.payload, 0x3C) == int((dev(rows)[dev(filled % 64)] != 0x3C).sum())  # the state is only read
        assert np.array_equal(d_sl.get(), sl)
    finally:
        del img, stream, nimg, outs, want_rows
        d_sl = offs = lens = d_adv = info = cnt = a_adv = d_sq = nsl = nsq = None
        torch.cuda.empty_cache()


def test_flows_flush_full_image_past_4_gib(W, chunk_pool):
    """Three flows of 2^20 slots that all hold 1456 bytes: Q_K = 3 * 2^20 * 1456 > 2^32, the
    delivered stream equals the image byte for byte, and d_counts, d_flow_info and d_offsets_out
    are exact 64-bit values.  The advance then slides the state by 1, 2^20 and 12345 slots into a
    second image."""
    rows, _ = chunk_pool
    nflows, window, off = 3, 1 << 20, 5
    S, adv = nflows * window, np.array([1, 1 << 20, 12345], dtype=np.uint64)
    total = S * MAXP
    seq0 = np.array([0xFFFFFFFF, 0xFFF00000, 7], dtype=np.uint32)
    need(2 * total + 3 * PIECE)
    assert total > BOUNDS[1]
    assert_straddles(np.arange(S) * MAXP, np.full(S, MAXP), MAXP)
    assert_straddles(off + np.arange(S) * MAXP, np.full(S, MAXP), MAXP)
    img = stream = nimg = outs = None
    try:
        img = periodic(rows.reshape(-1), total)   # slot g holds pool chunk g % 64
        stream = Bytes(fill=FILL, size=off + total + 100, guard=FILL)
        outs = [Words(MAXP, S), Words(77, S + 2, np.uint64), Words(77, S + 2), Words(SENT64, nflows, np.uint64),
                Words(SENT64, 4 * nflows, np.uint64), Words(SENT64, 4, np.uint64)]
        d_sl, offs, lens, d_adv, info, cnt = outs
        W.rx_deliver_flows(img.t, d_sl.t, nflows, window, window, stream.t, off + total + 100, off, offs.t, lens.t, d_adv.t, info.t,
                           cnt.t, work=misaligned(W.rx_deliver_flows_work_bytes(nflows, window)))
        torch.cuda.synchronize()
        assert cnt.get().tolist() == [S, S, total, total] and d_adv.get().tolist() == [window] * nflows
        assert info.get().reshape(nflows, 4).tolist() == [[window, f * window, off + f * window * MAXP, window * MAXP]
                                                           for f in range(nflows)]
        assert np.array_equal(offs.get(), np.concatenate([off + np.arange(S, dtype=np.uint64) * np.uint64(MAXP), [77, 77]]))
        assert np.array_equal(lens.get(), np.concatenate([np.full(S, MAXP), [77, 77]]))
        assert_same(stream.payload[off:off + total], img.payload)
        assert_filled(stream.payload[:off], FILL)
        assert_filled(stream.payload[off + total:], FILL)
        stream.check_guards()
        stream = None
        torch.cuda.empty_cache()
        # the slide
        nimg = Bytes(fill=FILL, size=total, front=64, back=64)
        outs += [Words(adv, dtype=np.uint64), Words(seq0), Words(SENT32, S), Words(SENT32, nflows)]
        a_adv, d_sq, nsl, nsq = outs[-4:]
        W.rx_advance_flows(img.t, d_sl.t, nflows, window, a_adv.t, d_sq.t, nimg.t, nsl.t, nsq.t)
        torch.cuda.synchronize()
        a = np.minimum(adv, window).astype(np.int64)
        assert np.array_equal(nsq.get(), (seq0 + a) & M32)
        assert np.array_equal(nsl.get(), np.where(np.tile(np.arange(window), nflows) < np.repeat(window - a, window), MAXP, F.EMPTY))
        for f in range(nflows):
            lo, keep, hi = f * window * MAXP, (f * window + window - int(a[f])) * MAXP, (f + 1) * window * MAXP
            assert_same(nimg.payload[lo:keep], img.payload[lo + int(a[f]) * MAXP:hi])
            assert_filled(nimg.payload[keep:hi], FILL)
        nimg.check_guards()
        img.check_guards()
    finally:
        del img, stream, nimg, outs
        d_sl = offs = lens = d_adv = info = cnt = a_adv = d_sq = nsl = nsq = None
        torch.cuda.empty_cache()
