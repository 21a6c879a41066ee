"""What the protocol GPU tests (tests/test_gpu_<call>.py) share: the library fixtures, the
u32 conversions, guarded device buffers, the first-mismatch reporter, the graph capture and
replay choreography, the record batch of the mixed-length calls, the guarded receive window
and the device endpoints behind the model loops, and the sparse rings and periodic buffers of
the tests past 4 GiB.  Nothing here is about one call; a new call's test file takes these
from here and defines none of its own."""
import numpy as np
import pytest

import accept_model
import buildvar_model
import oracle as O
import retx_model as R

torch = pytest.importorskip("torch")
DATA_ERROR_BITS = 0b101  # wtp_device_status: bit 0 (length > max), bit 2 (recv_len changed)
MAXP, STRIDE, M32 = R.MAXP, R.STRIDE, R.M32
GUARD_WORD = 0x5A5A5A5A


def assert_no_data_error(W):
    assert W.device_status(0, clear=False) & DATA_ERROR_BITS == 0


# ---- fixtures ---------------------------------------------------------------------------------
def _library():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import wtp_crc32 as W
    return W


@pytest.fixture(scope="module")
def W():
    """The binding after wtp_init(0), with the device status cleared."""
    W = _library()
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    W.device_status(0, clear=True)
    return W


@pytest.fixture(scope="module")
def W_noinit():
    """The binding with the device status cleared and no wtp_init: for the calls that read
    no library table, whose tests show that they need none."""
    W = _library()
    W.device_status(0, clear=True)
    return W


# ---- conversions ------------------------------------------------------------------------------
def s32(a):
    """The int32 view of a host array of uint32 values (torch has no uint32 arithmetic)."""
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def dev_s32(a):
    """s32(a) as a device tensor."""
    return torch.from_numpy(s32(a)).cuda()


def u32(t):
    """The host uint32 view of an int32 tensor."""
    return t.cpu().numpy().view(np.uint32)


# ---- guarded buffers --------------------------------------------------------------------------
class Words:
    """A device array of n u32 (or u64) words behind a view `t`, with 4 guard words
    (0x5A5A5A5A) after it.  Words(array) or Words(value, n)."""

    def __init__(self, init, n=None, dtype=np.uint32, device="cuda"):
        self.np_t, self.guard = dtype, dtype(GUARD_WORD)
        init = np.full(n, init, dtype=dtype) if n is not None else np.ascontiguousarray(init, dtype=dtype)
        self.n = init.size
        signed = np.int32 if dtype is np.uint32 else np.int64
        self.buf = torch.from_numpy(np.concatenate([init, np.full(4, self.guard, dtype)]).view(signed)).to(device)
        self.t = self.buf[:max(self.n, 1)]

    def get(self):
        h = self.buf.cpu().numpy().view(self.np_t)
        assert (h[self.n:] == self.guard).all()  # nothing written past the array
        return h[:self.n].copy()


class Bytes:
    """`size` payload bytes on the device, `off` bytes past `front` guard bytes at the start of
    a 16-B aligned allocation, and `back` guard bytes behind them (none with flush: the
    payload ends with its allocation).  The payload is a copy of `host`, or `fill`; the guards
    hold `guard`.  `t` is the view from the payload's first byte on."""

    def __init__(self, host=None, fill=None, size=None, off=0, front=0, back=16, guard=0xC3, flush=False, device="cuda"):
        self.host = None if host is None else np.ascontiguousarray(host, dtype=np.uint8)
        self.size = size if host is None else self.host.size
        self.lo, self.guard = front + off, guard
        self.buf = torch.full((self.lo + self.size + (0 if flush else back),), guard, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        if host is not None:
            self.payload.copy_(torch.from_numpy(self.host))
        elif fill != guard:
            self.payload.fill_(fill)
        self.t = self.buf[self.lo:]

    @property
    def payload(self):
        return self.buf[self.lo:self.lo + self.size]

    def get(self):
        """The payload on the host, after asserting that both guards are intact."""
        h = self.buf.cpu().numpy()
        assert (h[:self.lo] == self.guard).all() and (h[self.lo + self.size:] == self.guard).all()  # nothing outside
        return h[self.lo:self.lo + self.size]

    def check_guards(self):
        """The guard asserts alone, on the device: for payloads too large to bring to the host."""
        assert bool((self.buf[:self.lo] == self.guard).all()) and bool((self.buf[self.lo + self.size:] == self.guard).all())


def assert_bytes_equal(got, want, unit, describe):
    """got == want, or an AssertionError that says how many bytes differ and where the first
    one is: its `unit`-byte unit (a slot, a ring entry), the byte within it, and the caller's
    context, `describe` (a string, or a function of the unit's index)."""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    first = int(bad[0])
    context = describe(first // unit) if callable(describe) else describe
    raise AssertionError(f"{bad.size} bytes differ, first at {first}: unit {first // unit}, byte {first % unit} ({context})")


# ---- graphs -----------------------------------------------------------------------------------
def capture(call, stream=None):
    """`call` once on a side stream (outside the capture: what it leaves behind is the state
    the graph starts from), then captured there.  Returns (graph, stream)."""
    stream = torch.cuda.Stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        call()
    return graph, stream


def replay_each_then_together(g, alone, others, together):
    """`g` (an object with graph, stream, reset(*args) and check()) replayed alone once per
    argument tuple of `alone`, each time reset before and checked after; then `others()` makes
    two more, h and k, all three are reset with the tuples of `together` and replayed at once,
    each on its own stream, and checked.  Returns (g, h, k)."""
    for args in alone:
        g.reset(*args)
        torch.cuda.synchronize()
        g.graph.replay()
        torch.cuda.synchronize()
        g.check()
    h, k = others()
    for x, args in zip((g, h, k), together):
        x.reset(*args)
    torch.cuda.synchronize()
    for x in (h, k, g):
        with torch.cuda.stream(x.stream):
            x.graph.replay()
    torch.cuda.synchronize()
    for x in (g, h, k):
        x.check()
    return g, h, k


# ---- records and rings ------------------------------------------------------------------------
class Batch:
    """The device copy of a batch of records: `base` at byte `base_off` of its allocation (16
    guard bytes after it), offsets (u64) and lengths (u32)."""

    def __init__(self, base, offs, lens, base_off=0, base_bytes=None):
        self.mem = Bytes(base, off=base_off)
        self.host = self.mem.host
        self.offs = np.ascontiguousarray(offs, dtype=np.uint64)
        self.lens = np.ascontiguousarray(lens, dtype=np.uint32)
        self.n = self.lens.size
        self.base_bytes = self.host.size if base_bytes is None else base_bytes
        self.base = self.mem.t
        self.o = torch.from_numpy(np.concatenate([self.offs, [np.uint64(0x7E7E)]]).view(np.int64)).cuda()
        self.l = Words(self.lens)

    def phases(self):
        """The source address mod 16 of every non-empty payload."""
        return set(((self.base.data_ptr() + self.offs[self.lens > 0]) % 16).astype(int).tolist())

    def check_untouched(self):
        assert np.array_equal(self.mem.get(), self.host)
        assert np.array_equal(self.o.cpu().numpy().view(np.uint64), np.concatenate([self.offs, [np.uint64(0x7E7E)]]))
        assert np.array_equal(self.l.get(), self.lens)


def packed(lens, salt=0, base_off=0):
    """A Batch of synthetic records of these lengths, back to back."""
    lens = np.asarray(lens, dtype=np.uint32)
    return Batch(O.synth_fill_np(max(int(lens.sum()), 1), start_byte=salt), buildvar_model.packed_offsets(lens), lens,
                 base_off, base_bytes=int(lens.sum()))


def datagram_ring(dgrams, stride, salt=0):
    """(ring, recv_len): `dgrams` in `stride`-byte slots (cut at the slot's end; recv_len
    keeps the full length); the slot bytes past a datagram are random, so a copy that ran
    past recv_len would show."""
    rng = np.random.default_rng(len(dgrams) * 131 + stride + salt)
    ring = rng.integers(0, 256, len(dgrams) * stride, dtype=np.uint8)
    rl = np.zeros(len(dgrams), dtype=np.uint32)
    for i, d in enumerate(dgrams):
        cut = min(len(d), stride)
        ring[i * stride:i * stride + cut] = np.frombuffer(d[:cut], dtype=np.uint8)
        rl[i] = len(d)
    return ring, rl


# ---- the receive window ---------------------------------------------------------------------
class DevWindow:
    """The caller-owned state of wtp_accept_data_packets on the device and its host copy: a
    0xA5 image of `window` slots at byte `out_off` past a 16-B aligned address, between 64
    guard bytes, and slot_len (EMPTY, or the values of `slot_len`) with guard words.  stage()
    uploads one batch (the ring at byte `ring_off` between guards, recv_len) and sentinel-filled
    outputs; check() compares all five outputs with the model's, every guard, and the ring and
    recv_len with what was uploaded; accept() is stage, the call, the model from the same entry
    state, check, and the carry-over of the state."""
    OK_SENT, PLACE_SENT, ACK_SENT = 7, 12345, 0x0BADACC0

    def __init__(self, window, out_off=0, slot_len=None, device="cuda"):
        self.window, self.device = window, device
        self.h_out = np.full(window * MAXP, 0xA5, dtype=np.uint8)
        self.h_slot_len = (np.full(window, accept_model.EMPTY, dtype=np.uint32) if slot_len is None
                           else np.array(slot_len, dtype=np.uint32))
        assert self.h_slot_len.size == window
        self.img = Bytes(self.h_out, off=out_off, front=64, back=64, device=device)
        self.sl = Words(self.h_slot_len, device=device)
        self.out, self.slot_len = self.img.t, self.sl.t

    def stage(self, ring, recv_len, ring_off=0):
        self.ring = Bytes(ring, off=ring_off, front=64, back=64, device=self.device)
        self.rl_host = np.array(recv_len, dtype=np.uint32)
        self.rl = Words(self.rl_host, device=self.device)
        n = self.n = self.rl.n
        self.ok = Bytes(fill=self.OK_SENT, size=n, front=16, back=16, device=self.device)
        self.place = Words(self.PLACE_SENT, n, device=self.device)
        self.ack = Words(self.ACK_SENT, 1, device=self.device)

    def check(self, want, with_place=True, with_ack=True):
        """`want`: accept_model.accept's (ok, place, out, slot_len, ack).  An output that was
        not given to the call still holds its sentinel."""
        want_ok, want_place, want_out, want_sl, want_ack = want
        n = self.n
        assert np.array_equal(self.ok.get(), want_ok)
        assert np.array_equal(self.place.get(), want_place if with_place else np.full(n, self.PLACE_SENT, np.uint32))
        assert np.array_equal(self.sl.get(), want_sl)
        assert_bytes_equal(self.img.get(), want_out, MAXP, lambda s: f"image slot {s}, slot_len {want_sl[s]:#x}")
        assert int(self.ack.get()[0]) == (want_ack if with_ack else self.ACK_SENT)
        assert np.array_equal(self.ring.get(), self.ring.host)  # the inputs are only read
        assert np.array_equal(self.rl.get(), self.rl_host)

    def accept(self, W, ring, stride, recv_len, seq0, ring_off=0, with_place=True, with_ack=True):
        """One call on the device and in the model; returns the model's (ok, place, ack)."""
        self.stage(ring, recv_len, ring_off)
        W.accept_data_packets(self.ring.t, stride, self.rl.t, self.n, seq0, self.window, self.out, self.slot_len,
                              self.ok.t, self.place.t if with_place else None, self.ack.t if with_ack else None)
        torch.cuda.synchronize()
        want = accept_model.accept(ring, stride, recv_len, seq0, self.window, self.h_out, self.h_slot_len)
        self.check(want, with_place, with_ack)
        if self.n or with_ack:  # n == 0 without d_ack launches nothing
            assert W.LIB.wtp_last_kernel().decode() == "k_accept_place"
        assert_no_data_error(W)
        self.h_out, self.h_slot_len = want[2], want[3]
        return want[0], want[1], want[4]


# ---- device endpoints -------------------------------------------------------------------------
def _z(k, v=0):
    return torch.full((k,), v, dtype=torch.int32, device="cuda")


class DevEnd:
    """Both windows on the device, behind the calls of retx_model.transfer: no payload byte
    crosses to the host (it reads back verdicts, 8 header bytes per datagram and counts).
    The state is sized by the transfer; rx_state and tx_state give the calls their part of it."""

    def __init__(self, W, src, total, nchunks, window, seq_base):
        self.W, self.src, self.total, self.window, self.seq_base = W, src, total, window, seq_base
        self.counts, self.ack = _z(2), _z(1)
        self.icounts = self.counts  # where ingest_ring leaves its counts
        self.alloc_state(nchunks, window)
        self.retx_wire = torch.zeros((0, STRIDE), dtype=torch.uint8, device="cuda")
        self.retx_len = _z(0)

    def alloc_state(self, nchunks, window):
        self.acked, self.sent, self.slot_len = _z(nchunks + window), _z(nchunks + window), _z(nchunks + window, -1)
        self.img = torch.full(((nchunks + window) * MAXP,), 0xA5, dtype=torch.uint8, device="cuda")

    def rx_state(self, rbase):
        """(img, slot_len) from chunk rbase on."""
        return self.img[rbase * MAXP:], self.slot_len[rbase:]

    def tx_state(self, sbase):
        """(acked, sent) from chunk sbase on."""
        return self.acked[sbase:], self.sent[sbase:]

    def seq(self, chunk):
        return (self.seq_base + chunk) & M32

    def send(self, c0, cnt, now):
        wire = torch.zeros((cnt, STRIDE), dtype=torch.uint8, device="cuda")
        wlen = torch.zeros(cnt, dtype=torch.int32, device="cuda")
        if cnt:
            nbytes = min(self.total, (c0 + cnt) * MAXP) - c0 * MAXP
            self.W.build_data_packets(self.src[c0 * MAXP:], nbytes, self.seq(c0), wire, STRIDE, wlen)
            self.tx_state(c0)[1][:cnt] = int(s32([now])[0])
        self.wire, self.wlen = torch.cat([wire, self.retx_wire]), torch.cat([wlen, self.retx_len])
        return self.wire.shape[0]

    def accept(self, idx, rbase):
        n = idx.size
        sel = torch.from_numpy(idx.astype(np.int64)).cuda()
        ring, rl = self.wire[sel].contiguous(), self.wlen[sel].contiguous()
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.W.accept_data_packets(ring if n else ok, STRIDE, rl if n else self.ack, n, self.seq(rbase), self.window,
                                   *self.rx_state(rbase), ok, None, self.ack)
        hdr = np.ascontiguousarray(ring[:, :8].cpu().numpy()).reshape(n, 8).view(">u4")
        return (ok[:n].cpu().numpy(), hdr[:, 0].astype(np.uint32), hdr[:, 1].astype(np.uint32),
                int(self.ack.cpu().numpy().view(np.uint32)[0]))

    def ingest(self, acks, mode, sbase, inflight):
        ring, rl = R.make_ring(acks, 16)
        n = rl.size
        d = torch.from_numpy(ring).cuda()
        r = torch.from_numpy(s32(rl)).cuda() if n else self.ack
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.W.tx_ingest_acks(d, 16, r, n, mode, self.seq(sbase), inflight, self.tx_state(sbase)[0], ok, None, self.counts)
        return int(self.counts[0].item())

    def retransmit(self, sbase, inflight, now, timeout, flags, max_sel):
        wire = torch.zeros((max_sel, STRIDE), dtype=torch.uint8, device="cuda")
        sel, wlen = (torch.zeros(max_sel, dtype=torch.int32, device="cuda") for _ in range(2))
        self.W.tx_build_retransmit(self.src[sbase * MAXP:], self.total - sbase * MAXP, self.seq(sbase), inflight,
                                   *self.tx_state(sbase), now, timeout, flags, wire, STRIDE, max_sel, sel, wlen, self.counts)
        e = int(self.counts[0].item())
        self.retx_wire, self.retx_len = wire[:e], wlen[:e]
        return sel[:e].cpu().numpy()


class DevAckEnd(DevEnd):
    """DevEnd behind the calls of ack_model.transfer.  The ACK ring is built by
    wtp_rx_build_acks and never leaves the device: the lossy channel is an index_select over
    its entries, and the selected ring goes straight into wtp_tx_ingest_acks.  The host reads
    back counts only."""

    def accept(self, idx, rbase):
        n = self.n = idx.size
        sel = torch.from_numpy(idx.astype(np.int64)).cuda()
        self.ring, self.rl = self.wire[sel].contiguous(), self.wlen[sel].contiguous()
        self.ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.place = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        self.W.accept_data_packets(self.ring if n else self.ok, STRIDE, self.rl if n else self.ack, n, self.seq(rbase),
                                   self.window, *self.rx_state(rbase), self.ok, self.place, self.ack)
        return int(u32(self.ack)[0])

    def build_acks(self, mode, rbase):
        n = self.n
        self.ack_ring = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device="cuda")
        self.W.rx_build_acks(self.ring if n else self.ok, STRIDE, self.rl if n else self.ack, n, mode, self.seq(rbase),
                             self.window, self.ok, self.place, self.rx_state(rbase)[1], self.ack_ring, 16, 0, n, None,
                             self.counts)
        return int(self.counts[0].item())

    def ingest_ring(self, aidx, mode, sbase, inflight):
        n = aidx.size
        ring = self.ack_ring.index_select(0, torch.from_numpy(aidx.astype(np.int64)).cuda())
        rl = torch.full((max(n, 1),), 16, dtype=torch.int32, device="cuda")
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.W.tx_ingest_acks(ring if n else ok, 16, rl, n, mode, self.seq(sbase), inflight, self.tx_state(sbase)[0], ok,
                              None, self.icounts)
        return int(self.icounts[0].item())


class DevBoundedEnd(DevAckEnd):
    """DevAckEnd with bounded state: `acked` / `sent` hold `window` entries in two buffers slid
    by wtp_tx_advance (fed on the device with the count wtp_tx_ingest_acks wrote, kept in its
    own buffer so that retransmit's counts do not overwrite it), and `slot_len` / `img` hold
    `window` slots in two buffers slid by wtp_rx_advance (fed with wtp_rx_deliver's counts,
    which also appends the leading run to the file)."""

    def alloc_state(self, nchunks, window):
        self.acked, self.sent = [_z(window), _z(window)], [_z(window), _z(window)]
        self.slot_len = [_z(window, -1), _z(window, -1)]
        self.img = [torch.full((window * MAXP,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.file = torch.full((self.total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.adv = self.icounts = _z(2)
        self.dcounts = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.work = torch.empty(self.W.rx_deliver_work_bytes(window), dtype=torch.uint8, device="cuda")
        self.sbase = self.off = 0

    def rx_state(self, rbase):
        return self.img[0], self.slot_len[0]

    def tx_state(self, sbase):
        return self.acked[0][sbase - self.sbase:], self.sent[0][sbase - self.sbase:]

    def send(self, c0, cnt, now):
        if cnt:
            assert 0 <= c0 - self.sbase and c0 - self.sbase + cnt <= self.window
        return super().send(c0, cnt, now)

    def accept(self, idx, rbase):
        ack = super().accept(idx, rbase)
        self.lead = (ack - self.seq(rbase)) & M32
        return ack

    def build_acks(self, mode, rbase):
        emitted = super().build_acks(mode, rbase)
        # the end of the receiver's round: flush the leading run to the file and slide by it
        w = self.window
        self.W.rx_deliver(self.img[0], self.slot_len[0], w, w, self.file, self.total, self.off, None, None, self.dcounts,
                          work=self.work)
        self.W.rx_advance(self.img[0], self.slot_len[0], w, self.dcounts, self.img[1], self.slot_len[1])
        self.img.reverse()
        self.slot_len.reverse()
        k, run, pk, _ = self.dcounts.cpu().tolist()
        assert k == run == self.lead  # deliver's run is accept's cumulative ACK
        self.off += pk
        return emitted

    def ingest_ring(self, aidx, mode, sbase, inflight):
        assert sbase == self.sbase
        self.advance = super().ingest_ring(aidx, mode, sbase, inflight)
        return self.advance

    def retransmit(self, sbase, inflight, now, timeout, flags, max_sel):
        sel = super().retransmit(sbase, inflight, now, timeout, flags, max_sel)
        # the end of the sender's round: slide by the count ingest left on the device
        self.W.tx_advance(self.acked[0], self.sent[0], self.window, self.adv, 0, self.acked[1], self.sent[1])
        self.acked.reverse()
        self.sent.reverse()
        self.sbase += self.advance
        return sel


class DevStreamEnd:
    """The receiver of advance_model.stream_rounds on the device: two (img, slot_len) pairs of
    `window` slots and nothing sized by the transfer but the output stream.  A round is accept
    -> rx_build_acks -> rx_deliver -> rx_advance on the stream, the swap of the pairs, and one
    synchronisation to read deliver's counts."""

    def __init__(self, W, wire, wl, n, stride, seq0, window, total):
        self.W, self.wire, self.wl, self.n, self.stride, self.seq0, self.window = W, wire, wl, n, stride, seq0, window
        self.img = [torch.full((window * MAXP,), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.sl = [torch.full((window,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.whole = Bytes(fill=0xA5, size=total, front=64, back=64, guard=0xA5)
        self.total = total
        self.counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.ack_counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.offs_out = torch.zeros(window, dtype=torch.int64, device="cuda")
        self.lens_out = torch.zeros(window, dtype=torch.int32, device="cuda")
        self.work = torch.empty(W.rx_deliver_work_bytes(window), dtype=torch.uint8, device="cuda")
        self.ack_ring = torch.zeros((window, 16), dtype=torch.uint8, device="cuda")
        self.offs, self.lens, self.acked = [], [], []

    def round(self, idx, base, off, then=None):
        """`then`: what a sender puts on the stream behind the receiver's calls, before the
        round's synchronisation."""
        W, w, n = self.W, self.window, idx.size
        sel = torch.from_numpy(idx.astype(np.int64)).cuda()
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        ring = self.wire.view(self.n, self.stride)[sel].contiguous().view(-1) if n else ok  # n == 0: any pointer
        rl = self.wl[sel].contiguous() if n else self.ack_counts
        seq = (self.seq0 + base) & M32
        W.accept_data_packets(ring, self.stride, rl, n, seq, w, self.img[0], self.sl[0], ok)
        W.rx_build_acks(ring, self.stride, rl, n, R.SELECTIVE, seq, w, ok, None, None, self.ack_ring, 16, 0, w, None,
                        self.ack_counts)
        W.rx_deliver(self.img[0], self.sl[0], w, w, self.whole.t, self.total, off, self.offs_out, self.lens_out,
                     self.counts, work=self.work)
        W.rx_advance(self.img[0], self.sl[0], w, self.counts, self.img[1], self.sl[1])
        self.img.reverse()
        self.sl.reverse()
        if then is not None:
            then()
        torch.cuda.synchronize()
        counts = self.counts.cpu().numpy().view(np.uint64)
        k = int(counts[0])
        assert bool(ok[:n].all()) and u32(self.ack_counts).tolist() == [n, n]  # every arrival is intact and answered
        self.offs += self.offs_out[:k].cpu().numpy().view(np.uint64).tolist()
        self.lens += u32(self.lens_out[:k]).tolist()
        return counts


# ---- extents past 4 GiB -----------------------------------------------------------------------
# What tests/test_gpu_wide.py shares: buffers whose extent passes 2^32 bytes while the work in
# them stays small.  Every helper takes the two boundaries as an argument, so the CPU tests
# (tests/test_gpu_support.py) run the same expectation code around a boundary of 2^12.
BOUNDS = (1 << 31, 1 << 32)
# 2049 * WIDE_STRIDE = 2^31 - 512 and 4098 * WIDE_STRIDE = 2^32 - 1024: a 1472-byte entry in
# slot 2049 contains byte 2^31 and one in slot 4098 contains byte 2^32; stride % 16 == 0
WIDE_STRIDE = (1 << 20) - 512
# 2046 * ODD_STRIDE = 2^31 - 2 and 4092 * ODD_STRIDE = 2^32 - 4: an odd stride at which 16-byte
# entries (ACKs) in slots 2046 and 4092 contain the boundaries
ODD_STRIDE = 1049601
WIDE_N = 4104       # slots of a WIDE_STRIDE ring: 4104 * WIDE_STRIDE > 2^32 + 6 MB
PIECE = 512 << 20   # the most one device comparison looks at


def slots(t, n, stride, width):
    """The view (n, width) of the first `width` bytes of n slots `stride` bytes apart, from the
    first byte of the byte tensor `t` on."""
    assert n == 0 or (n - 1) * stride + width <= t.numel()
    return t.as_strided((n, width), (stride, 1))


class SparseRing:
    """n slots of `stride` bytes that hold `fill`, at byte `off` of a 16-B aligned allocation
    with `back` bytes of `fill` behind the last slot; rows (n x width bytes, on the ring's
    device) go to the start of the slots.  `t` is the view from the ring's first byte on."""

    def __init__(self, n, stride, rows=None, fill=0xEE, off=0, back=64, device="cuda"):
        self.n, self.stride, self.fill, self.off = n, stride, fill, off
        self.buf = torch.full((off + n * stride + back,), fill, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[off:]
        if rows is not None:
            slots(self.t, n, stride, rows.shape[1]).copy_(rows)

    def rows(self, width, first=0, count=None):
        count = self.n - first if count is None else count
        return slots(self.t[first * self.stride:], count, self.stride, width)

    def assert_rows(self, want, width=None):
        """Slot i starts with want[i] (n x width, on the device; or a function of (a, b) that
        makes rows a .. b - 1, with `width` given); every other byte of the allocation holds
        `fill`: the slot tails, the bytes in front of the ring and behind it."""
        n = self.n
        if not callable(want):
            assert want.shape[0] == n
            rows, width = want, want.shape[1]
            want = lambda a, b: rows[a:b]  # noqa: E731
        per = max(1, PIECE // max(width, 1))
        for a in range(0, n, per):
            got, exp = self.rows(width, a, min(per, n - a)), want(a, min(a + per, n))
            if not torch.equal(got, exp):
                bad = torch.nonzero((got != exp).any(dim=1))[:5, 0].cpu().numpy() + a
                raise AssertionError(f"slots {bad.tolist()} differ (byte offsets {[int(b) * self.stride for b in bad]})")
        tail = self.stride - width
        per = max(1, PIECE // max(tail, 1))
        for a in range(0, n if tail else 0, per):
            got = slots(self.t[a * self.stride + width:], min(per, n - a), self.stride, tail)
            if not bool((got == self.fill).all()):
                bad = torch.nonzero((got != self.fill).any(dim=1))[:5, 0].cpu().numpy() + a
                raise AssertionError(f"the tails of slots {bad.tolist()} were written")
        assert_filled(self.buf[:self.off], self.fill)
        assert_filled(self.t[n * self.stride:], self.fill)


def assert_filled(t, value, piece=PIECE):
    """Every element of the 1-d tensor `t` equals `value`, looked at in pieces."""
    for a in range(0, t.numel(), piece):
        if not bool((t[a:a + piece] == value).all()):
            first = a + int(torch.nonzero(t[a:a + piece] != value)[0, 0])
            raise AssertionError(f"element {first} is {int(t[first])}, not {value}")


def assert_straddles(starts, lens, stride, bounds=BOUNDS, contains=True):
    """The batch whose entry i occupies bytes [starts[i], starts[i] + lens[i]) of its buffer has,
    for each boundary B: a non-empty entry that ends in (B - stride, B], an entry that begins at
    or above B and, with `contains` (where stride or offset can be chosen), an entry with
    start < B < end."""
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    ends = starts + lens
    for b in bounds:
        assert ((lens > 0) & (ends <= b) & (ends > b - stride)).any(), f"no entry ends just below {b:#x}"
        assert (starts >= b).any(), f"no entry begins at or above {b:#x}"
        assert not contains or ((starts < b) & (ends > b)).any(), f"no entry contains {b:#x}"


def straddling_stride(start, width, step=1, bounds=BOUNDS):
    """The first stride >= start (in steps of `step`) at which, for each boundary B, the entry
    of `width` bytes in slot B // stride contains B: 0 < B % stride < width."""
    stride = start
    while not all(0 < b % stride < width for b in bounds):
        stride += step
    return stride


def periodic(period, nbytes, off=0, device="cuda"):
    """A Bytes of `nbytes` payload bytes at byte `off` of its allocation: the host array
    `period` repeated on the device, cut at nbytes."""
    mem = Bytes(fill=0, size=nbytes, off=off, device=device)
    p = torch.from_numpy(np.ascontiguousarray(period, dtype=np.uint8)).to(device)
    k, tail = divmod(nbytes, p.numel())
    if k:
        mem.payload[:k * p.numel()].view(k, p.numel()).copy_(p)
    mem.payload[k * p.numel():].copy_(p[:tail])
    return mem


def periodic_crc(period, nbytes):
    """crc32 of `period` repeated and cut at nbytes, from the oracle's CRC of one period (and
    of the cut one at the end) folded on the host with concat_model.combine, by doubling."""
    import concat_model
    period = np.ascontiguousarray(period, dtype=np.uint8)
    k, tail = divmod(nbytes, period.size)
    acc, blk, blk_len = 0, O.crc32(period), period.size
    while k:
        if k & 1:
            acc = concat_model.combine(acc, blk, blk_len)
        blk, blk_len, k = concat_model.combine(blk, blk, blk_len), 2 * blk_len, k >> 1
    return concat_model.combine(acc, O.crc32(period[:tail]), tail)


def be_words(cols):
    """(n, 4 * len(cols)) bytes: the int64 device tensors `cols` (values below 2^32) as
    big-endian 32-bit words side by side, the layout of a header."""
    w = torch.stack([c.to(torch.int64) for c in cols], dim=1)
    sh = torch.tensor([24, 16, 8, 0], dtype=torch.int64, device=w.device)
    return ((w[:, :, None] >> sh) & 0xFF).to(torch.uint8).reshape(w.shape[0], -1)
