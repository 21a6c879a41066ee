"""GPU tests of the device-side sender window, wtp_tx_ingest_acks and
wtp_tx_build_retransmit: every output is compared element-wise with the sequential model
(tests/retx_model.py) from the same entry state, and the state is carried across calls.
Buffers are pre-filled with sentinels (0xA5 wire, 12345 in sel / hit / wire_len) and have
16 guard bytes past their end, so a byte that must stay untouched is checkable."""
import numpy as np
import pytest

import oracle as O
import retx_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DATA_ERROR_BITS = 0b101  # wtp_device_status: bit 0 (length > max), bit 2 (recv_len changed)
MAXP, STRIDE, SENT = M.MAXP, M.STRIDE, 12345


@pytest.fixture(scope="module")
def W():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import wtp_crc32 as W
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    W.device_status(0, clear=True)
    return W


def _s32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


class Words:
    """A u32 device array of n words behind a view, with 4 guard words (0x5A5A5A5A) after it."""

    def __init__(self, init, n=None):
        init = np.full(n, init, dtype=np.uint32) if n is not None else np.ascontiguousarray(init, dtype=np.uint32)
        self.n = init.size
        self.buf = torch.from_numpy(_s32(np.concatenate([init, np.full(4, 0x5A5A5A5A, np.uint32)]))).cuda()
        self.t = self.buf[:max(self.n, 1)]

    def get(self):
        h = self.buf.cpu().numpy().view(np.uint32)
        assert (h[self.n:] == 0x5A5A5A5A).all()  # nothing written past the array
        return h[:self.n].copy()


def _bytes(host, off=0):
    """Device copy of a host byte array at byte offset `off` of its allocation; 16 guard
    bytes (0xC3) after it.  Returns (view, whole buffer)."""
    buf = torch.full((host.size + off + 16,), 0xC3, dtype=torch.uint8, device="cuda")
    buf[off:off + host.size].copy_(torch.from_numpy(host))
    return buf[off:off + max(host.size, 1)], buf


def _ring(dgrams, stride, salt=0):
    """(ring, recv_len): `dgrams` in `stride`-byte slots (cut at the slot's end; recv_len
    keeps the full length); the slot bytes past a datagram are random."""
    rng = np.random.default_rng(len(dgrams) * 131 + stride + salt)
    ring = rng.integers(0, 256, len(dgrams) * stride, dtype=np.uint8)
    rl = np.zeros(len(dgrams), dtype=np.uint32)
    for i, d in enumerate(dgrams):
        cut = min(len(d), stride)
        ring[i * stride:i * stride + cut] = np.frombuffer(d[:cut], dtype=np.uint8)
        rl[i] = len(d)
    return ring, rl


# ---- ingest --------------------------------------------------------------------------------
def ingest(W, ring, rl, stride, mode, seq0, inflight, acked, ring_off=0, with_hit=True):
    """One call on the device and in the model from the same entry state `acked` (numpy);
    asserts every output equal; returns the model's (ok, hit, acked, counts)."""
    n = rl.size
    d, dbuf = _bytes(ring, ring_off)
    r, ok, hit = Words(rl), torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda"), Words(SENT, n)
    st, counts = Words(acked), Words(0x77777777, 2)
    W.tx_ingest_acks(d, stride, r.t, n, mode, seq0, inflight, st.t, ok, hit.t if with_hit else None, counts.t)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == ("k_tx_lead" if mode == M.SELECTIVE else "k_tx_window")
    want_ok, want_hit, want_acked, want_counts = M.ingest(ring, stride, rl, mode, seq0, inflight, acked)
    got_ok = ok.cpu().numpy()
    assert np.array_equal(got_ok[:n], want_ok) and (got_ok[n:] == 7).all()
    assert np.array_equal(hit.get(), want_hit if with_hit else np.full(n, SENT, np.uint32))
    assert np.array_equal(st.get(), want_acked)
    assert tuple(counts.get()) == want_counts
    assert np.array_equal(r.get(), rl) and (dbuf[dbuf.numel() - 16:] == 0xC3).all()
    if n:  # d_ok is what wtp_crc32_verify_batch writes for the same ring
        ok2 = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        W.verify_batch(d, stride, r.t, n, ok2)
        torch.cuda.synchronize()
        assert torch.equal(ok2, ok[:n])
    assert W.device_status(0, clear=False) & DATA_ERROR_BITS == 0
    return want_ok, want_hit, want_acked, want_counts


def _plain_batch(rng, seq0, inflight, hi):
    """Valid ACKs for random slots below `hi`, one of them three times."""
    slots = rng.integers(0, hi, max(hi // 2, 1)).tolist() if hi > 0 else []
    if slots:
        slots += [slots[0]] * 2
    return [M.ack_datagram((seq0 + s) & M.M32) for s in slots]


def _mixed_batch(rng, seq0, inflight):
    """Every kind of datagram the ACK ring can hold, in a seeded random order."""
    pay = O.synth_fill_np(32, start_byte=inflight).tobytes()
    last = (seq0 + max(inflight, 1) - 1) & M.M32
    dg = _plain_batch(rng, seq0, inflight, inflight)
    dg += [M.ack_datagram(seq0, checksum=0x01000000),                    # a non-zero checksum
           M.ack_datagram((seq0 + inflight // 3) & M.M32, ptype=2),      # type DATA in the ACK ring
           M.ack_datagram(last)[:12],                                     # a 12-byte runt
           M.ack_datagram(last) + b"\0" * 1457,                           # recv_len 1473 > stride
           M.ack_datagram((seq0 - 1) & M.M32),                            # just below the window
           M.ack_datagram((seq0 + inflight) & M.M32),                     # counts in cumulative mode only
           M.ack_datagram((seq0 + inflight + 1) & M.M32),                 # past the window in both modes
           M.ack_datagram(last, checksum=O.crc32(pay), payload=pay),      # 48 bytes, payload CRC right
           M.ack_datagram((seq0 + inflight // 2) & M.M32, checksum=O.crc32(pay) ^ 0x80, payload=pay)]  # wrong
    return [dg[i] for i in rng.permutation(len(dg))]


@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
@pytest.mark.parametrize("seq0", [0, 0xFFFFFFF0])
@pytest.mark.parametrize("inflight", [0, 1, 63, 64, 65, 257, 1000])
def test_ingest_mixed_batches(W, mode, seq0, inflight):
    """Two batches on one window: plain ACKs (with duplicates) for its lower half, then the
    full mix; the state carries over."""
    rng = np.random.default_rng(inflight * 7 + mode)
    acked = (rng.random(inflight) < 0.2).astype(np.uint32)
    _, hit, acked, counts = ingest(W, *_ring(_plain_batch(rng, seq0, inflight, inflight // 2), STRIDE), STRIDE, mode,
                                   seq0, inflight, acked)
    if inflight >= 63:
        assert counts[1] > 0 and not acked.all()
    ok, hit, acked, counts = ingest(W, *_ring(_mixed_batch(rng, seq0, inflight), STRIDE), STRIDE, mode, seq0, inflight,
                                    acked)
    assert 0 < ok.sum() < ok.size and (hit == M.NOT_PLACED).any()
    if mode == M.CUMULATIVE:
        assert acked.all() and counts[0] == inflight  # the ACK of seq0 + inflight covers the window


@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
def test_ingest_strides_alignment_null_hit_and_empty_batch(W, mode):
    seq0, inflight = 0xFFFFFFFE, 130
    rng = np.random.default_rng(3 + mode)
    acked = np.zeros(inflight, dtype=np.uint32)
    acked[:5] = 1  # a pre-ACKed leading run: n == 0 still reports it
    none = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    _, _, acked, counts = ingest(W, none[0], none[1], 16, mode, seq0, inflight, acked)
    assert counts == (5, 0)
    # stride 16 (the 48-byte datagrams are then longer than their slot), a ring at byte
    # offset 4, d_hit NULL
    dg = _plain_batch(rng, seq0, inflight, 40) + _mixed_batch(rng, seq0, inflight)[:6]
    _, _, acked, _ = ingest(W, *_ring(dg, 16), 16, mode, seq0, inflight, acked, ring_off=4, with_hit=False)
    _, _, acked, _ = ingest(W, *_ring(_mixed_batch(rng, seq0, inflight), 48), 48, mode, seq0, inflight, acked, ring_off=4)
    # inflight == 0: nothing counts, d_counts = {0, 0}
    _, hit, _, counts = ingest(W, *_ring(_mixed_batch(rng, seq0, 0), STRIDE), STRIDE, mode, seq0, 0, np.zeros(0, np.uint32))
    assert counts == (0, 0) and (hit == M.NOT_PLACED).all()


def test_ingest_many_duplicates_across_workgroups(W):
    """5000 ACKs for 3 slots (many waves race for one word): the 0 -> 1 count is exact."""
    seqs = np.random.default_rng(1).choice([10, 11, 13], 5000)
    ring, rl = _ring([M.ack_datagram(int(s)) for s in seqs], 16)
    _, _, acked, counts = ingest(W, ring, rl, 16, M.SELECTIVE, 10, 8, np.array([0, 1, 0, 0, 0, 0, 0, 0], np.uint32))
    assert counts == (2, 2) and acked.tolist() == [1, 1, 0, 1, 0, 0, 0, 0]


# ---- select and emit -----------------------------------------------------------------------
class Source:
    """A synthetic file on the device, its host copy, and its wtp_build_data_packets wire
    image (what every retransmitted datagram must equal)."""

    def __init__(self, W, inflight, last_len, seq0, pay_off=0, host=True):
        self.inflight, self.seq0 = inflight, seq0
        self.total = (inflight - 1) * MAXP + last_len
        self.buf = torch.full((self.total + pay_off + 16,), 0xC3, dtype=torch.uint8, device="cuda")
        self.dev = self.buf[pay_off:pay_off + self.total]
        W.synth_fill(self.dev, seed=0x7E7 + inflight)
        self.image = torch.full((inflight, STRIDE), 0xA5, dtype=torch.uint8, device="cuda")
        W.build_data_packets(self.dev, self.total, seq0, self.image, STRIDE)
        self.image[inflight - 1, 16 + last_len:] = 0xA5  # a retransmitted short datagram leaves its slot's tail
        torch.cuda.synchronize()
        self.host = self.dev.cpu().numpy() if host else None


def retx(W, src, acked, sent, now, timeout, flags, max_sel, stride=STRIDE, wire_off=0, with_sel=True):
    """One wtp_tx_build_retransmit on the device and in the model from the same entry state;
    asserts every output equal and returns the model's (sel, sent, (emitted, due))."""
    cap, inflight = max_sel + 2, src.inflight  # two ring entries more than the call may use
    wbuf = torch.full((cap * stride + wire_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    wire = wbuf[wire_off:wire_off + cap * stride]
    sel, wlen, counts = Words(SENT, cap), Words(SENT, cap), Words(0x77777777, 2)
    d_acked, d_sent = Words(acked), Words(sent)
    W.tx_build_retransmit(src.dev, src.total, src.seq0, inflight, d_acked.t, d_sent.t, now, timeout, flags, wire, stride,
                          max_sel, sel.t if with_sel else None, wlen.t if with_sel else None, counts.t)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == ("k_tx_emit" if min(max_sel, inflight) else "k_tx_select")
    w_sel, w_dg, w_sent, (emitted, due) = M.retransmit(src.host, src.total, src.seq0, inflight, acked, sent, now, timeout,
                                                       flags, max_sel, build=src.host is not None)
    assert tuple(counts.get()) == (emitted, due)
    lens = np.minimum(MAXP, src.total - w_sel.astype(np.int64) * MAXP) + 16
    if with_sel:
        assert np.array_equal(sel.get(), np.concatenate([w_sel, np.full(cap - emitted, SENT, np.uint32)]))
        assert np.array_equal(wlen.get(), np.concatenate([lens.astype(np.uint32), np.full(cap - emitted, SENT, np.uint32)]))
    else:
        assert (sel.get() == SENT).all() and (wlen.get() == SENT).all()
    assert np.array_equal(d_sent.get(), w_sent) and np.array_equal(d_acked.get(), acked)
    rows = wire.view(cap, stride)
    assert (rows[emitted:] == 0xA5).all() and (rows[:, STRIDE:] == 0xA5).all()  # past the count / the datagram
    assert (wbuf[:wire_off] == 0xA5).all() and (wbuf[wbuf.numel() - 16:] == 0xA5).all()
    assert (src.buf[src.buf.numel() - 16:] == 0xC3).all()
    # byte-equal to the builder's wire image of the same buffer ...
    assert torch.equal(rows[:emitted, :STRIDE], src.image[torch.from_numpy(w_sel.astype(np.int64)).cuda()])
    if w_dg:  # ... and to the model's datagrams
        got = rows[:emitted].cpu().numpy()
        for k, d in enumerate(w_dg):
            assert got[k, :len(d)].tobytes() == d
    if emitted:  # ... and intact for a receiver
        ok = torch.zeros(emitted, dtype=torch.uint8, device="cuda")
        ring = rows[:emitted].contiguous()
        W.verify_batch(ring, stride, torch.from_numpy(_s32(lens)).cuda(), emitted, ok)
        torch.cuda.synchronize()
        assert bool(ok.all())
    assert W.device_status(0, clear=False) & DATA_ERROR_BITS == 0
    return w_sel, w_sent, (emitted, due)


NOW, TIMEOUT = 0x100, 500  # the clock has just wrapped: every stale timer lies before 2^32


def _state(inflight, due_mask):
    """Window state in which exactly `due_mask` is due at NOW: the other slots are ACKed
    (odd) or were sent exactly TIMEOUT ms ago (even), which is not yet due."""
    s = np.arange(inflight)
    acked = np.where(due_mask, 0, s & 1).astype(np.uint32)
    age = np.where(due_mask, TIMEOUT + 1 + (s % 7) * 1000, np.where(s & 1, 5000, TIMEOUT))
    return acked, ((NOW - age) & M.M32).astype(np.uint32)


BLOCK_EDGES = (1023, 1024, 1025, 2049)  # around the 1024-slot blocks of k_tx_count / k_tx_select


def _fractions(inflight):
    s = np.arange(inflight)
    if inflight in BLOCK_EDGES:  # a sparse and a dense due set
        return {"hundredth": np.random.default_rng(inflight).random(inflight) < 0.01, "all": s >= 0}
    return {"none": s < 0, "one": s == inflight * 2 // 3, "alternate": s % 2 == 0,
            "tenth": np.random.default_rng(inflight).random(inflight) < 0.1, "all": s >= 0}


LAST_LEN = {1: 1, 64: 15, 65: 16, 256: 17, 257: 1455, 1000: 1, 1023: 1456, 1024: 1, 1025: 16, 2049: 15, 70000: 15}


@pytest.mark.parametrize("inflight", sorted(LAST_LEN))
def test_select_and_emit(W, inflight):
    """Due fractions x ring sizes; 70 000 slots cross 69 scan blocks, and the windows of
    BLOCK_EDGES end one slot before, at and one slot after a block's end (above 1000 slots
    the bytes are compared with the builder's wire image on the device only)."""
    seq0 = 0xFFFFFFF0 if inflight % 2 else 7
    src = Source(W, inflight, LAST_LEN[inflight], seq0, host=inflight <= 1000)
    for name, mask in _fractions(inflight).items():
        acked, sent = _state(inflight, mask)
        due = int(mask.sum())
        full = inflight <= 2049 or name == "tenth"  # the 100 MB window: every ring size at one fraction only
        for max_sel in sorted({0, 1, max(due - 1, 0), due, due + 7} if full else {due + 7}):
            sel, sent2, (emitted, got_due) = retx(W, src, acked, sent, NOW, TIMEOUT, 0, max_sel)
            assert got_due == due and emitted == min(due, max_sel), (name, max_sel)
            assert np.array_equal(sel, np.flatnonzero(mask)[:emitted])
            # only the emitted slots' timers moved
            assert np.array_equal(np.flatnonzero(sent2 != sent), sel)
        if 0 < due and full:  # a ring one short: the caller calls again and gets the rest
            _, sent2, _ = retx(W, src, acked, sent, NOW, TIMEOUT, 0, max(due - 1, 1))
            sel, _, counts = retx(W, src, acked, sent2, NOW, TIMEOUT, 0, due)
            assert counts == ((1, 1) if due > 1 else (0, 0)) and sel.tolist() == np.flatnonzero(mask)[due - 1:due][:counts[0]].tolist()


@pytest.mark.parametrize("last_len", [1, 15, 16, 17, 1455, 1456])
@pytest.mark.parametrize("pay_off,wire_off,stride", [(0, 0, 1472), (1, 0, 1472), (0, 1, 1472), (0, 0, 1473), (0, 0, 1504),
                                                     (1, 1, 1473)])
def test_last_chunk_lengths_and_alignment(W, last_len, pay_off, wire_off, stride):
    """The 16-B vector path and the bytewise path (payload or wire at byte offset 1, stride
    1473) give the same bytes, for every tail length of the short last chunk."""
    src = Source(W, 5, last_len, 0xFFFFFFFD, pay_off=pay_off)
    acked, sent = _state(5, np.arange(5) != 1)
    sel, _, counts = retx(W, src, acked, sent, NOW, TIMEOUT, 0, 5, stride=stride, wire_off=wire_off)
    assert counts == (4, 4) and sel.tolist() == [0, 2, 3, 4]


def test_timers_flags_and_null_outputs(W):
    inflight = 100
    src = Source(W, inflight, 100, 0)
    fresh = np.full(inflight, 0x100, np.uint32)
    acked = (np.arange(inflight) % 3 == 0).astype(np.uint32)
    # all timers fresh: nothing is due, with WTP_RETX_ALL every un-ACKed slot is
    assert retx(W, src, acked, fresh, 0x100, TIMEOUT, 0, inflight)[2] == (0, 0)
    sel, _, counts = retx(W, src, acked, fresh, 0x100, TIMEOUT, M.RETX_ALL, inflight)
    assert counts == (66, 66) and np.array_equal(sel, np.flatnonzero(acked == 0))
    # clock wrap: sent at 0xFFFFFF00, now 0x100, 0x200 = 512 ms elapsed; a timeout of
    # exactly the elapsed time is not due
    old = np.full(inflight, 0xFFFFFF00, np.uint32)
    assert retx(W, src, acked, old, 0x100, 511, 0, inflight)[2] == (66, 66)
    assert retx(W, src, acked, old, 0x100, 512, 0, inflight)[2] == (0, 0)
    # d_sel and d_wire_len NULL
    assert retx(W, src, acked, old, 0x100, TIMEOUT, 0, 10, with_sel=False)[2] == (10, 66)


# ---- graph capture ---------------------------------------------------------------------------
def test_graph_replay(W):
    """ingest + build-retransmit captured into one graph on a side stream, replayed twice
    from different states and ACK batches: both replays match the model."""
    inflight, seq0, n, max_sel, now = 300, 0xFFFFFF00, 200, 64, 5000
    src = Source(W, inflight, 99, seq0)
    rng = np.random.default_rng(11)
    ring_t = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    rl_t = torch.full((n,), 16, dtype=torch.int32, device="cuda")
    acked_t = torch.zeros(inflight, dtype=torch.int32, device="cuda")
    sent_t = torch.zeros(inflight, dtype=torch.int32, device="cuda")
    ok_t = torch.zeros(n, dtype=torch.uint8, device="cuda")
    hit_t = torch.zeros(n, dtype=torch.int32, device="cuda")
    c1, c2 = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    wire = torch.zeros(max_sel * STRIDE, dtype=torch.uint8, device="cuda")
    sel_t, wlen_t = torch.zeros(max_sel, dtype=torch.int32, device="cuda"), torch.zeros(max_sel, dtype=torch.int32, device="cuda")
    work = torch.zeros(W.tx_work_bytes(inflight, max_sel), dtype=torch.uint8, device="cuda")

    def call():
        W.tx_ingest_acks(ring_t, 16, rl_t, n, M.SELECTIVE, seq0, inflight, acked_t, ok_t, hit_t, c1)
        W.tx_build_retransmit(src.dev, src.total, seq0, inflight, acked_t, sent_t, now, TIMEOUT, 0, wire, STRIDE, max_sel,
                              sel_t, wlen_t, c2, work=work)

    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):
        call()
    cs.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        call()
    for salt in (1, 2):
        acked = (rng.random(inflight) < 0.3).astype(np.uint32)
        sent = (now - rng.integers(0, 1000, inflight)).astype(np.uint32)
        seqs = (seq0 + rng.integers(-2, inflight + 2, n)) & M.M32
        ring, rl = M.make_ring([M.ack_datagram(int(s), checksum=int(k % 13 == 0)) for k, s in enumerate(seqs)], 16)
        ring_t.copy_(torch.from_numpy(ring))
        acked_t.copy_(torch.from_numpy(_s32(acked)))
        sent_t.copy_(torch.from_numpy(_s32(sent)))
        wire.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        w_ok, w_hit, w_acked, w_c1 = M.ingest(ring, 16, rl, M.SELECTIVE, seq0, inflight, acked)
        w_sel, w_dg, w_sent, w_c2 = M.retransmit(src.host, src.total, seq0, inflight, w_acked, sent, now, TIMEOUT, 0, max_sel)
        u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        assert np.array_equal(ok_t.cpu().numpy(), w_ok) and np.array_equal(u(hit_t), w_hit)
        assert np.array_equal(u(acked_t), w_acked) and tuple(u(c1)) == w_c1 and tuple(u(c2)) == w_c2
        assert np.array_equal(u(sent_t), w_sent) and np.array_equal(u(sel_t)[:w_c2[0]], w_sel)
        got = wire.view(max_sel, STRIDE).cpu().numpy()
        assert 0 < w_c2[0] and all(got[k, :len(d)].tobytes() == d for k, d in enumerate(w_dg))
        assert (got[w_c2[0]:] == 0xA5).all()
    assert W.device_status(0, clear=False) & DATA_ERROR_BITS == 0


# ---- end to end on the device -------------------------------------------------------------------
class DevEnd:
    """Both windows on the device, behind the calls of retx_model.transfer: no payload byte
    crosses to the host (it reads back verdicts, 8 header bytes per datagram and counts)."""

    def __init__(self, W, src, total, nchunks, window, seq_base):
        self.W, self.src, self.total, self.window, self.seq_base = W, src, total, window, seq_base
        z = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        self.acked, self.sent, self.slot_len = z(nchunks + window), z(nchunks + window), z(nchunks + window, -1)
        self.img = torch.full(((nchunks + window) * MAXP,), 0xA5, dtype=torch.uint8, device="cuda")
        self.counts, self.ack = z(2), z(1)
        self.retx_wire = torch.zeros((0, STRIDE), dtype=torch.uint8, device="cuda")
        self.retx_len = z(0)

    def seq(self, chunk):
        return (self.seq_base + chunk) & M.M32

    def send(self, c0, cnt, now):
        wire = torch.zeros((cnt, STRIDE), dtype=torch.uint8, device="cuda")
        wlen = torch.zeros(cnt, dtype=torch.int32, device="cuda")
        if cnt:
            nbytes = min(self.total, (c0 + cnt) * MAXP) - c0 * MAXP
            self.W.build_data_packets(self.src[c0 * MAXP:], nbytes, self.seq(c0), wire, STRIDE, wlen)
            self.sent[c0:c0 + cnt] = int(_s32([now])[0])
        self.wire, self.wlen = torch.cat([wire, self.retx_wire]), torch.cat([wlen, self.retx_len])
        return self.wire.shape[0]

    def accept(self, idx, rbase):
        n = idx.size
        sel = torch.from_numpy(idx.astype(np.int64)).cuda()
        ring, rl = self.wire[sel].contiguous(), self.wlen[sel].contiguous()
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.W.accept_data_packets(ring if n else ok, STRIDE, rl if n else self.ack, n, self.seq(rbase), self.window,
                                   self.img[rbase * MAXP:], self.slot_len[rbase:], ok, None, self.ack)
        hdr = np.ascontiguousarray(ring[:, :8].cpu().numpy()).reshape(n, 8).view(">u4")
        return (ok[:n].cpu().numpy(), hdr[:, 0].astype(np.uint32), hdr[:, 1].astype(np.uint32),
                int(self.ack.cpu().numpy().view(np.uint32)[0]))

    def ingest(self, acks, mode, sbase, inflight):
        ring, rl = M.make_ring(acks, 16)
        n = rl.size
        d = torch.from_numpy(ring).cuda()
        r = torch.from_numpy(_s32(rl)).cuda() if n else self.ack
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        self.W.tx_ingest_acks(d, 16, r, n, mode, self.seq(sbase), inflight, self.acked[sbase:], ok, None, self.counts)
        return int(self.counts[0].item())

    def retransmit(self, sbase, inflight, now, timeout, flags, max_sel):
        wire = torch.zeros((max_sel, STRIDE), dtype=torch.uint8, device="cuda")
        sel, wlen = (torch.zeros(max_sel, dtype=torch.int32, device="cuda") for _ in range(2))
        self.W.tx_build_retransmit(self.src[sbase * MAXP:], self.total - sbase * MAXP, self.seq(sbase), inflight,
                                   self.acked[sbase:], self.sent[sbase:], now, timeout, flags, wire, STRIDE, max_sel, sel,
                                   wlen, self.counts)
        e = int(self.counts[0].item())
        self.retx_wire, self.retx_len = wire[:e], wlen[:e]
        return sel[:e].cpu().numpy()


@pytest.mark.parametrize("mode,seq_base", [(M.SELECTIVE, 0), (M.SELECTIVE, 0xFFFFFF80), (M.CUMULATIVE, 0),
                                           (M.CUMULATIVE, 0xFFFFFF80)])
def test_end_to_end_transfer_on_the_device(W, mode, seq_base):
    """build -> lossy channel -> accept -> lossy ACK channel -> ingest -> retransmit -> shift
    until the sender's base reaches the end, against the model driving the same loop with
    the same seeds: the same number of rounds (the model needs 33 in selective and 25 in
    cumulative mode; the loop fails at 40), the same retransmit set every round, an exact
    image and whole-file CRC at the receiver."""
    nchunks, window = M.E2E_CHUNKS, M.E2E_WINDOW
    total = nchunks * MAXP - M.E2E_SHORT
    host = O.synth_fill_np(total, seed=M.E2E_SEED)
    want_rounds, want_sets = M.transfer(M.ModelEnd(host, nchunks, window, seq_base), nchunks, window, seq_base, mode,
                                        M.E2E_SEED, M.E2E_LOSS)
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=M.E2E_SEED)
    end = DevEnd(W, src, total, nchunks, window, seq_base)
    rounds, sets = M.transfer(end, nchunks, window, seq_base, mode, M.E2E_SEED, M.E2E_LOSS)
    assert rounds == want_rounds and sets == want_sets
    assert torch.equal(end.img[:total], src) and bool((end.img[total:nchunks * MAXP] == 0xA5).all())
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(end.img, total, crc)
    assert int(crc.cpu().numpy().view(np.uint32)[0]) == O.crc32(host)
    assert W.device_status(0, clear=False) & DATA_ERROR_BITS == 0
