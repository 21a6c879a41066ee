"""GPU tests of the device-side sender window, wtp_tx_ingest_acks and
wtp_tx_build_retransmit: every output is compared element-wise with the sequential model
(tests/retx_model.py) from the same entry state, and the state is carried across calls.
Buffers are pre-filled with sentinels (0xA5 wire, 12345 in sel / hit / wire_len) and have
16 guard bytes past their end, so a byte that must stay untouched is checkable.  Windows
above about 3000 slots, up to WTP_TX_MAX_INFLIGHT, are compared with the model's vectorised
path, and the largest ones also with themselves (split, order and paging invariance)."""
import numpy as np
import pytest

import oracle as O
import retx_model as M
from gpu_support import W  # noqa: F401 (fixture)
from gpu_support import DATA_ERROR_BITS, Bytes, DevEnd, Words, assert_no_data_error, capture, dev_s32, s32, u32
from gpu_support import datagram_ring as _ring

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, STRIDE, SENT = M.MAXP, M.STRIDE, 12345


# ---- ingest --------------------------------------------------------------------------------
def dev_ingest(W, ring, rl, stride, mode, seq0, inflight, acked, ring_off=0, with_hit=True):
    """One wtp_tx_ingest_acks from the entry state `acked` (numpy), with the guard and
    untouched-input checks; returns the device's (ok, hit, acked, counts) as numpy."""
    n = rl.size
    dbuf = Bytes(ring, off=ring_off)  # 16 guard bytes (0xC3) after it
    d = dbuf.t
    r, ok, hit = Words(rl), torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda"), Words(SENT, n)
    st, counts = Words(acked), Words(0x77777777, 2)
    W.tx_ingest_acks(d, stride, r.t, n, mode, seq0, inflight, st.t, ok, hit.t if with_hit else None, counts.t)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == ("k_tx_lead" if mode == M.SELECTIVE else "k_tx_window")
    got_ok = ok.cpu().numpy()
    assert (got_ok[n:] == 7).all()
    assert np.array_equal(r.get(), rl)
    assert np.array_equal(dbuf.get(), ring)  # the ring is only read
    # this call alone never sets a data-error flag, whatever the ring holds
    assert_no_data_error(W)
    if n:  # d_ok is what wtp_crc32_verify_batch writes for the same ring
        ok2 = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        W.verify_batch(d, stride, r.t, n, ok2)
        torch.cuda.synchronize()
        assert torch.equal(ok2, ok[:n])
    # verify flags an in-slot payload above WTP_MAX_KERNEL_LEN (bit 0), and nothing else here
    over = bool(((rl >= 16) & (rl <= stride) & (rl.astype(np.int64) - 16 > M.MAX_KERNEL_LEN)).any())
    assert W.device_status(0, clear=over) & DATA_ERROR_BITS == (1 if over else 0)
    return got_ok[:n], hit.get(), st.get(), tuple(int(c) for c in counts.get())


def ingest(W, ring, rl, stride, mode, seq0, inflight, acked, ring_off=0, with_hit=True, vectorised=False):
    """One call on the device and in the model from the same entry state `acked` (numpy);
    asserts every output equal; returns the model's (ok, hit, acked, counts).  `vectorised`:
    the model's numpy path, for windows too large for its literal loop."""
    got_ok, got_hit, got_acked, got_counts = dev_ingest(W, ring, rl, stride, mode, seq0, inflight, acked, ring_off, with_hit)
    want_ok, want_hit, want_acked, want_counts = M.ingest(ring, stride, rl, mode, seq0, inflight, acked, vectorised=vectorised)
    assert np.array_equal(got_ok, want_ok)
    assert np.array_equal(got_hit, want_hit if with_hit else np.full(rl.size, SENT, np.uint32))
    assert np.array_equal(got_acked, want_acked)
    assert got_counts == want_counts
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
        self.inflight, self.seq0, self.seed = inflight, seq0, 0x7E7 + inflight
        self.total = (inflight - 1) * MAXP + last_len
        self.buf = torch.full((self.total + pay_off + 16,), 0xC3, dtype=torch.uint8, device="cuda")
        self.dev = self.buf[pay_off:pay_off + self.total]
        W.synth_fill(self.dev, seed=self.seed)
        self.image = torch.full((inflight, STRIDE), 0xA5, dtype=torch.uint8, device="cuda")
        W.build_data_packets(self.dev, self.total, seq0, self.image, STRIDE)
        self.image[inflight - 1, 16 + last_len:] = 0xA5  # a retransmitted short datagram leaves its slot's tail
        torch.cuda.synchronize()
        self.host = self.dev.cpu().numpy() if host else None


def retx(W, src, acked, sent, now, timeout, flags, max_sel, stride=STRIDE, wire_off=0, with_sel=True, vectorised=False,
         oracle=False, keep=None):
    """One wtp_tx_build_retransmit on the device and in the model from the same entry state;
    asserts every output equal and returns the model's (sel, sent, (emitted, due)).
    `vectorised`: the model's numpy path.  `oracle`: every emitted datagram is also compared
    with the oracle's, built from the generator's bytes of its slot (for sources without a
    host copy).  `keep`: a list that receives the device's (sel, datagrams, timers)."""
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
                                                       flags, max_sel, build=src.host is not None, vectorised=vectorised)
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
    if oracle:  # ... and to the oracle's, from the generator's bytes of each slot
        got = rows[:emitted].cpu().numpy()
        for k, s in enumerate(w_sel.tolist()):
            d = O.build_datagram((src.seq0 + s) & M.M32, O.synth_fill_np(int(lens[k]) - 16, start_byte=s * MAXP, seed=src.seed))
            assert got[k, :len(d)].tobytes() == d, (k, s)
    if keep is not None:
        keep.append((sel.get()[:emitted], rows[:emitted, :STRIDE].clone(), d_sent.get()))
    if emitted:  # ... and intact for a receiver
        ok = torch.zeros(emitted, dtype=torch.uint8, device="cuda")
        ring = rows[:emitted].contiguous()
        W.verify_batch(ring, stride, dev_s32(lens), emitted, ok)
        torch.cuda.synchronize()
        assert bool(ok.all())
    assert_no_data_error(W)
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

    g, _ = capture(call)
    for salt in (1, 2):
        acked = (rng.random(inflight) < 0.3).astype(np.uint32)
        sent = (now - rng.integers(0, 1000, inflight)).astype(np.uint32)
        seqs = (seq0 + rng.integers(-2, inflight + 2, n)) & M.M32
        ring, rl = M.make_ring([M.ack_datagram(int(s), checksum=int(k % 13 == 0)) for k, s in enumerate(seqs)], 16)
        ring_t.copy_(torch.from_numpy(ring))
        acked_t.copy_(torch.from_numpy(s32(acked)))
        sent_t.copy_(torch.from_numpy(s32(sent)))
        wire.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        w_ok, w_hit, w_acked, w_c1 = M.ingest(ring, 16, rl, M.SELECTIVE, seq0, inflight, acked)
        w_sel, w_dg, w_sent, w_c2 = M.retransmit(src.host, src.total, seq0, inflight, w_acked, sent, now, TIMEOUT, 0, max_sel)
        assert np.array_equal(ok_t.cpu().numpy(), w_ok) and np.array_equal(u32(hit_t), w_hit)
        assert np.array_equal(u32(acked_t), w_acked) and tuple(u32(c1)) == w_c1 and tuple(u32(c2)) == w_c2
        assert np.array_equal(u32(sent_t), w_sent) and np.array_equal(u32(sel_t)[:w_c2[0]], w_sel)
        got = wire.view(max_sel, STRIDE).cpu().numpy()
        assert 0 < w_c2[0] and all(got[k, :len(d)].tobytes() == d for k, d in enumerate(w_dg))
        assert (got[w_c2[0]:] == 0xA5).all()
    assert_no_data_error(W)


# ---- end to end on the device -------------------------------------------------------------------
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
    assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)


# ---- ingest at the sizes where its kernels change behaviour -----------------------------------
# csrc/wtp_tx.hip: kTxBlock = 1024 lanes in k_tx_window's one workgroup (its fill loop steps by
# it), kTxScan * kTxBlock = 16 * 1024 slots per round of its leading-run scan, and k_tx_lead's
# grid of at most 1024 blocks x 256 lanes (its strided loop takes a second step above that).
TX_BLOCK = 1024
TX_SCAN_ROUND = 16 * 1024
TX_LEAD_GRID = 1024 * 256
MAX_INFLIGHT = 1 << 20  # WTP_TX_MAX_INFLIGHT


def _seq0(inflight, wrap):
    """7, or a seq0 whose window wraps 2^32 a third of the way in."""
    return (-(inflight // 3 + 1)) & M.M32 if wrap else 7


def _ack_ring(seqs):
    """(ring, recv_len) of plain 16-byte ACKs with these seqNums at stride 16, without a loop."""
    h = np.zeros((len(seqs), 4), dtype=">u4")
    h[:, 0] = 3
    h[:, 1] = np.asarray(seqs, dtype=np.int64) & M.M32
    return h.view(np.uint8).reshape(-1).copy(), np.full(len(seqs), 16, dtype=np.uint32)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("inflight,top,steps", [(1023, 1023, 1), (1023, 511, 1), (1024, 1024, 1), (1024, 512, 1),
                                                (1025, 1025, 2), (1025, 513, 1), (2049, 2049, 3), (2049, 1025, 2)])
def test_ingest_cumulative_fill_steps(W, inflight, top, steps, wrap):
    """k_tx_window's fill loop around its 1024-lane stride: the batch's largest ACK at the
    window's end and at about its half, over a window with a fifth of its slots ACKed before,
    so that d_counts[1] is the number of zeros filled and not the largest ACK.  Against the
    model's literal loop."""
    rng = np.random.default_rng(inflight * 3 + top)
    seq0 = _seq0(inflight, wrap)
    acked = (rng.random(inflight) < 0.2).astype(np.uint32)
    a = rng.integers(1, top + 1, 200)
    a[int(rng.integers(0, 200))] = top
    ring, rl = _ack_ring(seq0 + a)
    _, hit, after, counts = ingest(W, ring, rl, 16, M.CUMULATIVE, seq0, inflight, acked)
    zeros = int((acked[:top] == 0).sum())
    assert int(hit.max()) == top and -(-top // TX_BLOCK) == steps  # lane 0 takes `steps` steps
    assert counts[1] == zeros and 0 < zeros < top
    assert after[:top].all() and np.array_equal(after[top:], acked[top:])


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("top", [5, 1500])
def test_ingest_cumulative_scan_rounds(W, top, wrap):
    """k_tx_window's leading-run scan in rounds of 16 384 slots from the largest ACK: the
    first un-ACKed slot one before, at and one past the end of the first round and in the
    fourth, then windows that are fully ACKed after the call and end exactly at, one past
    and further past a round's end."""
    rng = np.random.default_rng(top)
    R = TX_SCAN_ROUND
    a = rng.integers(1, top + 1, 40)
    a[7] = top
    for gap, rounds_before in ((R - 1, 0), (R, 1), (R + 1, 1), (3 * R + 7, 3)):
        first = top + gap
        inflight = first + 778
        seq0 = _seq0(inflight, wrap)
        acked = (rng.random(inflight) < 0.5).astype(np.uint32)
        acked[:top] = rng.random(top) < 0.2
        acked[top:first], acked[first] = 1, 0
        _, _, _, counts = ingest(W, *_ack_ring(seq0 + a), 16, M.CUMULATIVE, seq0, inflight, acked, vectorised=True)
        # the run ends in the round the case is for: `rounds_before` whole rounds hold no un-ACKed slot
        assert counts[0] == first and (counts[0] - top) // R == rounds_before
        assert counts[1] == int((acked[:top] == 0).sum()) > 0
    for rest in (R, R + 1, 2 * R, 3 * R + 1):
        inflight = top + rest
        seq0 = _seq0(inflight, wrap)
        acked = np.ones(inflight, dtype=np.uint32)
        acked[:top] = rng.random(top) < 0.2
        _, _, after, counts = ingest(W, *_ack_ring(seq0 + a), 16, M.CUMULATIVE, seq0, inflight, acked, vectorised=True)
        assert counts == (inflight, int((acked[:top] == 0).sum())) and after.all() and not acked.all()


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("inflight", [TX_LEAD_GRID - 1, TX_LEAD_GRID, TX_LEAD_GRID + 1, MAX_INFLIGHT])
def test_ingest_selective_lead_pass(W, inflight, wrap):
    """k_tx_lead around the window size at which its grid stops growing (1024 blocks x 256
    lanes) and its loop takes a second step: the first un-ACKed slot at the edges of the
    first block, of the grid and of the window, and nowhere.  The slots before it include
    some that only this batch ACKs (the one just before it too), so the run depends on the
    call's own marks."""
    seq0 = _seq0(inflight, wrap)
    firsts = [f for f in dict.fromkeys([0, 255, 256, TX_LEAD_GRID - 1, TX_LEAD_GRID, inflight - 1]) if f < inflight]
    for first in firsts + [None]:
        rng = np.random.default_rng(inflight + (first or 0))
        end = inflight if first is None else first
        acked = np.ones(inflight, dtype=np.uint32)
        pend = np.unique(np.append(rng.integers(0, end, 64), end - 1)) if end else np.zeros(0, np.int64)
        acked[pend] = 0
        above = np.zeros(0, np.int64)
        if first is not None:
            acked[first + 1:] = rng.random(inflight - first - 1) < 0.5
            acked[first] = 0
            if first + 1 < inflight:
                above = rng.integers(first + 1, inflight, 64)
        slots = np.concatenate([pend, pend[:5], above])
        slots = slots[rng.permutation(slots.size)]
        _, hit, after, counts = ingest(W, *_ack_ring(seq0 + slots), 16, M.SELECTIVE, seq0, inflight, acked, vectorised=True)
        assert counts[0] == end and counts[1] >= pend.size and (first is None or after[first] == 0)
        assert np.array_equal(hit, slots)  # every ACK of the batch counts
    assert inflight - 1 in firsts and (TX_LEAD_GRID in firsts) == (inflight > TX_LEAD_GRID)


def _max_batch(mode, wrap, seed, n=300_000):
    """A window of WTP_TX_MAX_INFLIGHT slots, a fifth of them and a run of 20 000 above the
    batch's largest ACK pre-ACKed, and n plain ACKs in random order: 189 500 below `top`,
    100 000 copies of some of these, 500 of `top` itself, and 5 000 each below and past the
    window.  Returns (ring, recv_len, seq0, acked, top)."""
    rng = np.random.default_rng(seed)
    inflight, top = MAX_INFLIGHT, MAX_INFLIGHT - 54321
    seq0 = _seq0(inflight, wrap)
    acked = (rng.random(inflight) < 0.2).astype(np.uint32)
    acked[top:top + 20000] = 1
    acked[0], acked[top + 20000] = 1, 0  # no ACK names slot 0: the selective run starts past it
    base = rng.integers(1, top, n - 110_500)
    d = np.concatenate([base, rng.choice(base, 100_000), np.full(500, top), rng.integers(-5000, 0, 5000),
                        rng.integers(inflight + 1, inflight + 5001, 5000)])
    ring, rl = _ack_ring(seq0 + d[rng.permutation(n)])
    return ring, rl, seq0, acked, top


def _max_batch_properties(mode, hit, acked, top, counts):
    """What the 2^20 cases exist for, from the model's (or the device's) outputs alone."""
    n, counting = hit.size, hit != M.NOT_PLACED
    assert counting.sum() - np.unique(hit[counting]).size > n // 4  # duplicates inside the batch
    assert (~counting).sum() > n // 50  # below or past the window
    assert -(-n // 256) > 1000  # blocks of k_tx_ingest
    if mode == M.CUMULATIVE:
        assert int(hit[counting].max()) == top > TX_BLOCK
        assert np.unique(np.flatnonzero(hit == top) // 256).size > 256  # the largest ACK in many blocks
        assert counts[1] == int((acked[:top] == 0).sum()) and counts[0] == top + 20000
        assert counts[0] - top >= TX_SCAN_ROUND  # the run ends beyond the first scan round
    else:
        marks = np.unique(hit[counting])
        assert counts[1] == int((acked[marks] == 0).sum()) and 0 < counts[0] < TX_BLOCK


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
def test_ingest_max_inflight_contended(W, mode, wrap):
    """300 000 ACKs (about 1200 blocks of k_tx_ingest) over the largest window: a third of
    them duplicates of another datagram of the batch, so the atomicCAS / atomicAdd (selective)
    and the atomicMax (cumulative) are contended and d_counts[1] must still be exact."""
    ring, rl, seq0, acked, top = _max_batch(mode, wrap, 0xACC + mode)
    _, hit, _, counts = ingest(W, ring, rl, 16, mode, seq0, MAX_INFLIGHT, acked, vectorised=True)
    _max_batch_properties(mode, hit, acked, top, counts)


# ---- model-free invariants: "equals processing the datagrams one by one in index order" -----
@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
def test_ingest_split_and_order_invariance(W, mode):
    """On the device alone: one call over A || B leaves the window that a call over A and then
    one over B on the carried state leave, d_counts[1] adds up, d_ok and d_hit concatenate;
    and a permuted batch leaves the same window with d_hit permuted."""
    ring, rl, seq0, acked, top = _max_batch(mode, True, 0x5B17 + mode)
    n, inflight = rl.size, MAX_INFLIGHT
    ok, hit, after, counts = dev_ingest(W, ring, rl, 16, mode, seq0, inflight, acked)
    _max_batch_properties(mode, hit, acked, top, counts)
    for cut in (1, n // 2, n - 1):
        ok_a, hit_a, mid, c_a = dev_ingest(W, ring[:cut * 16], rl[:cut], 16, mode, seq0, inflight, acked)
        ok_b, hit_b, end, c_b = dev_ingest(W, ring[cut * 16:], rl[cut:], 16, mode, seq0, inflight, mid)
        assert np.array_equal(end, after) and c_b[0] == counts[0] and c_a[1] + c_b[1] == counts[1]
        assert np.array_equal(np.concatenate([ok_a, ok_b]), ok) and np.array_equal(np.concatenate([hit_a, hit_b]), hit)
    perm = np.random.default_rng(5).permutation(n)
    ok_p, hit_p, after_p, c_p = dev_ingest(W, ring.reshape(n, 16)[perm].reshape(-1), rl[perm], 16, mode, seq0, inflight, acked)
    assert np.array_equal(after_p, after) and c_p == counts
    assert np.array_equal(ok_p, ok[perm]) and np.array_equal(hit_p, hit[perm])


# ---- the payload-length limit in the ACK ring ---------------------------------------------------
@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("stride", [4128, 5000, 16384])
def test_ingest_payload_limit(W, stride, off, mode):
    """ACK-typed datagrams with payloads of 0 .. 4097 and stride - 16 bytes (retx_model.
    limit_corpus): ingest hashes up to WTP_MAX_KERNEL_LEN bytes itself, a longer payload is
    not ok; d_ok is byte-equal to wtp_crc32_verify_batch's on the same ring (the braided
    launch's fix-up at strides 4128 and 16 384 with a 16-B aligned base, the general kernel
    otherwise), and only verify sets status bit 0 (dev_ingest asserts both)."""
    W.device_status(0, clear=True)
    seq0, inflight = M.M32, 513  # seqNum s is slot s + 1: it counts in both modes
    for over in (True, False):
        dg, lens = M.limit_corpus(stride, 3, 330, stride + off, 512, over=over)
        ring, rl = M.make_ring(dg, stride)
        ok, hit, _, _ = ingest(W, ring, rl, stride, mode, seq0, inflight, np.zeros(inflight, np.uint32), ring_off=off)
        assert ((lens > M.MAX_KERNEL_LEN).sum() > 0) == over and np.array_equal(rl, lens + 16)
        assert not ok[lens > M.MAX_KERNEL_LEN].any() and np.array_equal(hit != M.NOT_PLACED, ok != 0)
        for ln in (0, 1, 3, 4, 255, MAXP, MAXP + 1, 4095, 4096):  # the 30 intact ones of each length count
            assert (hit[lens == ln] != M.NOT_PLACED).sum() == 30 and (lens == ln).sum() == 30 + (ln > MAXP)


# ---- retransmit at 1023 and 1024 select blocks ---------------------------------------------------
def _sparse_due(inflight):
    """About 1500 random slots, slot 0, the last slot and both sides of the last three block
    edges of k_tx_count / k_tx_select."""
    mask = np.zeros(inflight, dtype=bool)
    mask[np.random.default_rng(inflight).integers(0, inflight, 1500)] = True
    mask[[0, inflight - 1]] = True
    for e in ((inflight - 1) // TX_BLOCK - np.arange(3)) * TX_BLOCK:
        mask[[e - 1, e]] = True
    return mask


@pytest.fixture(scope="module")
def src_max(W):
    src = Source(W, MAX_INFLIGHT, 15, 0xFFFFFFF0, host=False)
    yield src
    del src.buf, src.dev, src.image
    torch.cuda.empty_cache()


def _retx_block_limit(W, src):
    inflight = src.inflight
    nblk = -(-inflight // TX_BLOCK)
    s = np.arange(inflight)
    # sparse: timers, every ring size, and the bytes against the oracle as well
    mask = _sparse_due(inflight)
    acked, sent = _state(inflight, mask)
    due = int(mask.sum())
    assert 1400 < due < 1510 and mask[(nblk - 1) * TX_BLOCK - 1] and mask[(nblk - 1) * TX_BLOCK]
    for max_sel in (due, due - 1, 7):
        sel, sent2, counts = retx(W, src, acked, sent, NOW, TIMEOUT, 0, max_sel, vectorised=True, oracle=True)
        assert counts == (max_sel, due) and np.array_equal(sel, np.flatnonzero(mask)[:max_sel])
        assert np.array_equal(np.flatnonzero(sent2 != sent), sel)  # only the emitted slots' timers moved
    # every un-ACKed slot under WTP_RETX_ALL, a ring of 64 (and of 7)
    rng = np.random.default_rng(inflight + 1)
    acked = (rng.random(inflight) < 0.5).astype(np.uint32)
    sent = rng.integers(0, 1 << 32, inflight, dtype=np.uint64).astype(np.uint32)
    due = int((acked == 0).sum())
    for max_sel in (64, 7):
        sel, sent2, counts = retx(W, src, acked, sent, NOW, TIMEOUT, M.RETX_ALL, max_sel, vectorised=True)
        assert counts == (max_sel, due) and due > inflight // 3 and np.array_equal(sel, np.flatnonzero(acked == 0)[:max_sel])
        assert np.array_equal(np.flatnonzero(sent2 != sent), sel[sent[sel] != NOW])
    # dense: the last full block and the partial one after it
    mask = s >= (inflight // TX_BLOCK - 1) * TX_BLOCK
    acked, sent = _state(inflight, mask)
    due = int(mask.sum())
    assert due == TX_BLOCK + inflight % TX_BLOCK
    for max_sel in (due, due - 1, 7):
        sel, sent2, counts = retx(W, src, acked, sent, NOW, TIMEOUT, 0, max_sel, vectorised=True)
        assert counts == (max_sel, due) and np.array_equal(sel, np.flatnonzero(mask)[:max_sel])
        assert np.array_equal(np.flatnonzero(sent2 != sent), sel)


@pytest.mark.parametrize("inflight,last_len,nblk", [(MAX_INFLIGHT - 1024, 1, 1023), (MAX_INFLIGHT - 1023, 16, 1024)])
def test_retransmit_at_the_select_block_limit(W, inflight, last_len, nblk):
    """k_tx_select reads one block count per lane of its 1024: windows of 1023 blocks and the
    first one of 1024, with a short last chunk; payload and builder image stay on the device."""
    assert -(-inflight // TX_BLOCK) == nblk
    src = Source(W, inflight, last_len, 7 if nblk == 1023 else 0xFFFFFFF0, host=False)
    _retx_block_limit(W, src)
    del src.buf, src.dev, src.image
    torch.cuda.empty_cache()


def test_retransmit_at_max_inflight(W, src_max):
    """The same at WTP_TX_MAX_INFLIGHT: 1024 full blocks."""
    assert src_max.inflight == TX_BLOCK * TX_BLOCK
    _retx_block_limit(W, src_max)


def test_retransmit_paging_invariance(W, src_max):
    """On the device alone: calling with max_sel = 500 until nothing is emitted gives, in
    order, exactly the datagrams of one call with max_sel = due, and the same timers."""
    inflight, m = src_max.inflight, 500
    mask = _sparse_due(inflight)
    acked, sent = _state(inflight, mask)
    due = int(mask.sum())
    whole = []
    retx(W, src_max, acked, sent, NOW, TIMEOUT, 0, due, vectorised=True, keep=whole)
    pages, state = [], sent
    for _ in range(-(-due // m) + 1):
        _, state, (emitted, left) = retx(W, src_max, acked, state, NOW, TIMEOUT, 0, m, vectorised=True, keep=pages)
        assert left == due - sum(p[0].size for p in pages[:-1]) and emitted == min(left, m)
    assert emitted == 0 and [p[0].size for p in pages] == [500] * (due // m) + [due % m, 0]
    assert np.array_equal(np.concatenate([p[0] for p in pages]), whole[0][0])
    assert np.array_equal(whole[0][0], np.flatnonzero(mask))
    assert torch.equal(torch.cat([p[1] for p in pages]), whole[0][1])
    assert np.array_equal(pages[-1][2], whole[0][2]) and np.array_equal(state, whole[0][2])
