"""GPU tests of the one structure all eight protocol calls share, the 16-byte header
htonl{type, seqNum, length, checksum}: the five writers against the bytes the reference's own
Packet code produced (tests/golden/wire.json; the reference itself is never read here), and
the three readers at the header's edges: type words that are right in one byte only, sequence
distances around 2^31, every bit of the checksum field, and a length field that disagrees
with the datagram.  Every comparison is bit-exact.  Beside the models' outputs stand literal
expectations that pass through no model, so a misreading that a model and a kernel share
still fails.  Buffers carry guards and sentinels as in the sibling files."""
import numpy as np
import pytest

import ack_model as A
import buildvar_model
import oracle as O
import retx_model as R
import wire_golden as G
from gpu_support import W, W_noinit  # noqa: F401 (fixtures: W for the calls that verify or use the braided builder)
from gpu_support import Batch, Bytes, DevWindow, Words, assert_no_data_error, datagram_ring

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, M32, NOT_PLACED, EMPTY, SENT = A.MAXP, A.M32, A.NOT_PLACED, A.EMPTY, 12345
MODES = [A.SELECTIVE, A.CUMULATIVE]
SEQS, LENS = G.load()["seqs"], G.load()["lens"]
TYPES = G.load()["types"]
# the vector path (a 16-B aligned ring whose stride is a multiple of 16) and the bytewise path
WIRE_LAYOUTS = [(1472, 0), (1473, 1)]
# load_header's dword branch (every slot 4-B aligned), the issue's odd layout (three slots in
# four take the byte branch) and a layout in which every slot takes the byte branch
HEADER_LAYOUTS = [(1472, 0), (1473, 1), (1472, 1)]


# ---- helpers --------------------------------------------------------------------------------
def _source(seq, ln):
    """(payload, the 16 header bytes a DATA datagram (seq, payload) must carry, the corpus key
    or None): the reference's recorded header where the corpus has the pair, else the oracle's."""
    key = (2, seq, ln)
    if key in G.corpus():
        sb, hdr = G.corpus()[key]
        return G.payload(sb, ln), hdr, key
    pay = O.synth_fill_np(ln, start_byte=977 * (seq & 0xFFFF) + ln).tobytes()
    return pay, O.build_datagram(seq, pay)[:16], None


def _u8(data):
    return np.frombuffer(data, dtype=np.uint8).copy()


def _wire(n, stride, off):
    """n slots of 0xA5 at byte `off` past a 16-B aligned address, between guards."""
    return Bytes(fill=0xA5, size=n * stride, off=off, front=16)


def _check_wire(wire, stride, parts, seen, tails=True):
    got = wire.get().reshape(len(parts), stride)  # get(): the guards around the ring are intact
    for i, (pay, hdr, key) in enumerate(parts):
        assert got[i, :16].tobytes() == hdr, (i, got[i, :16].tobytes().hex(), hdr.hex())
        assert got[i, 16:16 + len(pay)].tobytes() == pay, i
        if tails:
            assert (got[i, 16 + len(pay):] == 0xA5).all(), i
        if key:
            seen.add(key)


def _checksums(parts):
    return [int.from_bytes(hdr[12:], "big") for _, hdr, _ in parts]


def _acks(W, win, stride, mode, seq0):
    """wtp_rx_build_acks for the batch `win` (a DevWindow) has just accepted, from accept's own
    device outputs; every output is compared with ack_model.  Returns the device's (ACK
    seqNums, datagram indices, eligible count)."""
    n = win.n
    wire, src, counts = Bytes(fill=0xA5, size=(n + 2) * 16, front=16), Words(SENT, n + 2), Words(0x77777777, 2)
    W.rx_build_acks(win.ring.t, stride, win.rl.t, n, mode, seq0, win.window, win.ok.t, win.place.t, win.slot_len, wire.t, 16,
                    0, n, src.t, counts.t)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == "k_ack_emit"
    seq, idx, (emitted, total) = A.build_acks(win.ring.host, stride, win.rl_host, mode, seq0, win.window, win.place.get(),
                                              win.sl.get(), ok=win.ok.get())
    assert tuple(counts.get()) == (emitted, total) and emitted == total
    rows, got_src = wire.get().reshape(n + 2, 16), src.get()
    assert np.array_equal(rows[:emitted], A.ack_bytes(seq)) and (rows[emitted:] == 0xA5).all()
    assert np.array_equal(got_src[:emitted], idx) and (got_src[emitted:] == SENT).all()
    assert np.array_equal(win.ring.get(), win.ring.host)  # the ring is only read
    assert_no_data_error(W)
    got_seq = np.ascontiguousarray(rows[:emitted, 4:8]).view(">u4").reshape(-1).astype(np.uint32)
    return got_seq, got_src[:emitted], int(counts.get()[1])


def _ingest(W, dgrams, stride, off, mode, seq0, inflight):
    """wtp_tx_ingest_acks on an un-ACKed window of `inflight` slots; every output is compared
    with retx_model.ingest.  Returns the device's (ok, hit, acked, counts)."""
    ring, rl = datagram_ring(dgrams, stride)
    n = rl.size
    dbuf, r, ok, hit = Bytes(ring, off=off, front=16), Words(rl), Bytes(fill=7, size=n, front=16), Words(SENT, n)
    st, counts = Words(0, inflight), Words(0x77777777, 2)
    W.tx_ingest_acks(dbuf.t, stride, r.t, n, mode, seq0, inflight, st.t, ok.t, hit.t, counts.t)
    torch.cuda.synchronize()
    got = ok.get().copy(), hit.get(), st.get(), tuple(int(c) for c in counts.get())
    want = R.ingest(ring, stride, rl, mode, seq0, inflight, np.zeros(inflight, np.uint32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert np.array_equal(dbuf.get(), ring) and np.array_equal(r.get(), rl)  # the inputs are only read
    assert_no_data_error(W)
    return got


def _verify(W, win, stride):
    """wtp_crc32_verify_batch alone on the ring `win` holds: (ok, the kernel it launched)."""
    ok = Bytes(fill=7, size=win.n, front=16)
    W.verify_batch(win.ring.t, stride, win.rl.t, win.n, ok.t)
    torch.cuda.synchronize()
    return ok.get().copy(), W.LIB.wtp_last_kernel().decode()


# ---- a. the writers against the recorded reference bytes ------------------------------------
@pytest.mark.parametrize("stride,off", WIRE_LAYOUTS)
def test_fixed_writers_against_the_reference(W, stride, off):
    """wtp_build_data_packets and wtp_tx_build_retransmit: a call expresses one full chunk and
    one tail, so one call per (seqNum, tail length) of the corpus with seq0 = seqNum - 1, which
    also puts the wrap values 0xFFFFFFFF -> 0 and 0x7FFFFFFF -> 0x80000000 on one call's two
    datagrams.  (Neither call can express an empty payload.)"""
    seen = set()
    for tail in LENS[1:]:
        for s in SEQS:
            seq0 = (s - 1) & M32
            parts = [_source(seq0, MAXP), _source(s, tail)]
            src = Bytes(_u8(parts[0][0] + parts[1][0]))
            wire, wlen = _wire(2, stride, off), Words(SENT, 2)
            W.build_data_packets(src.t, MAXP + tail, seq0, wire.t, stride, wlen.t)
            torch.cuda.synchronize()
            _check_wire(wire, stride, parts, seen, tails=False)  # the builder leaves a slot's tail unspecified
            assert wlen.get().tolist() == [16 + MAXP, 16 + tail]

            wire, wlen, sel, counts = _wire(2, stride, off), Words(SENT, 2), Words(SENT, 2), Words(0x77777777, 2)
            acked, sent = Words(0, 2), Words(0, 2)
            W.tx_build_retransmit(src.t, MAXP + tail, seq0, 2, acked.t, sent.t, 1000, 500, R.RETX_ALL, wire.t, stride, 2,
                                  sel.t, wlen.t, counts.t)
            torch.cuda.synchronize()
            _check_wire(wire, stride, parts, seen)
            assert wlen.get().tolist() == [16 + MAXP, 16 + tail] and sel.get().tolist() == [0, 1]
            assert tuple(counts.get()) == (2, 2) and sent.get().tolist() == [1000, 1000] and acked.get().tolist() == [0, 0]
            assert np.array_equal(src.get(), src.host)
    assert seen == {(2, s, ln) for s in SEQS for ln in LENS[1:]}  # every pair met the reference's bytes
    assert_no_data_error(W)


@pytest.mark.parametrize("stride,off", WIRE_LAYOUTS)
def test_var_writers_against_the_reference(W_noinit, stride, off):
    """wtp_build_data_packets_var and wtp_tx_build_retransmit_var: the seven lengths in one
    batch, and for every (seqNum, length) of the corpus one batch whose seq0 puts that seqNum on
    that length; the other six records meet the corpus where it has their pair, else the oracle."""
    W, seen, n = W_noinit, set(), len(LENS)
    for s in SEQS:
        for li in range(n):
            seq0 = (s - li) & M32
            parts = [_source((seq0 + j) & M32, LENS[j]) for j in range(n)]
            b = Batch(_u8(b"".join(p[0] for p in parts)), buildvar_model.packed_offsets(LENS), LENS)
            want_len, want_crc = [16 + ln for ln in LENS], _checksums(parts)

            wire, wlen, crc = _wire(n, stride, off), Words(SENT, n), Words(SENT, n)
            W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, wire.t, stride, wlen.t, crc.t)
            torch.cuda.synchronize()
            assert W.LIB.wtp_last_kernel().decode() == "k_build_var"
            _check_wire(wire, stride, parts, seen)
            assert wlen.get().tolist() == want_len and crc.get().tolist() == want_crc

            wire, wlen, crc = _wire(n, stride, off), Words(SENT, n), Words(SENT, n)
            sel, counts, acked, sent = Words(SENT, n), Words(0x77777777, 2), Words(0, n), Words(0, n)
            W.tx_build_retransmit_var(b.base, b.base_bytes, b.o, b.l.t, seq0, n, acked.t, sent.t, 1000, 500, R.RETX_ALL,
                                      wire.t, stride, n, sel.t, wlen.t, crc.t, counts.t)
            torch.cuda.synchronize()
            assert W.LIB.wtp_last_kernel().decode() == "k_tx_emit_var"
            _check_wire(wire, stride, parts, seen)
            assert wlen.get().tolist() == want_len and crc.get().tolist() == want_crc
            assert sel.get().tolist() == list(range(n)) and tuple(counts.get()) == (n, n)
            b.check_untouched()
    assert seen == {(2, s, ln) for s in SEQS for ln in LENS}
    assert_no_data_error(W)


@pytest.mark.parametrize("ack_stride,ack_off", [(16, 0), (17, 1)])
def test_ack_writer_against_the_reference(W_noinit, ack_stride, ack_off):
    """wtp_rx_build_acks in selective mode answers the reference's five header-only DATA
    datagrams (seq0 = 0x7FFFFFFF, window 2: two inside, three below) with the reference's five
    empty ACKs: the 16-B store and the bytewise path."""
    W = W_noinit
    order = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0, 1]
    assert sorted(order) == sorted(SEQS)
    ring, rl = datagram_ring([G.datagram(2, s, 0) for s in order], 16)
    d, r, ok = Bytes(ring), Words(rl), Bytes(np.ones(5, np.uint8))
    wire, src, counts = Bytes(fill=0xA5, size=7 * ack_stride, off=ack_off, front=16), Words(SENT, 7), Words(0x77777777, 2)
    W.rx_build_acks(d.t, 16, r.t, 5, A.SELECTIVE, 0x7FFFFFFF, 2, ok.t, None, None, wire.t, ack_stride, 0, 5, src.t, counts.t)
    torch.cuda.synchronize()
    rows = wire.get().reshape(7, ack_stride)
    for k, s in enumerate(order):
        assert rows[k, :16].tobytes() == G.datagram(3, s, 0), (k, rows[k, :16].tobytes().hex())
    assert (rows[5:] == 0xA5).all() and (rows[:, 16:] == 0xA5).all()
    assert tuple(counts.get()) == (5, 5) and src.get().tolist() == [0, 1, 2, 3, 4, SENT, SENT]
    assert np.array_equal(d.get(), ring) and ok.get().all()
    assert_no_data_error(W)


# ---- b. adversarial type words --------------------------------------------------------------
def _type_corpus():
    """[(type word, payload length)]: every word of the corpus at 0, 17 and 1456 bytes, a DATA
    and an ACK control after each word's three."""
    out = []
    for t in TYPES:
        out += [(t, 0), (t, 17), (t, MAXP), (2, 17), (3, 17)]
    return out


@pytest.mark.parametrize("stride,off", HEADER_LAYOUTS)
def test_type_words_through_the_receive_calls(W, stride, off):
    """Every type word heads an otherwise perfect datagram (valid checksum, a seqNum of its own
    inside the window, an empty slot): verify accepts all, accept places and build_acks answers
    exactly the words equal to 2."""
    cases, seq0 = _type_corpus(), 0xFFFFFFE0
    n = len(cases)
    dg = [O.build_datagram((seq0 + i) & M32, O.synth_fill_np(ln, start_byte=131 * i).tobytes(), ptype=t)
          for i, (t, ln) in enumerate(cases)]
    words, lens = np.array([t for t, _ in cases], dtype=np.uint32), np.array([ln for _, ln in cases], dtype=np.uint32)
    data = np.flatnonzero(words == 2)
    assert data.size == 3 + len(TYPES) and (words & 0xFF == 2).sum() > data.size  # the control and the near misses
    ring, rl = datagram_ring(dg, stride)
    win = DevWindow(n)
    ok, place, ack = win.accept(W, ring, stride, rl, seq0, ring_off=off)  # compared with accept_model inside
    assert ok.all() and _verify(W, win, stride)[0].all()
    assert np.array_equal(place, np.where(words == 2, np.arange(n), NOT_PLACED).astype(np.uint32))
    assert np.array_equal(win.h_slot_len, np.where(words == 2, lens, EMPTY).astype(np.uint32))
    assert ack == seq0  # datagram 0 is of type 0: slot 0 stays empty
    for mode in MODES:
        seq, src, eligible = _acks(W, win, stride, mode, seq0)
        assert np.array_equal(src, data) and eligible == data.size
        assert np.array_equal(seq, (seq0 + data) & M32 if mode == A.SELECTIVE else np.full(data.size, seq0, np.uint32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride,off", HEADER_LAYOUTS)
def test_type_words_through_ingest(W, stride, off, mode):
    """The same words as 16-byte datagrams with checksum 0, one per slot of an un-ACKed sender
    window: all are ok, exactly the words equal to 3 hit, and d_acked changes for nothing else."""
    words = np.array([t for t, _ in _type_corpus()], dtype=np.uint32)
    n, seq0 = words.size, 0xFFFFFFE0
    dg = [R.ack_datagram((seq0 + i) & M32, ptype=int(t)) for i, t in enumerate(words)]
    ok, hit, acked, counts = _ingest(W, dg, stride, off, mode, seq0, n)
    acks = np.flatnonzero(words == 3)
    assert acks.size == 3 + len(TYPES) and (words & 0xFF == 3).sum() > acks.size and acks[0] > 0
    assert ok.all()
    assert np.array_equal(hit, np.where(words == 3, np.arange(n), NOT_PLACED).astype(np.uint32))
    if mode == A.SELECTIVE:
        assert np.array_equal(acked, (words == 3).astype(np.uint32)) and counts == (0, acks.size)
    else:  # the largest cumulative ACK covers every slot below it
        assert np.array_equal(acked, (np.arange(n) < acks[-1]).astype(np.uint32)) and counts == (acks[-1], acks[-1])


# ---- c. sequence-distance edges -------------------------------------------------------------
def _distances(window):
    return list(dict.fromkeys([0, window - 1, window, window + 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF]))


@pytest.mark.parametrize("seq0", [0, 0x80000000, 0xFFFFFFC0])
@pytest.mark.parametrize("window", [1, 64])
def test_sequence_distance_edges_on_receive(W, window, seq0):
    """Intact DATA at seq0 + d for d around the window's end and around 2^31: accept places iff
    d < window; build_acks answers iff d < window or d >= 0x80000000, in both modes."""
    ds = np.array(_distances(window), dtype=np.int64)
    seqs = (seq0 + ds) & M32
    dg = [O.build_datagram(int(s), O.synth_fill_np(17 + k, start_byte=53 * k).tobytes()) for k, s in enumerate(seqs)]
    ring, rl = datagram_ring(dg, 1472)
    win = DevWindow(window)
    ok, place, ack = win.accept(W, ring, 1472, rl, seq0)
    assert ok.all()
    assert np.array_equal(place, np.where(ds < window, ds, NOT_PLACED).astype(np.uint32))
    assert ack == (seq0 + 1) & M32  # d = 0 arrived; window 64 has no d = 1, window 1 ends there
    answered = np.flatnonzero((ds < window) | (ds >= 0x80000000))
    assert answered.size == len(ds) - 4  # all but d = window, window + 1, 0x7FFFFFFE, 0x7FFFFFFF
    for mode in MODES:
        seq, src, eligible = _acks(W, win, 1472, mode, seq0)  # cumulative: the running value, compared with the model
        assert np.array_equal(src, answered) and eligible == answered.size
        if mode == A.SELECTIVE:
            assert np.array_equal(seq, seqs[answered].astype(np.uint32))
        else:
            assert (seq == ((seq0 + 1) & M32)).all()  # slot 0 is filled by datagram 0; slot 1 never is


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seq0", [0, 0x80000000, 0xFFFFFFC0])
@pytest.mark.parametrize("inflight", [1, 64])
def test_sequence_distance_edges_on_ingest(W, inflight, seq0, mode):
    """The same distances as ACKs: selective hits iff d < inflight, cumulative iff 0 < d <= inflight."""
    ds = np.array(_distances(inflight), dtype=np.int64)
    dg = [R.ack_datagram(int((seq0 + d) & M32)) for d in ds]
    ok, hit, acked, counts = _ingest(W, dg, 16, 0, mode, seq0, inflight)
    assert ok.all()
    hits = ds < inflight if mode == A.SELECTIVE else (ds > 0) & (ds <= inflight)
    assert np.array_equal(hit, np.where(hits, ds, NOT_PLACED).astype(np.uint32))
    if mode == A.SELECTIVE:
        want = np.zeros(inflight, np.uint32)
        want[ds[hits]] = 1
        assert np.array_equal(acked, want) and counts == (1, int(hits.sum()))
    else:  # d = inflight is among them: the whole window
        assert acked.all() and counts == (inflight, inflight)


# ---- d. the checksum and length fields ------------------------------------------------------
@pytest.mark.parametrize("plen,stride,off,kernel,epilogue", [(MAXP, 1472, 0, "k_fixed_braid", "VerifyBEpi"),  # the braided rounds
                                                             (40, 1472, 0, "k_fixed_braid", "VerifyBEpi"),    # their fix-up phase
                                                             (40, 1473, 1, "k_pieces", "VerifyEpi")])         # the general kernel
def test_every_bit_of_the_checksum_field(W, plen, stride, off, kernel, epilogue):
    """One datagram per single-bit flip of the checksum field, and an unflipped control before
    and after them: each flip is not ok, not placed and not answered."""
    seq0, dg = 5, []
    for i in range(34):
        d = bytearray(O.build_datagram(seq0 + i, O.synth_fill_np(plen, start_byte=4096 * i).tobytes()))
        if 1 <= i <= 32:
            d[12:16] = (int.from_bytes(d[12:16], "big") ^ (1 << (i - 1))).to_bytes(4, "big")
        dg.append(bytes(d))
    ring, rl = datagram_ring(dg, stride)
    win = DevWindow(34)
    ok, place, ack = win.accept(W, ring, stride, rl, seq0, ring_off=off)
    vok, name = _verify(W, win, stride)
    assert name.split("<")[0] == kernel and name.endswith(epilogue + ">")
    want = [1] + [0] * 32 + [1]
    assert ok.tolist() == want and vok.tolist() == want
    assert place.tolist() == [0] + [NOT_PLACED] * 32 + [33] and ack == seq0 + 1
    assert win.h_slot_len.tolist() == [plen] + [EMPTY] * 32 + [plen]
    for mode in MODES:
        _, src, eligible = _acks(W, win, stride, mode, seq0)
        assert src.tolist() == [0, 33] and eligible == 2


@pytest.mark.parametrize("stride,off", WIRE_LAYOUTS)
def test_length_field_is_ignored_on_receive(W, stride, off):
    """The length field set to 0, len + 1, 1457 and 0xFFFFFFFF under the true checksum and
    recv_len: verdict, placement, the stored slot length (recv_len - 16) and the ACK are those
    of the control with the true field."""
    seq0, dg, lens = 0xFFFFFFF8, [], []
    for ln in (0, 17, MAXP):
        for field in (ln, 0, ln + 1, 1457, 0xFFFFFFFF):
            d = O.build_datagram((seq0 + len(dg)) & M32, O.synth_fill_np(ln, start_byte=211 * len(dg)).tobytes())
            assert int.from_bytes(d[8:12], "big") == ln
            dg.append(d[:8] + field.to_bytes(4, "big") + d[12:])
            lens.append(ln)
    n = len(dg)
    ring, rl = datagram_ring(dg, stride)
    assert rl.tolist() == [16 + ln for ln in lens]
    win = DevWindow(n)
    ok, place, ack = win.accept(W, ring, stride, rl, seq0, ring_off=off)
    assert ok.all() and _verify(W, win, stride)[0].all()
    assert place.tolist() == list(range(n)) and ack == (seq0 + n) & M32
    assert win.h_slot_len.tolist() == lens
    img = win.h_out.reshape(n, MAXP)
    for i, ln in enumerate(lens):
        assert img[i, :ln].tobytes() == dg[i][16:] and (img[i, ln:] == 0xA5).all()
    for mode in MODES:
        seq, src, eligible = _acks(W, win, stride, mode, seq0)
        assert src.tolist() == list(range(n)) and eligible == n
        if mode == A.SELECTIVE:
            assert np.array_equal(seq, (seq0 + np.arange(n)) & M32)
