"""GPU tests of the device-side ACK generation, wtp_rx_build_acks: a batch goes through the
real wtp_accept_data_packets, then every output of the ACK call is compared element-wise
with the sequential model (tests/ack_model.py).  Buffers carry sentinels (0xA5 in the ACK
ring, 12345 in d_src, 0x77777777 around d_counts, random bytes in and around d_work), so a
byte that must stay untouched is checkable."""
import numpy as np
import pytest

import accept_model
import ack_model as A
import oracle as O
import retx_model as R
from gpu_support import W  # noqa: F401 (fixture: wtp_init for accept's verify; the ACK call needs none)
from gpu_support import Bytes, DevAckEnd, Words, assert_no_data_error, capture, replay_each_then_together, s32, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, STRIDE, SENT = A.MAXP, R.STRIDE, 12345
MODES = [A.SELECTIVE, A.CUMULATIVE]


class AcceptedBatch:
    """A receive ring on the device after wtp_accept_data_packets on a pre-filled window, with
    the host copies the model needs; accept's outputs are compared with accept_model."""

    def __init__(self, W, ring, rl, stride, seq0, window, sl0, ring_off=0):
        self.ring, self.rl, self.stride, self.seq0, self.window, self.n = ring, rl, stride, seq0, window, rl.size
        n = self.n
        self.dbuf = Bytes(ring, off=ring_off)  # 16 guard bytes (0xC3) after it
        self.d = self.dbuf.t
        self.r, self.sl, self.pl = Words(rl), Words(sl0), Words(SENT, n)
        self.okt = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda")
        self.img = torch.empty(max(window, 1) * MAXP, dtype=torch.uint8, device="cuda")
        ack = Words(0, 1)
        W.accept_data_packets(self.d, stride, self.r.t, n, seq0, window, self.img, self.sl.t, self.okt, self.pl.t, ack.t)
        torch.cuda.synchronize()
        self.ack = int(ack.get()[0])
        self.ok, self.place, self.sl_after = self.okt.cpu().numpy()[:n].copy(), self.pl.get(), self.sl.get()
        ok, place, _, sl, m_ack = accept_model.accept(ring, stride, rl, seq0, window, np.zeros(window * MAXP, np.uint8), sl0)
        assert np.array_equal(self.ok, ok) and np.array_equal(self.place, place)
        assert np.array_equal(self.sl_after, sl) and self.ack == m_ack

    def set_inputs(self, ok, place, sl):
        """Arbitrary verdicts in place of accept's."""
        self.ok, self.place, self.sl_after = ok, place, sl
        self.okt[:self.n].copy_(torch.from_numpy(ok))
        self.pl, self.sl = Words(place), Words(sl)


def acks(W, b, mode, skip=0, max_acks=None, ack_stride=16, ack_off=0, with_src=True, with_place=True, work_off=16,
         vectorised=False):
    """One wtp_rx_build_acks on the device and in the model from the same inputs; asserts
    every output equal and every input and guard untouched; returns the model's (ack
    seqNums, src, (emitted, eligible))."""
    n = b.n
    max_acks = n if max_acks is None else max_acks
    cap = max_acks + 2  # two ring entries more than the call may use
    wbuf = torch.full((cap * ack_stride + ack_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    wire = wbuf[ack_off:ack_off + cap * ack_stride]
    src = Words(SENT, cap)
    cbuf = torch.full((6,), 0x77777777, dtype=torch.int32, device="cuda")
    need = W.rx_ack_work_bytes(n, b.window, mode)
    wkbuf = torch.randint(0, 256, (need + work_off + 16,), dtype=torch.uint8, device="cuda")
    before = wkbuf.clone()
    W.rx_build_acks(b.d, b.stride, b.r.t, n, mode, b.seq0, b.window, b.okt, b.pl.t if with_place else None,
                    b.sl.t if with_place else None, wire, ack_stride, skip, max_acks, src.t if with_src else None,
                    cbuf[2:4], work=wkbuf[work_off:work_off + need])
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == "k_ack_emit"
    seq, idx, (emitted, total) = A.build_acks(b.ring, b.stride, b.rl, mode, b.seq0, b.window, b.place, b.sl_after, ok=b.ok,
                                              skip=skip, max_acks=max_acks, vectorised=vectorised)
    assert u32(cbuf).tolist() == [0x77777777] * 2 + [emitted, total] + [0x77777777] * 2
    rows = wire.view(cap, ack_stride).cpu().numpy()
    assert np.array_equal(rows[:emitted, :16], A.ack_bytes(seq))
    assert (rows[emitted:] == 0xA5).all() and (rows[:, 16:] == 0xA5).all()  # past the count / the datagram
    assert (wbuf[:ack_off] == 0xA5).all() and (wbuf[wbuf.numel() - 16:] == 0xA5).all()
    want_src = np.concatenate([idx, np.full(cap - emitted, SENT, np.uint32)]) if with_src else np.full(cap, SENT, np.uint32)
    assert np.array_equal(src.get(), want_src)
    assert torch.equal(wkbuf[:work_off], before[:work_off]) and torch.equal(wkbuf[work_off + need:], before[work_off + need:])
    # every input is only read
    assert np.array_equal(b.r.get(), b.rl) and np.array_equal(b.pl.get(), b.place) and np.array_equal(b.sl.get(), b.sl_after)
    okh = b.okt.cpu().numpy()
    assert np.array_equal(okh[:n], b.ok) and (okh[n:] == 7).all() and np.array_equal(b.dbuf.get(), b.ring)
    assert_no_data_error(W)
    return seq, idx, (emitted, total)


def _mixed(W, rng, n, seq0, window, stride=STRIDE, ring_off=0):
    sl0 = A.prefilled(rng, window)
    dgrams, _ = A.trace(rng, n, seq0, window, sl0, stride)
    ring, _ = R.make_ring([d[:stride] for d in dgrams], stride)
    rl = np.array([len(d) for d in dgrams], dtype=np.uint32)
    return AcceptedBatch(W, ring[:n * stride], rl, stride, seq0, window, sl0, ring_off=ring_off)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seq0", [0, 0xFFFFFFF0])
@pytest.mark.parametrize("window", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_mixed_batches(W, mode, seq0, window):
    """Every disturbance class of the CPU traces, through the real accept on a window with a
    pre-filled leading run and scattered slots, at batch sizes around the wave and block
    boundaries."""
    rng = np.random.default_rng(window * 11 + mode)
    answered = 0
    for n in (0, 1, 63, 64, 65, 1023, 1025, 3000):
        b = _mixed(W, rng, n, seq0, window)
        seq, idx, (emitted, total) = acks(W, b, mode)
        assert emitted == total
        if mode == A.CUMULATIVE and total and idx[-1] == n - 1:
            assert seq[-1] == b.ack  # the last running ACK is accept's cumulative ACK
        answered += total
    assert answered > 300  # window 0: only datagrams below the window are answered


@pytest.mark.parametrize("mode", MODES)
def test_ring_limits(W, mode):
    """skip and max_acks around the eligible count; two pages concatenate to the whole."""
    rng = np.random.default_rng(77 + mode)
    b = _mixed(W, rng, 1500, 0xFFFFFFF0, 200)
    seq, idx, (e, _) = acks(W, b, mode)
    assert e > 300
    for max_acks in (0, 1, e - 1, e, e + 5):
        for skip in (0, 1, e - 1, e, e + 3):
            s, i, counts = acks(W, b, mode, skip=skip, max_acks=max_acks)
            assert counts == (min(max(e - skip, 0), max_acks), e)
            assert np.array_equal(s, seq[skip:skip + max_acks]) and np.array_equal(i, idx[skip:skip + max_acks])
    first = acks(W, b, mode, skip=0, max_acks=e // 3)
    rest = acks(W, b, mode, skip=e // 3, max_acks=e)
    assert np.array_equal(np.concatenate([first[0], rest[0]]), seq) and np.array_equal(np.concatenate([first[1], rest[1]]), idx)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride,ring_off,ack_stride,ack_off,work_off", [
    (1472, 0, 16, 0, 16), (1504, 0, 64, 0, 16), (1473, 0, 20, 0, 16), (1472, 1, 16, 1, 1), (1504, 0, 16, 8, 3),
    (1473, 1, 64, 8, 16), (1472, 0, 20, 1, 2)])
def test_layouts(W, mode, stride, ring_off, ack_stride, ack_off, work_off):
    """Ring strides and bases, ACK ring strides and bases (the 16-B store and the bytewise
    path give the same bytes), d_work at any alignment, NULL d_src, and NULL d_place /
    d_slot_len in selective mode."""
    rng = np.random.default_rng(stride + ack_stride + ack_off)
    b = _mixed(W, rng, 700, 0xFFFFFFFE, 130, stride=stride, ring_off=ring_off)
    _, _, (e, _) = acks(W, b, mode, ack_stride=ack_stride, ack_off=ack_off, work_off=work_off)
    assert e > 100
    acks(W, b, mode, ack_stride=ack_stride, ack_off=ack_off, work_off=work_off, with_src=False,
         with_place=mode == A.CUMULATIVE)


def _device_batch(W, slots, seq0):
    """len(slots) full DATA datagrams from the device builder, datagram i for window slot
    slots[i]: the builder numbers them in order, then their seqNum fields are rewritten (the
    checksum covers the payload only).  Returns (ring, recv_len) on the device."""
    n = slots.size
    pay = torch.empty(n * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(pay, seed=0xACE + n)
    ring = torch.empty((n, STRIDE), dtype=torch.uint8, device="cuda")
    rl = torch.empty(n, dtype=torch.int32, device="cuda")
    W.build_data_packets(pay, n * MAXP, 0, ring, STRIDE, rl)
    seqs = torch.from_numpy((slots.astype(np.int64) + seq0) & A.M32).cuda()
    for k in range(4):
        ring[:, 4 + k] = ((seqs >> (8 * (3 - k))) & 0xFF).to(torch.uint8)
    return ring, rl


def _big(W, mode, slots, seq0, window, prefill):
    """A device-built batch through accept and the ACK call, against the vectorised model
    fed with accept's own outputs."""
    n = slots.size
    ring, rl = _device_batch(W, slots, seq0)
    sl = torch.full((window + 4,), -1, dtype=torch.int32, device="cuda")
    sl[:prefill] = MAXP
    img = torch.empty(window * MAXP, dtype=torch.uint8, device="cuda")
    okt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    place = torch.zeros(n, dtype=torch.int32, device="cuda")
    ack, counts = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    W.accept_data_packets(ring, STRIDE, rl, n, seq0, window, img, sl, okt, place, ack)
    wire = torch.full((n + 2, 16), 0xA5, dtype=torch.uint8, device="cuda")
    src = torch.full((n + 2,), SENT, dtype=torch.int32, device="cuda")
    W.rx_build_acks(ring, STRIDE, rl, n, mode, seq0, window, okt, place, sl, wire, 16, 0, n, src, counts)
    torch.cuda.synchronize()
    assert bool(okt.all()) and bool((sl[window:] == -1).all())
    hdr = np.ascontiguousarray(ring[:, :8].cpu().numpy()).reshape(-1)
    seq, idx, (emitted, total) = A.build_acks(hdr, 8, u32(rl), mode, seq0, window, u32(place), u32(sl)[:window],
                                              ok=okt.cpu().numpy(), vectorised=True)
    assert emitted == total == n and tuple(u32(counts)) == (n, n)
    rows = wire.cpu().numpy()
    assert np.array_equal(rows[:n], A.ack_bytes(seq)) and (rows[n:] == 0xA5).all()
    assert np.array_equal(u32(src), np.concatenate([idx, [SENT, SENT]]))
    assert int(seq[-1]) == int(u32(ack)[0]) if mode == A.CUMULATIVE else True
    assert_no_data_error(W)
    return seq


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ["random", "local"])
def test_scan_across_blocks(W, mode, order):
    """Window 70 000 (69 scan blocks) with its datagrams in a seeded random order, 5 % of
    them dropped (all from the upper half, so the leading run crosses 34 blocks): a random
    permutation of the whole window, where the prefix maximum saturates early and the run
    moves in a few large steps, and one shuffled within runs of 97 slots, where the running
    ACK climbs steadily through the batch."""
    rng = np.random.default_rng(70000)
    window, seq0 = 70000, 0xFFFF0000
    if order == "random":
        slots = rng.permutation(window)
    else:
        slots = np.concatenate([c[rng.permutation(c.size)] for c in np.array_split(np.arange(window), window // 97)])
    slots = slots[(slots < window // 2) | (rng.random(window) >= 0.1)]
    seq = _big(W, mode, slots, seq0, window, 0)
    if mode == A.CUMULATIVE:
        run = (seq.astype(np.int64) - seq0) & A.M32
        assert (np.diff(run) >= 0).all() and window // 2 <= run[-1] < window
        assert np.unique(run).size > (300 if order == "local" else 1)


@pytest.mark.parametrize("mode", MODES)
def test_largest_window(W, mode):
    """window = WTP_RX_MAX_WINDOW (1024 scan blocks), the first 300 000 slots filled before,
    5 000 datagrams: every other one continues the leading run (runs of 50 slots, each in
    falling order, so the run grows by 50 at a time), the others are scattered above."""
    rng = np.random.default_rng(1 << 20)
    window, pre = W.RX_MAX_WINDOW, 300000
    slots = np.empty(5000, dtype=np.int64)
    slots[0::2] = pre + np.arange(2500).reshape(50, 50)[:, ::-1].ravel()
    slots[1::2] = rng.choice(np.arange(pre + 2500, window), 2500, replace=False)
    seq = _big(W, mode, slots, 0xFFF00000, window, pre)
    if mode == A.CUMULATIVE:
        run = (seq.astype(np.int64) - 0xFFF00000) & A.M32
        assert run[0] == pre and run[-1] >= pre + 2500 and np.unique(run).size >= 50


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("window,n", [(5, 40), (100, 700), (2049, 3000)])
def test_arbitrary_place(W, mode, window, n):
    """d_ok, d_place and d_slot_len are any input: entries >= window, slots named many times
    (the lowest index fills the slot), named slots that d_slot_len calls empty."""
    rng = np.random.default_rng(window + mode)
    b = _mixed(W, rng, n, 3, window)
    place = rng.integers(0, window + 5, n).astype(np.uint32)
    place[rng.random(n) < 0.3] = A.NOT_PLACED
    place[rng.random(n) < 0.1] = window // 2  # many writers for one slot
    b.set_inputs((rng.random(n) < 0.8).astype(np.uint8) & b.ok, place, A.prefilled(rng, window))
    _, _, (e, _) = acks(W, b, mode)
    assert e > n // 8


@pytest.mark.parametrize("mode", MODES)
def test_more_than_one_block_count_per_lane(W, mode):
    """2^20 + 1025 header-only DATA datagrams (stride 16, length 0, checksum 0) are 1026
    blocks of k_ack_mark, so a lane of k_ack_emit sums two block counts: the smallest batch
    that does.  d_ok (about half ones), d_place and d_slot_len are supplied directly: 2049
    datagrams spread over the batch name the window's slots in rising order, shuffled within
    runs of 16, so the running ACK climbs through the whole batch."""
    n, window, seq0 = (1 << 20) + 1025, 2049, 0xFFFFFF00
    rng = np.random.default_rng(n + mode)
    hdr = np.zeros((n, 4), dtype=">u4")
    hdr[:, 0] = 2
    hdr[:, 1] = (seq0 + rng.integers(-50, window + 50, n)) & A.M32  # some below and some past the window
    ring, rl = hdr.view(np.uint8).reshape(-1), np.full(n, 16, np.uint32)
    ok = (rng.random(n) < 0.5).astype(np.uint8)
    place = np.where(rng.random(n) < 0.001, window + 3, A.NOT_PLACED).astype(np.uint32)  # >= window: not placed
    place[np.sort(rng.choice(n, window, replace=False))] = np.concatenate(
        [c[rng.permutation(c.size)] for c in np.array_split(np.arange(window), window // 16)])
    sl = A.prefilled(rng, window)
    seq, idx, (emitted, total) = A.build_acks(ring, 16, rl, mode, seq0, window, place, sl, ok=ok, vectorised=True)
    assert n // 3 < emitted == total < n // 2
    if mode == A.CUMULATIVE:  # the running ACK still moves past datagram 2^20
        assert np.unique(seq).size > 100 and idx[np.flatnonzero(np.diff(seq.astype(np.int64)))[-1] + 1] > 1 << 20

    d, r, okt = torch.from_numpy(ring).cuda(), Words(rl), torch.from_numpy(ok).cuda()
    pl, slw, src, counts = Words(place), Words(sl), Words(SENT, n + 2), Words(0x77777777, 2)
    wire = torch.full((n + 2, 16), 0xA5, dtype=torch.uint8, device="cuda")
    W.rx_build_acks(d, 16, r.t, n, mode, seq0, window, okt, pl.t, slw.t, wire, 16, 0, n, src.t, counts.t)
    torch.cuda.synchronize()
    assert tuple(counts.get()) == (emitted, total)
    assert np.array_equal(src.get(), np.concatenate([idx, np.full(n + 2 - emitted, SENT, np.uint32)]))
    rows = wire.cpu().numpy()
    assert np.array_equal(rows[:emitted], A.ack_bytes(seq)) and (rows[emitted:] == 0xA5).all()
    assert np.array_equal(pl.get(), place) and np.array_equal(slw.get(), sl) and np.array_equal(r.get(), rl)
    assert_no_data_error(W)


def test_graph_replay(W):
    """accept + build_acks captured into one graph and replayed three times into cleared
    outputs and a scribbled work buffer; then two graphs on two streams with their own work
    buffers, replayed at once.  The ACK call itself needs no wtp_init: it reads no table."""
    window, n, seq0 = 300, 900, 0xFFFFFF00

    class G:
        def __init__(self, salt, mode):
            rng = np.random.default_rng(salt)
            self.mode, self.sl0 = mode, A.prefilled(rng, window)
            dgrams, _ = A.trace(rng, n, seq0, window, self.sl0, STRIDE)
            self.ring, _ = R.make_ring([d[:STRIDE] for d in dgrams], STRIDE)
            self.rl = np.array([len(d) for d in dgrams], dtype=np.uint32)
            z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
            self.d, self.r = torch.from_numpy(self.ring).cuda(), torch.from_numpy(s32(self.rl)).cuda()
            self.sl, self.img, self.ok, self.place, self.ack = z(window), z(window * MAXP, torch.uint8), z(n, torch.uint8), z(n), z(1)
            self.wire, self.src, self.counts = z(n * 16, torch.uint8), z(n), z(2)
            self.work = z(W.rx_ack_work_bytes(n, window, mode), torch.uint8)
            self.reset()
            self.graph, self.stream = capture(self.call)
            ok, place, _, sl, _ = accept_model.accept(self.ring, STRIDE, self.rl, seq0, window, np.zeros(window * MAXP, np.uint8),
                                                      self.sl0)
            self.want = A.build_acks(self.ring, STRIDE, self.rl, mode, seq0, window, place, sl, ok=ok)

        def call(self):
            W.accept_data_packets(self.d, STRIDE, self.r, n, seq0, window, self.img, self.sl, self.ok, self.place, self.ack)
            W.rx_build_acks(self.d, STRIDE, self.r, n, self.mode, seq0, window, self.ok, self.place, self.sl, self.wire, 16, 0,
                            n, self.src, self.counts, work=self.work)

        def reset(self):
            self.sl.copy_(torch.from_numpy(s32(self.sl0)))
            self.wire.fill_(0xA5)
            self.src.fill_(SENT)
            self.counts.fill_(0x77777777)
            self.work.random_(0, 256)

        def check(self):
            seq, idx, (emitted, total) = self.want
            assert tuple(u32(self.counts)) == (emitted, total) and emitted > 100
            rows = self.wire.view(n, 16).cpu().numpy()
            assert np.array_equal(rows[:emitted], A.ack_bytes(seq)) and (rows[emitted:] == 0xA5).all()
            assert np.array_equal(u32(self.src), np.concatenate([idx, np.full(n - emitted, SENT, np.uint32)]))

    replay_each_then_together(G(1, A.CUMULATIVE), [()] * 3, lambda: (G(2, A.SELECTIVE), G(3, A.CUMULATIVE)), [()] * 3)
    assert_no_data_error(W)


# ---- end to end on the device -------------------------------------------------------------------
@pytest.mark.parametrize("mode,seq_base", [(A.SELECTIVE, 0), (A.SELECTIVE, 0xFFFFFF80), (A.CUMULATIVE, 0),
                                           (A.CUMULATIVE, 0xFFFFFF80)])
def test_end_to_end_transfer_with_device_acks(W, mode, seq_base):
    """build -> lossy channel -> accept -> build_acks -> lossy ACK channel (index_select) ->
    ingest -> retransmit -> shift, against the model driving the same loop with the same
    seeds: the same number of rounds (whatever the model needs; the loop fails at 40), the
    same retransmit set every round, an exact image and whole-file CRC at the receiver."""
    nchunks, window = R.E2E_CHUNKS, R.E2E_WINDOW
    total = nchunks * MAXP - R.E2E_SHORT
    host = O.synth_fill_np(total, seed=R.E2E_SEED)
    want_rounds, want_sets = A.transfer(A.ModelEnd(host, nchunks, window, seq_base), nchunks, window, seq_base, mode,
                                        R.E2E_SEED, R.E2E_LOSS)
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=R.E2E_SEED)
    end = DevAckEnd(W, src, total, nchunks, window, seq_base)
    rounds, sets = A.transfer(end, nchunks, window, seq_base, mode, R.E2E_SEED, R.E2E_LOSS)
    assert rounds == want_rounds and sets == want_sets
    assert torch.equal(end.img[:total], src) and bool((end.img[total:nchunks * MAXP] == 0xA5).all())
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(end.img, total, crc)
    assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)
