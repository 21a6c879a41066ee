"""GPU tests of the device-side receive, wtp_accept_data_packets: every output (ok, place,
slot_len, out, ack) is compared element-wise with the sequential model
(tests/accept_model.py, ok pinned to the reference through oracle.verify_datagrams).
`out` is pre-filled with 0xA5, so a byte that must stay untouched is checkable."""
import numpy as np
import pytest

import accept_model as M
import oracle as O
from gpu_support import W  # noqa: F401 (fixture)
from gpu_support import assert_no_data_error, capture, datagram_ring, dev_s32, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _slots(dgrams, stride):
    """(ring, stride, recv_len) of `dgrams` (bytes, none longer than a slot) in `stride`-byte
    slots: accept()'s arguments."""
    ring, rl = datagram_ring(dgrams, stride)
    return ring, stride, rl


class Window:
    """The caller-owned window state on the device (0xA5 image, EMPTY slots), at byte
    offset `out_off` of its allocation."""

    def __init__(self, window, out_off=0):
        self.window = window
        self.buf = torch.full((window * M.MAXP + out_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        self.out = self.buf[out_off:out_off + max(window * M.MAXP, 1)]
        self.slot_len = torch.full((max(window, 1),), -1, dtype=torch.int32, device="cuda")
        self.h_out = np.full(window * M.MAXP, 0xA5, dtype=np.uint8)
        self.h_slot_len = np.full(window, M.EMPTY, dtype=np.uint32)


def accept(W, ring, stride, rl, seq0, win, ring_off=0, with_place=True):
    """One call on the device and in the model from the same entry state; asserts every
    output equal, carries the state over in `win`, returns the model's (ok, place, ack)."""
    n = rl.size
    dbuf = torch.zeros(ring.size + ring_off + 16, dtype=torch.uint8, device="cuda")
    d = dbuf[ring_off:ring_off + max(ring.size, 1)]
    d[:ring.size].copy_(torch.from_numpy(ring))
    r = dev_s32(rl) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = torch.full((max(n, 1),), 7, dtype=torch.uint8, device="cuda")
    place = torch.full((max(n, 1),), 12345, dtype=torch.int32, device="cuda")
    ack = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    W.accept_data_packets(d, stride, r, n, seq0, win.window, win.out, win.slot_len, ok,
                          place if with_place else None, ack)
    torch.cuda.synchronize()
    want_ok, want_place, want_out, want_sl, want_ack = M.accept(ring, stride, rl, seq0, win.window, win.h_out,
                                                                win.h_slot_len)
    assert np.array_equal(ok[:n].cpu().numpy(), want_ok)
    if with_place:
        assert np.array_equal(u32(place[:n]), want_place)
    assert np.array_equal(u32(win.slot_len[:win.window]), want_sl)
    got_out = win.out[:win.window * M.MAXP].cpu().numpy()
    assert np.array_equal(got_out, want_out)
    assert int(u32(ack[:1])[0]) == want_ack
    assert (win.buf[win.buf.numel() - 16:] == 0xA5).all()  # nothing written past the image
    assert W.LIB.wtp_last_kernel().decode() == "k_accept_place"
    assert_no_data_error(W)
    win.h_out, win.h_slot_len = want_out, want_sl
    return want_ok, want_place, want_ack


def _payload(i, ln):
    return O.synth_fill_np(ln, start_byte=4096 * i).tobytes()


@pytest.mark.parametrize("seq0", [0, 0xFFFFFFF0])
def test_round_trip_build_permute_accept(W, seq0):
    """wtp_build_data_packets -> permuted wire slots -> accept reproduces the file on the
    device, also across the 2^32 sequence wrap."""
    total, stride, n = 64 * 1456 - 100, 1472, 64
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=0xACCE)
    wire = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    wlen = torch.zeros(n, dtype=torch.int32, device="cuda")
    W.build_data_packets(src, total, seq0, wire, stride, wlen)
    perm = np.random.default_rng(5).permutation(n)
    ring = wire.view(n, stride)[torch.from_numpy(perm).cuda()].contiguous().view(-1)
    rl = wlen[torch.from_numpy(perm).cuda()]
    torch.cuda.synchronize()
    win = Window(n)
    ok, place, ack = accept(W, ring.cpu().numpy(), stride, rl.cpu().numpy().view(np.uint32), seq0, win)
    assert ok.all() and np.array_equal(place, perm.astype(np.uint32))
    assert ack == (seq0 + 64) & M.M32
    assert torch.equal(win.out[:total], src)
    assert win.h_slot_len.tolist() == [1456] * 63 + [1356]


def test_every_length(W):
    """Payload lengths 0 .. 1484, one datagram each, seq = length, in 1504-B slots: up to
    1456 placed (byte-exact vector tails; bytes [len, 1456) of the slot untouched), 1457 ..
    1484 intact but not placed."""
    dg = [O.build_datagram(ln, _payload(ln, ln)) for ln in range(1485)]
    win = Window(1500)
    ok, place, ack = accept(W, *_slots(dg, 1504), 0, win)
    assert ok.all()
    assert np.array_equal(place[:1457], np.arange(1457)) and (place[1457:] == M.NOT_PLACED).all()
    assert ack == 1457
    img = win.h_out.reshape(1500, 1456)
    for ln in (0, 1, 15, 16, 17, 1455):
        assert (img[ln, ln:] == 0xA5).all() and img[ln, :ln].tobytes() == _payload(ln, ln)


def test_corruption(W):
    """A bit flipped in a payload or in the checksum: ok 0, slot EMPTY, image untouched, ack
    stops at the gap.  A bit flipped in seqNum: still ok (the CRC covers the payload only)
    and placed where the header says, as the reference would."""
    dg = [bytearray(O.build_datagram(s, _payload(s, 1456))) for s in range(8)]
    dg[2][16 + 1455] ^= 0x80  # payload, last byte
    dg[5][13] ^= 0x04         # checksum
    dg[6][7] ^= 0x01          # seqNum 6 -> 7: arrives before the real 7, so it wins slot 7
    win = Window(8)
    ok, place, ack = accept(W, *_slots([bytes(d) for d in dg], 1472), 0, win)
    assert ok.tolist() == [1, 1, 0, 1, 1, 0, 1, 1]
    assert place.tolist() == [0, 1, M.NOT_PLACED, 3, 4, M.NOT_PLACED, 7, M.NOT_PLACED]
    assert ack == 2 and win.h_slot_len[2] == M.EMPTY and win.h_slot_len[5] == M.EMPTY and win.h_slot_len[6] == M.EMPTY
    img = win.h_out.reshape(8, 1456)
    assert (img[[2, 5, 6]] == 0xA5).all() and img[7].tobytes() == _payload(6, 1456)


def test_window_edges_and_empty_window(W):
    seq0, window = 1000, 16
    seqs = [seq0 - 1, seq0, seq0 + window - 1, seq0 + window]
    dg = [O.build_datagram(s, _payload(s, 1456 - 16 * k)) for k, s in enumerate(seqs)]
    ring, _, rl = _slots(dg, 1472)
    win = Window(window)
    ok, place, ack = accept(W, ring, 1472, rl, seq0, win)
    assert ok.all() and place.tolist() == [M.NOT_PLACED, 0, window - 1, M.NOT_PLACED] and ack == seq0 + 1
    # a window that starts at seq 0: seq 2^32 - 1 lies below it (unsigned distance 2^32 - 1)
    win = Window(window)
    dg = [O.build_datagram(s, _payload(s, 100)) for s in (0xFFFFFFFF, 0, window - 1, window)]
    _, place, ack = accept(W, *_slots(dg, 1472), 0, win)
    assert place.tolist() == [M.NOT_PLACED, 0, window - 1, M.NOT_PLACED] and ack == 1
    # window == 0: nothing placed, ok still written, ack == seq0; d_place NULL is allowed
    for with_place in (True, False):
        win = Window(0)
        ok, place, ack = accept(W, ring, 1472, rl, seq0, win, with_place=with_place)
        assert ok.all() and (place == M.NOT_PLACED).all() and ack == seq0
    # n == 0: ack from the existing state
    win = Window(4)
    accept(W, *_slots([O.build_datagram(7, b"abc"), O.build_datagram(8, b"")], 1472), 7, win)
    ok, place, ack = accept(W, np.zeros(0, np.uint8), 1472, np.zeros(0, np.uint32), 7, win)
    assert ack == 9


def test_non_data_types_runts_and_long_lengths(W):
    stride = 1504
    dg = [O.build_datagram(k, _payload(k, 200 + k), ptype=t) for k, t in enumerate((0, 1, 3, 7))]
    dg.append(O.build_datagram(4, _payload(4, 300)))          # the one placeable datagram
    dg += [O.build_datagram(5, _payload(5, 64))] * 4            # runts and over-long, below
    ring, _, rl = _slots(dg, stride)
    rl[5:9] = [0, 15, stride + 1, 5000]
    win = Window(16)
    ok, place, ack = accept(W, ring, stride, rl, 0, win)
    assert ok.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert place.tolist() == [M.NOT_PLACED] * 4 + [4] + [M.NOT_PLACED] * 4 and ack == 0


def test_first_wins_no_tearing(W):
    """2048 datagrams (many workgroups) with one seq, each its own full-length payload and
    valid checksum: the slot is datagram 0's payload exactly; with datagram 0 corrupt,
    datagram 1's; a later call never changes a filled slot."""
    n, stride = 2048, 1472
    dg = [O.build_datagram(3, _payload(i, 1456)) for i in range(n)]
    ring, _, rl = _slots(dg, stride)
    win = Window(8)
    ok, place, ack = accept(W, ring, stride, rl, 0, win)
    assert ok.all() and place.tolist() == [3] + [M.NOT_PLACED] * (n - 1) and ack == 0
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(0, 1456)
    # second call, other valid bytes for the filled slot: nothing changes
    ok, place, _ = accept(W, ring[stride:], stride, rl[1:], 0, win)
    assert ok.all() and (place == M.NOT_PLACED).all()
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(0, 1456)
    # datagram 0 corrupt: datagram 1 wins
    ring2 = ring.copy()
    ring2[16 + 77] ^= 0x02
    win = Window(8)
    ok, place, _ = accept(W, ring2, stride, rl, 0, win)
    assert ok.tolist() == [0] + [1] * (n - 1) and place.tolist() == [M.NOT_PLACED, 3] + [M.NOT_PLACED] * (n - 2)
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(1, 1456)


def test_two_batch_window(W):
    """Evens first, then odds plus re-sent evens: the state carries over, ack moves from
    seq0 + 1 to seq0 + window, the final image is exact."""
    seq0, window, stride = 0xFFFFFFF8, 32, 1504
    lens = [1456] * (window - 1) + [333]
    dg = [O.build_datagram((seq0 + s) & M.M32, _payload(s, lens[s])) for s in range(window)]
    win = Window(window)
    _, _, ack = accept(W, *_slots(dg[0::2], stride), seq0, win)
    assert ack == (seq0 + 1) & M.M32
    resent = [O.build_datagram((seq0 + s) & M.M32, _payload(s + 99, lens[s])) for s in (0, 4, 30)]  # other bytes
    _, place, ack = accept(W, *_slots(dg[1::2] + resent, stride), seq0, win)
    assert place.tolist() == list(range(1, window, 2)) + [M.NOT_PLACED] * 3 and ack == (seq0 + window) & M.M32
    want = b"".join(_payload(s, lens[s]) for s in range(window))
    assert win.h_out[:len(want)].tobytes() == want


@pytest.mark.parametrize("stride,ring_off,out_off", [(1500, 1, 0), (1472, 0, 4), (1472, 0, 0), (1504, 0, 0),
                                                     (1500, 1, 4)])
def test_alignment(W, stride, ring_off, out_off):
    """The 16-B vector path (aligned ring and image) and the exact path for any other
    alignment give the same bytes."""
    n = 200
    rng = np.random.default_rng(stride + ring_off)
    lens = rng.integers(0, min(1456, stride - 16) + 1, n)
    lens[:8] = min(1456, stride - 16)
    perm = rng.permutation(n)
    dg = [O.build_datagram(int(s), _payload(int(s), int(lens[s]))) for s in perm]
    win = Window(n, out_off=out_off)
    ok, place, ack = accept(W, *_slots(dg, stride), 0, win, ring_off=ring_off)
    assert ok.all() and np.array_equal(place, perm.astype(np.uint32)) and ack == n


def test_graph_replay(W):
    """memset(slot_len) + accept captured on a side stream (a linear graph), replayed
    twice, the second time over other ring contents: model-exact both times."""
    n, stride, window, seq0 = 300, 1472, 256, 50
    rng = np.random.default_rng(9)

    def batch(salt):
        seqs = rng.integers(seq0 - 10, seq0 + window + 10, n)
        dg = [bytearray(O.build_datagram(int(s), _payload(int(s) + salt, int(rng.integers(0, 1457))))) for s in seqs]
        for i in range(0, n, 17):
            dg[i][16 + (len(dg[i]) - 16) // 2 if len(dg[i]) > 16 else 12] ^= 0x40
        ring, _, rl = _slots([bytes(d) for d in dg], stride)
        return ring, rl

    ring, rl = batch(0)
    d, r = torch.from_numpy(ring).cuda(), dev_s32(rl)
    win = Window(window)
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    place = torch.zeros(n, dtype=torch.int32, device="cuda")
    ack = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        win.slot_len.fill_(-1)
        W.accept_data_packets(d, stride, r, n, seq0, window, win.out, win.slot_len, ok, place, ack)

    g, _ = capture(call)
    for salt in (0, 1000):
        if salt:
            ring, rl = batch(salt)
            d.copy_(torch.from_numpy(ring))
            r.copy_(dev_s32(rl))
        win.out.fill_(0xA5)
        ok.fill_(9)
        place.fill_(9)
        ack.fill_(9)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        w_ok, w_place, w_out, w_sl, w_ack = M.accept(ring, stride, rl, seq0, window, win.h_out, win.h_slot_len)
        assert np.array_equal(ok.cpu().numpy(), w_ok) and np.array_equal(u32(place[:n]), w_place)
        assert np.array_equal(u32(win.slot_len[:window]), w_sl)
        assert np.array_equal(win.out.cpu().numpy(), w_out) and int(u32(ack[:1])[0]) == w_ack
        assert 0 < (w_place != M.NOT_PLACED).sum() < n
    assert_no_data_error(W)
