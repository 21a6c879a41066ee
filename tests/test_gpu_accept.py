"""GPU tests of the device-side receive, wtp_accept_data_packets: every output (ok, place,
slot_len, out, ack) is compared element-wise with the sequential model
(tests/accept_model.py, ok pinned to the reference through oracle.verify_datagrams).
Every call goes through gpu_support.DevWindow: `out` is pre-filled with 0xA5, so a byte that
must stay untouched is checkable; the image, the ring and ok sit between guard bytes, place,
ack, slot_len and recv_len have guard words, and the ring and recv_len are read back."""
import numpy as np
import pytest

import accept_model as M
import oracle as O
from gpu_support import W  # noqa: F401 (fixture)
from gpu_support import Bytes, DevWindow, Words, assert_no_data_error, capture, datagram_ring, dev_s32
from gpu_support import replay_each_then_together, s32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _slots(dgrams, stride):
    """(ring, stride, recv_len) of `dgrams` (bytes, none longer than a slot) in `stride`-byte
    slots: DevWindow.accept's arguments."""
    ring, rl = datagram_ring(dgrams, stride)
    return ring, stride, rl


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
    win = DevWindow(n)
    ok, place, ack = win.accept(W, ring.cpu().numpy(), stride, rl.cpu().numpy().view(np.uint32), seq0)
    assert ok.all() and np.array_equal(place, perm.astype(np.uint32))
    assert ack == (seq0 + 64) & M.M32
    assert torch.equal(win.img.payload[:total], src)
    assert win.h_slot_len.tolist() == [1456] * 63 + [1356]


@pytest.mark.parametrize("ring_off,out_off", [(0, 0), (1, 0), (0, 4)])
def test_every_length(W, ring_off, out_off):
    """Payload lengths 0 .. 1484, one datagram each, seq = length, in 1504-B slots: up to
    1456 placed (bytes [len, 1456) of the slot untouched), 1457 .. 1484 intact but not placed;
    on the vector path (byte-exact vector tails: a kernel that drops the tail bytes behind the
    last whole vector fails here) and, with the ring or the image off the 16-B grid, every
    length on the bytewise path (a byte loop that rounds its length or starts a lane at the
    wrong byte fails there)."""
    dg = [O.build_datagram(ln, _payload(ln, ln)) for ln in range(1485)]
    win = DevWindow(1500, out_off=out_off)
    ok, place, ack = win.accept(W, *_slots(dg, 1504), 0, ring_off=ring_off)
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
    win = DevWindow(8)
    ok, place, ack = win.accept(W, *_slots([bytes(d) for d in dg], 1472), 0)
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
    win = DevWindow(window)
    ok, place, ack = win.accept(W, ring, 1472, rl, seq0)
    assert ok.all() and place.tolist() == [M.NOT_PLACED, 0, window - 1, M.NOT_PLACED] and ack == seq0 + 1
    # a window that starts at seq 0: seq 2^32 - 1 lies below it (unsigned distance 2^32 - 1)
    win = DevWindow(window)
    dg = [O.build_datagram(s, _payload(s, 100)) for s in (0xFFFFFFFF, 0, window - 1, window)]
    _, place, ack = win.accept(W, *_slots(dg, 1472), 0)
    assert place.tolist() == [M.NOT_PLACED, 0, window - 1, M.NOT_PLACED] and ack == 1
    # window == 0: nothing placed, ok still written, ack == seq0; d_place NULL is allowed
    for with_place in (True, False):
        win = DevWindow(0)
        ok, place, ack = win.accept(W, ring, 1472, rl, seq0, with_place=with_place)
        assert ok.all() and (place == M.NOT_PLACED).all() and ack == seq0
    # n == 0: ack from the existing state
    win = DevWindow(4)
    win.accept(W, *_slots([O.build_datagram(7, b"abc"), O.build_datagram(8, b"")], 1472), 7)
    ok, place, ack = win.accept(W, np.zeros(0, np.uint8), 1472, np.zeros(0, np.uint32), 7)
    assert ack == 9


def test_non_data_types_runts_and_long_lengths(W):
    stride = 1504
    dg = [O.build_datagram(k, _payload(k, 200 + k), ptype=t) for k, t in enumerate((0, 1, 3, 7))]
    dg.append(O.build_datagram(4, _payload(4, 300)))          # the one placeable datagram
    dg += [O.build_datagram(5, _payload(5, 64))] * 4            # runts and over-long, below
    ring, _, rl = _slots(dg, stride)
    rl[5:9] = [0, 15, stride + 1, 5000]
    win = DevWindow(16)
    ok, place, ack = win.accept(W, ring, stride, rl, 0)
    assert ok.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert place.tolist() == [M.NOT_PLACED] * 4 + [4] + [M.NOT_PLACED] * 4 and ack == 0


def test_first_wins_no_tearing(W):
    """2048 datagrams (many workgroups) with one seq, each its own full-length payload and
    valid checksum: the slot is datagram 0's payload exactly; with datagram 0 corrupt,
    datagram 1's; a later call never changes a filled slot."""
    n, stride = 2048, 1472
    dg = [O.build_datagram(3, _payload(i, 1456)) for i in range(n)]
    ring, _, rl = _slots(dg, stride)
    win = DevWindow(8)
    ok, place, ack = win.accept(W, ring, stride, rl, 0)
    assert ok.all() and place.tolist() == [3] + [M.NOT_PLACED] * (n - 1) and ack == 0
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(0, 1456)
    # second call, other valid bytes for the filled slot: nothing changes
    ok, place, _ = win.accept(W, ring[stride:], stride, rl[1:], 0)
    assert ok.all() and (place == M.NOT_PLACED).all()
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(0, 1456)
    # datagram 0 corrupt: datagram 1 wins
    ring2 = ring.copy()
    ring2[16 + 77] ^= 0x02
    win = DevWindow(8)
    ok, place, _ = win.accept(W, ring2, stride, rl, 0)
    assert ok.tolist() == [0] + [1] * (n - 1) and place.tolist() == [M.NOT_PLACED, 3] + [M.NOT_PLACED] * (n - 2)
    assert win.h_out[3 * 1456:4 * 1456].tobytes() == _payload(1, 1456)


def test_loser_longer_than_winner(W):
    """600 intact datagrams with one seq and lengths 100, 1456, 0, 1455, 101, then random: the
    slot holds datagram 0's 100 bytes and bytes [100, 1456) are still 0xA5 (a loser of the race
    that wrote the bytes past the winner's length, or a kernel that copied before it knew the
    owner, fails here).  Then the same datagrams led by the 0-length one, for another slot: it
    is filled with length 0 and no byte of it changes; and a full-length datagram re-sent to
    that slot changes nothing (a kernel that took a stored length 0 for "empty" fails here)."""
    n, stride = 600, 1472
    rng = np.random.default_rng(600)
    lens = [100, 1456, 0, 1455, 101] + rng.integers(0, 1457, n - 5).tolist()
    win = DevWindow(8)
    ring, _, rl = _slots([O.build_datagram(3, _payload(i, ln)) for i, ln in enumerate(lens)], stride)
    ok, place, ack = win.accept(W, ring, stride, rl, 0)
    assert ok.all() and place.tolist() == [3] + [M.NOT_PLACED] * (n - 1) and ack == 0
    slot = win.h_out[3 * 1456:4 * 1456]
    assert slot[:100].tobytes() == _payload(0, 100) and (slot[100:] == 0xA5).all() and win.h_slot_len[3] == 100
    lens[0], lens[2] = lens[2], lens[0]
    ring, _, rl = _slots([O.build_datagram(5, _payload(i, ln)) for i, ln in enumerate(lens)], stride)
    ok, place, _ = win.accept(W, ring, stride, rl, 0)
    assert ok.all() and place.tolist() == [5] + [M.NOT_PLACED] * (n - 1)
    assert win.h_slot_len[5] == 0 and (win.h_out[5 * 1456:6 * 1456] == 0xA5).all()
    ok, place, _ = win.accept(W, *_slots([O.build_datagram(5, _payload(9, 1456))], stride), 0)
    assert ok.all() and place.tolist() == [M.NOT_PLACED]
    assert win.h_slot_len.tolist() == [M.EMPTY] * 3 + [100, M.EMPTY, 0] + [M.EMPTY] * 2
    assert (win.h_out[5 * 1456:6 * 1456] == 0xA5).all()


def test_filled_slots_with_any_stored_value(W):
    """Slots that hold 0, 1, 1456, 1457 and 0x7FFFFFFF on entry (any value below 0x80000000 is
    a filled slot; wtp_rx_deliver and wtp_rx_advance carry such values unchanged), then EMPTY
    ones.  Intact datagrams arrive for all five: none is placed, the values and the image are
    unchanged, and the ACK counts them as filled.  A claim that compared lengths instead of
    taking the minimum with EMPTY on top, or an ACK scan that looked for "<= 1456", fails
    here."""
    stored = [0, 1, 1456, 1457, 0x7FFFFFFF]
    win = DevWindow(9, slot_len=stored + [M.EMPTY] * 4)
    dg = [O.build_datagram(50 + s, _payload(s, 1456 - 16 * s)) for s in (4, 0, 3, 1, 2)]
    ok, place, ack = win.accept(W, *_slots(dg, 1472), 50)
    assert ok.all() and (place == M.NOT_PLACED).all() and ack == 55
    assert win.h_slot_len.tolist() == stored + [M.EMPTY] * 4 and (win.h_out == 0xA5).all()
    # the same again with a placeable datagram for slot 6 between them: only that slot changes
    dg.insert(2, O.build_datagram(56, _payload(6, 777)))
    ok, place, ack = win.accept(W, *_slots(dg, 1472), 50)
    assert ok.all() and place.tolist() == [M.NOT_PLACED] * 2 + [6] + [M.NOT_PLACED] * 3 and ack == 55
    assert win.h_slot_len.tolist() == stored + [M.EMPTY, 777] + [M.EMPTY] * 2


def test_two_batch_window(W):
    """Evens first, then odds plus re-sent evens: the state carries over, ack moves from
    seq0 + 1 to seq0 + window, the final image is exact."""
    seq0, window, stride = 0xFFFFFFF8, 32, 1504
    lens = [1456] * (window - 1) + [333]
    dg = [O.build_datagram((seq0 + s) & M.M32, _payload(s, lens[s])) for s in range(window)]
    win = DevWindow(window)
    _, _, ack = win.accept(W, *_slots(dg[0::2], stride), seq0)
    assert ack == (seq0 + 1) & M.M32
    resent = [O.build_datagram((seq0 + s) & M.M32, _payload(s + 99, lens[s])) for s in (0, 4, 30)]  # other bytes
    _, place, ack = win.accept(W, *_slots(dg[1::2] + resent, stride), seq0)
    assert place.tolist() == list(range(1, window, 2)) + [M.NOT_PLACED] * 3 and ack == (seq0 + window) & M.M32
    want = b"".join(_payload(s, lens[s]) for s in range(window))
    assert win.h_out[:len(want)].tobytes() == want


@pytest.mark.parametrize("stride,ring_off,out_off", [(1500, 1, 0), (1472, 0, 4), (1472, 0, 0), (1504, 0, 0),
                                                     (1500, 1, 4), (1472, 0, 8), (1472, 8, 0), (1504, 0, 1),
                                                     (1480, 0, 0), (1480, 8, 0), (1476, 0, 0), (1476, 4, 0),
                                                     (1488, 0, 0)])
def test_alignment(W, stride, ring_off, out_off):
    """The 16-B vector path (aligned source and destination) and the exact path for any other
    alignment give the same bytes.  The path is chosen per datagram: with a stride of 8 or 4
    mod 16, every second or fourth datagram of one batch has an aligned source, so both paths
    run in one launch, behind verify's general kernel (a kernel that chose the path once per
    batch, or from the ring's base address, would store vectors at misaligned addresses or
    tear those slots).  Which datagrams take which path is computed from the device
    pointers."""
    n = 200
    rng = np.random.default_rng(stride + ring_off)
    lens = rng.integers(0, min(1456, stride - 16) + 1, n)
    lens[:8] = min(1456, stride - 16)
    perm = rng.permutation(n)
    dg = [O.build_datagram(int(s), _payload(int(s), int(lens[s]))) for s in perm]
    win = DevWindow(n, out_off=out_off)
    ok, place, ack = win.accept(W, *_slots(dg, stride), 0, ring_off=ring_off)
    assert ok.all() and np.array_equal(place, perm.astype(np.uint32)) and ack == n
    src = win.ring.t.data_ptr() + np.arange(n) * stride + 16
    dst = win.out.data_ptr() + place.astype(np.int64) * 1456
    aligned = (src | dst) % 16 == 0
    vector = "both" if stride in (1480, 1476) else "all" if (stride | ring_off | out_off) % 16 == 0 else "none"
    assert {"all": aligned.all(), "none": not aligned.any(), "both": aligned.any() and not aligned.all()}[vector]
    if vector == "both":  # full-length and short payloads on both paths
        assert {bool(a) for a, s in zip(aligned, perm) if lens[s] == 1456} == {True, False}
        assert {bool(a) for a, s in zip(aligned, perm) if 0 < lens[s] < 1456} == {True, False}


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097])
def test_batch_sizes_around_the_group_sizes(W, n):
    """n around the 4 datagrams of a wave and the 16 of a workgroup in k_accept_place and the
    256 of a workgroup in k_accept_claim, all seqs distinct and permuted, lengths 0 .. 1456
    with both ends present, the last two datagrams placeable.  A grid that is one group short
    leaves the last datagrams' claims (0x80000000 | i) in slot_len or their payloads unplaced,
    which the exact comparison of slot_len and the image shows."""
    window, stride = n + 3, 1472
    rng = np.random.default_rng(n)
    slots = rng.permutation(window)[:n]
    lens = rng.integers(0, 1457, n)
    lens[-2:] = np.maximum(lens[-2:], 1)  # the last two bring bytes
    lens[:2] = [0, 1456][-min(n, 2):]  # n == 1: 1456 alone
    dg = [O.build_datagram(int(77 + s), _payload(int(s), int(ln))) for s, ln in zip(slots, lens)]
    win = DevWindow(window)
    ok, place, _ = win.accept(W, *_slots(dg, stride), 77)
    assert ok.all() and np.array_equal(place, slots.astype(np.uint32))
    assert 1456 in lens and (n < 3 or 0 in lens)
    assert np.array_equal(win.h_slot_len[slots], lens) and (win.h_slot_len < 0x80000000).sum() == n


def _mixed_batch(rng, n, seq0, window, salt=0, stride=1472):
    """n datagrams with seqs from 10 below to 10 past the window (duplicates within the batch
    as soon as n > window), random lengths, every 17th corrupt: (ring, recv_len) in
    `stride`-byte slots."""
    seqs = rng.integers(seq0 - 10, seq0 + window + 10, n)
    dg = [bytearray(O.build_datagram(int(s) & M.M32, _payload((int(s) & 0xFFFFF) + salt, int(rng.integers(0, 1457)))))
          for s in seqs]
    for i in range(0, n, 17):
        dg[i][16 + (len(dg[i]) - 16) // 2 if len(dg[i]) > 16 else 12] ^= 0x40
    ring, _, rl = _slots([bytes(d) for d in dg], stride)
    return ring, rl


@pytest.mark.parametrize("with_place,with_ack", [(True, True), (False, True), (True, False), (False, False)])
def test_optional_outputs(W, with_place, with_ack):
    """d_place and d_ack given or NULL, on a batch that places, rejects duplicates (of an
    earlier call and within the batch) and holds corrupt datagrams: the outputs that are given
    and the window state are exact, the ones that are not keep their sentinel.  Without d_ack
    the scan is skipped and the grid is sized by n alone; a kernel that dereferenced a NULL
    output, or whose placement depended on the scan's grid, fails here."""
    window, n, seq0 = 300, 500, 0xFFFFFF00
    rng = np.random.default_rng(300)
    win = DevWindow(window)
    ring, rl = _mixed_batch(rng, 60, seq0, window)
    win.accept(W, ring, 1472, rl, seq0)  # an earlier call fills some slots
    filled = int((win.h_slot_len != M.EMPTY).sum())
    ring, rl = _mixed_batch(rng, n, seq0, window, salt=5000)
    ok, place, _ = win.accept(W, ring, 1472, rl, seq0, with_place=with_place, with_ack=with_ack)
    placed = int((place != M.NOT_PLACED).sum())
    assert 0 < filled < window and 0 < placed < int(ok.sum()) < n
    assert int((win.h_slot_len != M.EMPTY).sum()) == filled + placed


# ---- the cumulative-ACK scan past one grid step ------------------------------------------------
BIG_WINDOW, BIG_SEQ0 = 262144 + 300, 0xFFFFFF00


@pytest.fixture(scope="module")
def big_image():
    """One image of BIG_WINDOW slots (about 382 MB) on the device, 0xA5 between guards, for all
    cases of test_ack_scan_past_one_grid_step; each case restores the slots it changed."""
    return Bytes(fill=0xA5, size=BIG_WINDOW * M.MAXP, front=64, back=64)


@pytest.mark.parametrize("case,empty,lead", [("a", [262150], 262150), ("b", [262143, 262149], 262143),
                                             ("c", [5, 262149], 5), ("d", [], BIG_WINDOW), ("e", [7, 262151], 262151)])
def test_ack_scan_past_one_grid_step(W, big_image, case, empty, lead):
    """window = 262144 + 300 with n = 3: the place grid is 1024 workgroups, so lanes 0 .. 299
    scan a second slot, 262144 slots on.  Every slot is filled (length 0) on entry but `empty`.
    a: the only EMPTY slot is found on a second step (a scan that ends after one step reports
    seq0 + window).  b: a first-step find of one lane beats a second-step find of another (an
    ACK that took the last writer instead of the lowest slot fails).  c: a lane stops at its
    first EMPTY slot, and the lower of two finds wins.  d: no EMPTY slot, ACK = seq0 + window
    across the 2^32 wrap.  e: an intact datagram arrives for slot 7: the slot is claimed, so
    its lane must count it as filled and walk on to slot 262151 (a lane that stopped at a
    claimed slot, or took a claim for EMPTY, reports seq0 + 7).  The image stays on the
    device: its first 8 slots are compared with the model, the rest with 0xA5."""
    window, seq0, stride, low = BIG_WINDOW, BIG_SEQ0, 1472, 8
    h_sl = np.zeros(window, dtype=np.uint32)
    h_sl[empty] = M.EMPTY
    corrupt = bytearray(O.build_datagram((seq0 + (empty[-1] if empty else 9)) & M.M32, _payload(1, 1456)))
    corrupt[16 + 700] ^= 0x08
    dg = [O.build_datagram(seq0, _payload(0, 1456)),                      # a duplicate of filled slot 0
          bytes(corrupt),                                                 # corrupt, for the highest EMPTY slot
          O.build_datagram((seq0 + 7) & M.M32, _payload(7, 1000)) if case == "e"
          else O.build_datagram((seq0 - 1) & M.M32, _payload(2, 64))]    # placeable (e), else below the window
    h_ring, _, h_rl = _slots(dg, stride)
    want_ok, want_place, want_out, want_sl, want_ack = M.accept(h_ring, stride, h_rl, seq0, window,
                                                                np.full(low * M.MAXP, 0xA5, np.uint8), h_sl)
    assert want_ack == (seq0 + lead) & M.M32 and want_ok.tolist() == [1, 0, 1]
    assert want_place.tolist() == [M.NOT_PLACED, M.NOT_PLACED, 7 if case == "e" else M.NOT_PLACED]
    sl, ring, rl = Words(h_sl), Bytes(h_ring, front=64, back=64), Words(h_rl)
    ok, place, ack = Bytes(fill=7, size=3, front=16), Words(12345, 3), Words(0x0BADACC0, 1)
    W.accept_data_packets(ring.t, stride, rl.t, 3, seq0, window, big_image.t, sl.t, ok.t, place.t, ack.t)
    torch.cuda.synchronize()
    got_low = big_image.payload[:low * M.MAXP].cpu().numpy()
    rest_untouched = bool((big_image.payload[low * M.MAXP:] == 0xA5).all())
    big_image.payload[:low * M.MAXP].fill_(0xA5)  # for the next case, whatever this one finds
    assert int(ack.get()[0]) == want_ack
    assert np.array_equal(ok.get(), want_ok) and np.array_equal(place.get(), want_place)
    assert np.array_equal(sl.get(), want_sl)
    assert np.array_equal(got_low, want_out) and rest_untouched
    big_image.check_guards()
    assert np.array_equal(ring.get(), h_ring) and np.array_equal(rl.get(), h_rl)
    assert W.LIB.wtp_last_kernel().decode() == "k_accept_place"
    assert_no_data_error(W)


# ---- graphs ---------------------------------------------------------------------------------------
class Replayed:
    """memset(slot_len) + accept on one (ring, window) set, captured on a side stream (a linear
    graph).  reset(salt) uploads another batch into the captured buffers and re-sentinels every
    output; check() compares with the model from an EMPTY window."""

    def __init__(self, W, n, stride, window, seq0, seed, ring_off=0, out_off=0):
        self.n, self.stride, self.window, self.seq0 = n, stride, window, seq0
        self.rng = np.random.default_rng(seed)
        self.win = win = DevWindow(window, out_off=out_off)
        win.stage(*self.batch(0), ring_off=ring_off)

        def call():
            win.slot_len.fill_(-1)
            W.accept_data_packets(win.ring.t, stride, win.rl.t, n, seq0, window, win.out, win.slot_len, win.ok.t,
                                  win.place.t, win.ack.t)

        self.graph, self.stream = capture(call)

    def batch(self, salt):
        return _mixed_batch(self.rng, self.n, self.seq0, self.window, salt, self.stride)

    def reset(self, salt):
        win = self.win
        ring, rl = self.batch(salt)
        win.ring.host[:], win.rl_host[:] = ring, rl
        win.ring.payload.copy_(torch.from_numpy(ring))
        win.rl.t.copy_(dev_s32(rl))
        win.img.payload.fill_(0xA5)
        win.ok.payload.fill_(win.OK_SENT)
        win.place.t.fill_(win.PLACE_SENT)
        win.ack.t.fill_(win.ACK_SENT)
        win.slot_len.fill_(int(s32([0x12345678])[0]))  # the captured memset resets it

    def check(self):
        win = self.win
        self.want = M.accept(win.ring.host, self.stride, win.rl_host, self.seq0, self.window, win.h_out, win.h_slot_len)
        win.check(self.want)
        assert 0 < (self.want[1] != M.NOT_PLACED).sum() < self.n


def test_graph_replay(W):
    """memset(slot_len) + accept captured on a side stream (a linear graph), replayed
    twice, the second time over other ring contents: model-exact both times."""
    g = Replayed(W, 300, 1472, 256, 50, seed=9)
    for salt in (0, 1000):
        g.reset(salt)
        torch.cuda.synchronize()
        g.graph.replay()
        torch.cuda.synchronize()
        g.check()
    assert_no_data_error(W)


def test_graphs_on_three_windows_replayed_together(W):
    """Three independent (ring, window) sets with their own strides, alignments and seq0, each
    a linear graph on its own stream: one replayed alone twice, then all three at once over
    other ring contents, each model-exact.  Calls on different windows share nothing (slots are
    claimed in the caller's d_slot_len); a kernel that kept a claim table, a counter or the ACK
    in library memory would mix the three up here."""
    g = Replayed(W, 300, 1472, 256, 0xFFFFFF80, seed=31)
    replay_each_then_together(g, [(0,), (1000,)],
                              lambda: (Replayed(W, 257, 1504, 100, 50, seed=32, out_off=4),
                                       Replayed(W, 200, 1500, 300, 7, seed=33, ring_off=1)),
                              [(2000,), (3000,), (4000,)])
    assert_no_data_error(W)


# ---- the randomised differential test -----------------------------------------------------------
@pytest.mark.parametrize("seed", list(M.FUZZ_SEEDS))
def test_fuzz_against_the_model(W, seed):
    """Three successive calls on one window per seed, over accept_model.fuzz_batch's corpus
    (placeable datagrams, duplicates of earlier calls and within the batch, seqs around and
    far from the window, corrupt payloads and checksums, other types, runts, over-long
    lengths, empty payloads), at the strides and offsets that choose verify's and the copy's
    paths, half the seeds next to the 2^32 wrap: every output of every call is model-exact
    with the state carried over.  It is the net under the targeted tests: a kernel that is
    wrong only for a combination of these (a duplicate of a zero-length slot next to the wrap,
    a runt whose stale header names a free slot, a claim lost between two calls) differs from
    the model in some output here.  tests/test_accept_model.py shows without a GPU that the
    corpus reaches every one of these verdicts."""
    rng, window, seq0, stride, ring_off, out_off, ns = M.fuzz_case(seed)
    win = DevWindow(window, out_off=out_off)
    for n in ns:
        ring, rl, _ = M.fuzz_batch(rng, seq0, window, stride, win.h_slot_len, n)
        win.accept(W, ring, stride, rl, seq0, ring_off=ring_off)
