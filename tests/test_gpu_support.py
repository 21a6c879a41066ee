"""CPU test of tests/gpu_support.py's guards: every "nothing written past the array" claim of
the protocol GPU tests rests on get() failing when a guard byte changed, and on the mismatch
reporter naming the right place.  The buffers live on the CPU device, so no GPU is needed."""
import numpy as np
import pytest

import accept_model
import oracle as O
from gpu_support import Bytes, DevWindow, Words, assert_bytes_equal, datagram_ring, s32, torch


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_words_guard(dtype):
    w = Words(12345, 7, dtype, device="cpu")
    assert w.t.numel() == 7 and w.get().tolist() == [12345] * 7
    w.t[6] = 99  # inside the array: returned, not an error
    assert w.get().tolist() == [12345] * 6 + [99]
    w.buf[7] = 99  # the first word past it
    with pytest.raises(AssertionError):
        w.get()
    empty = Words(np.zeros(0, dtype), dtype=dtype, device="cpu")
    assert empty.t.numel() == 1 and empty.get().size == 0  # the view of an empty array is one guard word
    empty.t[0] = 0
    with pytest.raises(AssertionError):
        empty.get()


@pytest.mark.parametrize("kw", [dict(), dict(off=5), dict(off=3, front=4096, back=4096), dict(front=64, back=64, guard=0xA5),
                                dict(off=1, front=4096, flush=True)])
def test_bytes_guards(kw):
    host = np.arange(100, dtype=np.uint8)
    lo = kw.get("front", 0) + kw.get("off", 0)

    def fresh():
        b = Bytes(host, device="cpu", **kw)
        assert b.lo == lo and b.t.data_ptr() == b.buf.data_ptr() + lo and np.array_equal(b.get(), host)
        assert b.buf.numel() == lo + 100 + (0 if kw.get("flush") else kw.get("back", 16))
        return b

    b = fresh()
    b.t[0], b.t[99] = 200, 201  # the payload's first and last byte: returned, not an error
    got = b.get()
    assert got[0] == 200 and got[99] == 201 and np.array_equal(got[1:99], host[1:99])
    b.check_guards()
    if not kw.get("flush"):
        b = fresh()
        b.t[100] ^= 1  # the first byte past the payload
        with pytest.raises(AssertionError):
            b.get()
        with pytest.raises(AssertionError):
            b.check_guards()
    if lo:
        b = fresh()
        b.buf[lo - 1] ^= 1  # the last byte before it
        with pytest.raises(AssertionError):
            b.get()
        with pytest.raises(AssertionError):
            b.check_guards()


def test_bytes_filled_with_the_guard_or_another_byte():
    ring = Bytes(fill=0xA5, size=48, off=1, front=64, back=64, guard=0xA5, device="cpu")
    assert ring.buf.numel() == 64 + 1 + 48 + 64 and (ring.get() == 0xA5).all()
    img = Bytes(fill=0x3C, size=48, guard=0xC3, device="cpu")
    assert (img.get() == 0x3C).all() and (img.buf[48:] == 0xC3).all()


def test_dev_window_checks_every_output_guard_and_input():
    """DevWindow.check on the CPU device, with the model's own result written into the staged
    buffers in place of the call: it passes, it passes with an output withheld only if that
    output still holds its sentinel, and it fails for one wrong element of each output, one
    changed byte in front of or behind the image, behind ok, place, ack or slot_len, and one
    changed byte of the ring or of recv_len."""
    dg = [O.build_datagram(s, bytes([s]) * (100 + s)) for s in (2, 0, 2, 9)]
    ring, rl = datagram_ring(dg, 1472)
    want = accept_model.accept(ring, 1472, rl, 0, 4, np.full(4 * 1456, 0xA5, np.uint8), np.full(4, accept_model.EMPTY, np.uint32))
    assert want[1].tolist() == [2, 0, accept_model.NOT_PLACED, accept_model.NOT_PLACED] and want[4] == 1

    def staged(with_place=True, with_ack=True):
        win = DevWindow(4, out_off=4, device="cpu")
        assert win.out.data_ptr() % 16 == 4 and win.slot_len.numel() == 4
        win.stage(ring, rl, ring_off=1)
        assert win.ring.t.data_ptr() % 16 == 1
        win.ok.payload.copy_(torch.from_numpy(want[0]))
        if with_place:
            win.place.t.copy_(torch.from_numpy(s32(want[1])))
        win.img.payload.copy_(torch.from_numpy(want[2]))
        win.slot_len.copy_(torch.from_numpy(s32(want[3])))
        if with_ack:
            win.ack.t[0] = want[4]
        return win

    staged().check(want)
    staged(with_place=False).check(want, with_place=False)
    staged(with_ack=False).check(want, with_ack=False)
    spoil = [lambda w: w.ok.payload[3].fill_(0), lambda w: w.place.t[2].fill_(2), lambda w: w.slot_len[1].fill_(0),
             lambda w: w.img.payload[2 * 1456 + 102].fill_(2), lambda w: w.ack.t[0].fill_(2),
             lambda w: w.img.buf[w.img.lo - 1].fill_(0), lambda w: w.img.payload[4 * 1456 - 1].fill_(0),
             lambda w: w.img.t[4 * 1456].fill_(0), lambda w: w.ok.t[4].fill_(0), lambda w: w.ok.buf[15].fill_(0),
             lambda w: w.place.buf[4].fill_(0), lambda w: w.ack.buf[1].fill_(0), lambda w: w.sl.buf[4].fill_(0),
             lambda w: w.ring.payload[1472 * 3 + 1471].fill_(0x11), lambda w: w.ring.t[4 * 1472].fill_(0),
             lambda w: w.rl.t[3].fill_(16), lambda w: w.rl.buf[4].fill_(0)]
    for k, f in enumerate(spoil):
        win = staged()
        f(win)
        with pytest.raises(AssertionError):
            win.check(want)
            pytest.fail(f"spoiler {k} went unnoticed")
    for kw in (dict(with_place=False), dict(with_ack=False)):  # a withheld output that was written after all
        with pytest.raises(AssertionError):
            staged().check(want, **kw)


def test_mismatch_reporter():
    want = np.arange(4 * 1472, dtype=np.uint32).astype(np.uint8)
    assert_bytes_equal(want.copy(), want, 1472, "equal arrays pass")
    got = want.copy()
    got[2 * 1472 + 17] ^= 0x40  # one planted difference: unit 2, byte 17
    with pytest.raises(AssertionError, match=r"^1 bytes differ, first at 2961: unit 2, byte 17 \(slot 2 of the ring\)$"):
        assert_bytes_equal(got, want, 1472, lambda unit: f"slot {unit} of the ring")
    got[3 * 1472] ^= 1  # a later one changes the count only
    with pytest.raises(AssertionError, match=r"^2 bytes differ, first at 2961: unit 2, byte 17 \(context\)$"):
        assert_bytes_equal(got, want, 1472, "context")


# ---- the helpers of tests/test_gpu_wide.py, with 2^12 and 2^13 in place of 2^31 and 2^32 --------
SMALL_BOUNDS = (1 << 12, 1 << 13)


@pytest.mark.parametrize("nbytes", [0, 1, 99, 100, 101, (1 << 12) + 37, (1 << 13) + 5, 10 * 100])
@pytest.mark.parametrize("off", [0, 5])
def test_periodic_buffer_and_its_crc(nbytes, off):
    from gpu_support import periodic, periodic_crc
    period = O.synth_fill_np(100, start_byte=7)
    mem = periodic(period, nbytes, off=off, device="cpu")
    want = np.tile(period, nbytes // 100 + 1)[:nbytes]
    assert mem.t.data_ptr() % 16 == off and np.array_equal(mem.get(), want)
    assert periodic_crc(period, nbytes) == O.crc32(want)


def test_sparse_ring_and_its_check():
    from gpu_support import SparseRing, be_words, slots
    n, stride, width = 37, 240, 24   # 37 * 240 > 2^13
    rng = np.random.default_rng(5)
    host_rows = rng.integers(0, 256, (n, width), dtype=np.uint8)
    host_rows[host_rows == 0xEE] = 1
    rows = torch.from_numpy(host_rows)
    want = np.full(3 + n * stride + 64, 0xEE, np.uint8)
    for i in range(n):
        want[3 + i * stride:3 + i * stride + width] = host_rows[i]

    def fresh():
        r = SparseRing(n, stride, rows, off=3, device="cpu")
        assert r.t.data_ptr() % 16 == 3 and np.array_equal(r.buf.numpy(), want)
        return r

    fresh().assert_rows(rows)
    fresh().assert_rows(lambda a, b: rows[a:b], width)
    assert torch.equal(fresh().rows(width, 17, 2), rows[17:19])
    assert torch.equal(slots(fresh().t, n, stride, width), rows)
    # one changed byte anywhere is noticed: in a row, in a tail just below a boundary, in front, behind
    for at in (3 + 17 * stride + 5, 3 + 17 * stride + width, (1 << 12) - 1, (1 << 13) - 1, 0, 2, 3 + n * stride,
               3 + n * stride + 63):
        r = fresh()
        r.buf[at] ^= 0x10
        with pytest.raises(AssertionError):
            r.assert_rows(rows)
    got = be_words([torch.tensor([2, 0x01020304]), torch.tensor([0xFFFFFFFF, 7])]).numpy()
    assert got.tolist() == [[0, 0, 0, 2, 255, 255, 255, 255], [1, 2, 3, 4, 0, 0, 0, 7]]


def test_assert_filled_and_straddles():
    from gpu_support import assert_filled, assert_straddles
    t = torch.full((1000,), 9, dtype=torch.uint8)
    assert_filled(t, 9, piece=64)
    t[777] = 8
    with pytest.raises(AssertionError, match="element 777 is 8"):
        assert_filled(t, 9, piece=64)
    stride = 240
    starts = np.arange(37) * stride
    lens = np.full(37, 200)
    # 17 * 240 = 4080 < 4096 < 4280 and 34 * 240 = 8160 < 8192 < 8360
    assert_straddles(starts, lens, stride, SMALL_BOUNDS)
    for drop in (16, 17, 34):   # the entry that ends below 2^12, and the ones that contain 2^12 and 2^13
        keep = np.arange(37) != drop
        short = np.where(keep, lens, 0)
        with pytest.raises(AssertionError):
            assert_straddles(starts, short, stride, SMALL_BOUNDS)
    with pytest.raises(AssertionError, match="begins at or above 0x2000"):
        assert_straddles(starts[:35], lens[:35], stride, SMALL_BOUNDS)
    from gpu_support import BOUNDS, ODD_STRIDE, WIDE_N, WIDE_STRIDE, straddling_stride
    assert_straddles(np.arange(4100) * ODD_STRIDE, np.full(4100, 16), ODD_STRIDE, BOUNDS)
    assert straddling_stride(240, 200, bounds=SMALL_BOUNDS) == 240 and straddling_stride(256, 200, bounds=SMALL_BOUNDS) == 260
    assert straddling_stride(WIDE_STRIDE, 1025, step=16) == WIDE_STRIDE and WIDE_STRIDE % 16 == 0
    assert_straddles(np.arange(WIDE_N) * WIDE_STRIDE, np.full(WIDE_N, 1472), WIDE_STRIDE, BOUNDS)
    assert_straddles(np.arange(40) * 256, np.full(40, 256), 256, SMALL_BOUNDS, contains=False)  # a stride that divides them
