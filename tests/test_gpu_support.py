"""CPU test of tests/gpu_support.py's guards: every "nothing written past the array" claim of
the protocol GPU tests rests on get() failing when a guard byte changed, and on the mismatch
reporter naming the right place.  The buffers live on the CPU device, so no GPU is needed."""
import numpy as np
import pytest

from gpu_support import Bytes, Words, assert_bytes_equal


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
