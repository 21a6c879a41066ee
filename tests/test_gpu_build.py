"""GPU tests of the fixed-length DATA builder, wtp_build_data_packets: the fused braided path
(16-B aligned buffers and slots, stride <= 16384) and the three-step path (k_wire_copy, CRC,
k_wire_header: any other alignment or stride, and the short last chunk).  Every call's whole
wire ring is compared with oracle.build_datagram chunk by chunk: the ring is pre-filled with
0xA5 between guard bytes, so every slot tail [16 + len, stride) and everything around the ring
must be unchanged; d_wire_len is exact and has guard words; the payload buffer sits between
guards and is read back."""
import numpy as np
import pytest

import accept_model as M
import oracle as O
from gpu_support import W  # noqa: F401 (fixture)
from gpu_support import Bytes, DevWindow, Words, assert_bytes_equal, assert_no_data_error

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, SENT, WSENT, GUARD = M.MAXP, 12345, 0xA5, 64


def build(W, total, stride=1472, pay_off=0, wire_off=0, with_len=True, seq0=7):
    """One wtp_build_data_packets of `total` synthetic bytes `pay_off` bytes past a 16-B
    aligned address into a sentinel-filled ring `wire_off` bytes past one; asserts every output
    and every untouched byte; returns (payload, wire, wire_len) as the oracle has them, and the
    device ring and lengths (Bytes, Words)."""
    host = O.synth_fill_np(total, start_byte=total + stride + pay_off)
    pay = Bytes(host, off=pay_off, front=GUARD, back=GUARD)
    nch = (total + MAXP - 1) // MAXP
    wire = Bytes(fill=WSENT, size=nch * stride, off=wire_off, front=GUARD, back=GUARD)
    wl = Words(SENT, nch)
    fused = pay_off % 16 == 0 and wire_off % 16 == 0 and stride % 16 == 0 and stride <= 16384
    assert pay.t.data_ptr() % 16 == pay_off % 16 and wire.t.data_ptr() % 16 == wire_off % 16
    W.build_data_packets(pay.t, total, seq0, wire.t, stride, wl.t if with_len else None)
    torch.cuda.synchronize()
    want = np.full(nch * stride, WSENT, dtype=np.uint8)
    want_wl = np.zeros(nch, dtype=np.uint32)
    for i in range(nch):
        d = O.build_datagram((seq0 + i) & M.M32, host[i * MAXP:(i + 1) * MAXP].tobytes())
        want[i * stride:i * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
        want_wl[i] = len(d)
    path = (lambda i: "fused" if fused and i < total // MAXP else "three-step")
    assert_bytes_equal(wire.get(), want, stride, lambda i: f"slot {i} of {nch}, {path(i)} path, wire_len {want_wl[i]}")
    assert np.array_equal(wl.get(), want_wl if with_len else np.full(nch, SENT, np.uint32))
    assert np.array_equal(pay.get(), host)  # the payloads are only read
    assert_no_data_error(W)
    return host, want, want_wl, wire, wl


PATHS = [pytest.param(0, id="fused"), pytest.param(1, id="three-step")]


@pytest.mark.parametrize("pay_off", PATHS)
@pytest.mark.parametrize("tail", [0, 333])
@pytest.mark.parametrize("nch", [1, 2, 3, 4, 5, 63, 64, 65, 257, 4099])
def test_chunk_counts(W, nch, tail, pay_off):
    """nch full chunks around the braid's and the copy's group sizes, alone or followed by a
    333-byte chunk, on the fused path and (payloads one byte off) the three-step path.  A
    workgroup or grid-stride loop that is one chunk short, or a tail handled as a full chunk,
    leaves sentinel bytes in a slot or writes a slot's tail."""
    build(W, nch * MAXP + tail, pay_off=pay_off, seq0=nch)


@pytest.mark.parametrize("with_len", [True, False])
@pytest.mark.parametrize("pay_off", PATHS)
@pytest.mark.parametrize("r", [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 1453, 1454, 1455])
def test_tail_lengths(W, r, pay_off, with_len):
    """A last chunk of r bytes behind two full ones: k_wire_copy's dword loop ends in a byte
    tail of r % 4 bytes, and the tail's CRC is one general-kernel call.  With d_wire_len the
    CRCs of chunks [first, nch) are staged in d_wire_len[first ..) and then overwritten by the
    lengths, next to the entries the fused path wrote ([first - 1]); without it, fused chunks
    followed by a tail take the pool-scratch route.  A tail byte dropped or over-copied, a
    staged CRC left in d_wire_len, or a fused length overwritten shows in the exact
    comparison."""
    _, _, want_wl, _, wl = build(W, 2 * MAXP + r, pay_off=pay_off, with_len=with_len, seq0=r)
    assert want_wl.tolist() == [1472, 1472, 16 + r]
    if with_len:  # the handover: first == 2 on the fused path
        got = wl.get()
        assert got[1] == 1472 and got[2] == 16 + r


@pytest.mark.parametrize("stride", [1472, 1473, 1488, 1500])
@pytest.mark.parametrize("wire_off", [0, 1, 8])
@pytest.mark.parametrize("pay_off", [0, 1, 4, 8])
def test_alignments(W, pay_off, wire_off, stride):
    """70 full chunks and a 17-byte tail at every combination of payload offset, wire offset
    and stride: only (0, 0, stride % 16 == 0) is fused, every other one takes the three-step
    path with byte-odd, 4-B and 8-B aligned sources and destinations.  A path choice that
    ignored one of the three, or a dword copy that assumed alignment, tears the slots."""
    build(W, 70 * MAXP + 17, stride=stride, pay_off=pay_off, wire_off=wire_off, seq0=stride)


@pytest.mark.parametrize("with_len", [True, False])
@pytest.mark.parametrize("stride", [16384, 16400])
def test_stride_limit(W, stride, with_len):
    """8 full chunks and a tail in slots of 16384 bytes, the last fused stride, and 16400, the
    first three-step one on aligned buffers: a limit off by one slot size, or slot addresses
    that wrap at the braid's 16-KiB reach, misplace the datagrams."""
    build(W, 8 * MAXP + 333, stride=stride, with_len=with_len, seq0=3)


@pytest.mark.parametrize("pay_off", PATHS)
def test_sequence_wrap(W, pay_off):
    """seq0 = 2^32 - 2: seqNum wraps to 0 at the third chunk on both paths, and at the tail,
    whose seq is seq0 + first on the fused path."""
    build(W, 5 * MAXP + 100, pay_off=pay_off, seq0=0xFFFFFFFE)


@pytest.mark.parametrize("tail", [1, 1455])
def test_round_trip_through_accept(W, tail):
    """builder -> a permutation of the wire slots -> wtp_accept_data_packets on a guarded
    window: the image equals the source and slot_len the chunk lengths, for last chunks of 1
    and 1455 bytes.  Both ends use the vector path for the full chunks, so a row of 16-B
    vectors dropped by either shows here."""
    nch, stride, seq0 = 41, 1472, 0xFFFFFFF0
    total = (nch - 1) * MAXP + tail
    host, want, want_wl, wire, wl = build(W, total, seq0=seq0)
    perm = np.random.default_rng(tail).permutation(nch)
    ring = wire.get().reshape(nch, stride)[perm].ravel()  # what the device built
    win = DevWindow(nch)
    ok, place, ack = win.accept(W, ring, stride, want_wl[perm], seq0)
    assert ok.all() and np.array_equal(place, perm.astype(np.uint32)) and ack == (seq0 + nch) & M.M32
    assert np.array_equal(win.img.get()[:total], host) and (win.img.get()[total:] == 0xA5).all()
    assert win.h_slot_len.tolist() == [MAXP] * (nch - 1) + [tail]
