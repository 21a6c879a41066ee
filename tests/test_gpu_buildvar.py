"""GPU tests of the mixed-length DATA builder, wtp_build_data_packets_var: every output is
compared element-wise with the sequential model (tests/buildvar_model.py).  The whole wire
buffer is pre-filled with a sentinel (0xA5) and has 64 guard bytes before and after the
ring, d_wire_len and d_crc_out hold 12345 and have guard words, and the inputs are read
back, so a byte that must stay untouched is checkable."""
import numpy as np
import pytest

import buildvar_model as M
import oracle as O
from gpu_support import W_noinit as W  # noqa: F401 (fixture)
from gpu_support import Batch, Bytes, Words, assert_bytes_equal, assert_no_data_error, capture, packed
from gpu_support import replay_each_then_together, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, SENT, WSENT, GUARD = M.MAXP, 12345, 0xA5, 64
GROUPS = 2048 * 256  # above the 1280 x 256 datagrams the capped grid takes in one pass (wtp_buildvar.hip)


def run(W, b, seq0=0, stride=1472, ring_off=0, with_len=True, with_crc=True):
    """One wtp_build_data_packets_var over batch `b` into a sentinel-filled ring at byte
    `ring_off` past a 16-B aligned address; asserts every output and every untouched byte
    against the model; returns the model's (wire, wire_len, crc)."""
    n = b.n
    wire = Bytes(fill=WSENT, size=n * stride, off=ring_off, front=GUARD, back=GUARD, guard=WSENT)
    wl, crc = Words(SENT, n), Words(SENT, n)
    W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, wire.t, stride, wl.t if with_len else None,
                             crc.t if with_crc else None)
    torch.cuda.synchronize()
    if n:
        assert W.LIB.wtp_last_kernel().decode() == "k_build_var"
    want_wire, want_wl, want_crc = M.build(b.host, b.base_bytes, b.offs, b.lens, seq0,
                                           np.full(n * stride, WSENT, dtype=np.uint8), stride)
    got = wire.get()  # nothing outside the ring
    assert_bytes_equal(got, want_wire, stride, lambda slot: f"wire slots: len {b.lens[slot]}, offset {b.offs[slot]}")
    assert np.array_equal(wl.get(), want_wl if with_len else np.full(n, SENT, np.uint32))
    assert np.array_equal(crc.get(), want_crc if with_crc else np.full(n, SENT, np.uint32))
    b.check_untouched()
    assert_no_data_error(W)
    return want_wire, want_wl, want_crc


# ---- every length, every alignment -----------------------------------------------------------
@pytest.mark.parametrize("seq0", [0, 0xFFFFFF80])
def test_every_length_packed(W, seq0):
    """1457 datagrams, every length 0 .. 1456 once, back to back: all 16 source phases."""
    b = packed(np.arange(1457))
    assert b.phases() == set(range(16))
    _, wl, _ = run(W, b, seq0=seq0)
    assert np.array_equal(wl, np.arange(1457) + 16)


ALIGN_LENS = [0, 1, 3, 4, 15, 16, 17, 95, 96, 97, 1455, 1456]


@pytest.mark.parametrize("base_off", [0, 1, 4, 5])
def test_every_source_phase(W, base_off):
    """Every source address mod 16 x the lengths around the vector and segment sizes, with
    d_base itself 0, 1, 4 and 5 bytes past an allocation; the first payload starts at
    d_base and the last ends at d_base + base_bytes (the bytewise edges)."""
    offs, lens, at = [], [], 0
    for ln in ALIGN_LENS:
        for phase in range(16):
            at += (phase - base_off - at) % 16  # allocations are 16-B aligned (checked in Batch)
            offs.append(at)
            lens.append(ln)
            at += ln
    total = at  # the last payload laid out (1456 bytes at phase 15) ends the buffer
    offs += [0, 0, total - 3, total - 1455]
    lens += [7, 1456, 3, 1455]
    b = Batch(O.synth_fill_np(total, start_byte=base_off), offs, lens, base_off)
    got = ((b.base.data_ptr() + b.offs[:192]) % 16).astype(int).reshape(12, 16)
    assert (got == np.arange(16)).all()
    run(W, b, seq0=base_off)


# ---- wire shapes --------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,ring_off", [(1472, 0), (1504, 0), (1473, 0), (1472, 1), (1472, 4), (1472, 8), (1600, 8)])
def test_wire_shapes(W, stride, ring_off):
    """The fast path (16-B aligned ring, stride % 16 == 0) and the bytewise one (any other
    stride or ring address) over a 300-datagram Zipf batch."""
    run(W, packed(O.zipf_lengths(300), salt=stride), seq0=5, stride=stride, ring_off=ring_off)


# ---- unordered and overlapping ------------------------------------------------------------------
def test_unordered_and_overlapping_payloads(W):
    lens = O.zipf_lengths(200)
    offs = M.packed_offsets(lens)
    base = O.synth_fill_np(int(lens.sum()) + 3000, start_byte=77)
    perm = np.random.default_rng(5).permutation(200)
    run(W, Batch(base, offs[perm], lens[perm]))  # a permutation
    run(W, Batch(base, np.full(130, 1001, np.uint64), np.full(130, 777, np.uint32)))  # one payload, 130 times
    k = np.arange(100, dtype=np.uint64)
    run(W, Batch(base, 13 + k * 7, (1456 - 14 * k).astype(np.uint32)))  # nested ranges around one centre
    run(W, Batch(base, 500 + k, np.full(100, 1456, np.uint32)))  # full payloads sliding by one byte


# ---- invalid entries -----------------------------------------------------------------------------
def test_invalid_entries_are_left_alone(W):
    """Invalid entries between valid ones: slots untouched, wire_len 0, crc 0, no status
    flag; base_bytes is smaller than the device buffer, so the rule is about base_bytes."""
    nb = 6000
    base = O.synth_fill_np(nb + 2000, start_byte=9)
    rng = np.random.default_rng(11)
    offs, lens, valid = [], [], []
    bad = [(0, 1457), (100, 4096), (100, 4097), (100, 0xFFFFFFFF), (nb, 1), (nb + 1, 0), (nb + 1, 1), (1 << 40, 1),
           (0xFFFFFFFFFFFFFFFF, 0), (0xFFFFFFFFFFFFFFFF, 1), (nb - 5, 6), (nb - 1455, 1456), (1 << 32, 4)]
    good = [(nb - 5, 5), (nb - 1456, 1456), (nb, 0), (0, 0), (0, 1456), (nb - 1, 1)]
    for k in range(320):  # more than one workgroup round, invalid entries in every wave
        pick = bad[k % len(bad)] if k % 3 == 1 else good[k % len(good)] if k % 3 == 2 else \
            (int(rng.integers(0, nb - 1456)), int(rng.integers(0, 1457)))
        offs.append(pick[0])
        lens.append(pick[1])
        valid.append(M.is_valid(pick[0], pick[1], nb))
    assert valid.count(False) > 100 and valid.count(True) > 200
    b = Batch(base, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), base_bytes=nb)
    for stride, ring_off in ((1472, 0), (1473, 0)):
        wire, wl, crc = run(W, b, seq0=3, stride=stride, ring_off=ring_off)
        slots = wire.reshape(320, stride)
        inv = ~np.array(valid)
        assert (slots[inv] == WSENT).all() and (wl[inv] == 0).all() and (crc[inv] == 0).all()
        assert (wl[~inv] >= 16).all()
    # only invalid entries: nothing is written but the zeros
    run(W, Batch(base, np.array([p[0] for p in bad], dtype=np.uint64), np.array([p[1] for p in bad], dtype=np.uint32),
                 base_bytes=nb))


# ---- loop edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_around_the_group_sizes(W, n):
    run(W, packed(O.zipf_lengths(n), salt=n), seq0=n)


def test_70000_short_datagrams(W):
    """70 000 datagrams of lengths 0 .. 31."""
    run(W, packed(np.arange(70000) % 32, salt=1))


def test_more_datagrams_than_the_capped_grid_takes_in_one_round(W):
    """GROUPS + 300 datagrams of lengths 0 .. 7, so every workgroup runs its grid-stride loop
    a second time or leaves it.  A batch this long is compared on the device: the first 24
    bytes of every slot with a vectorised expectation (the oracle's CRCs, big-endian header
    words, the payload bytes), the rest of every slot with the sentinel; the expectation
    itself is compared with the model over the first and last 600 datagrams."""
    n, stride = GROUPS + 300, 1472
    lens = ((np.arange(n) * 5 + (np.arange(n) >> 8)) % 8).astype(np.uint32)
    offs = M.packed_offsets(lens)
    base = O.synth_fill_np(int(lens.sum()), start_byte=4)
    seq0 = 0xFFFF0000
    crc = O.batch_var(base, offs, lens)
    head = np.full((n, 24), WSENT, dtype=np.uint8)
    hdr = np.stack([np.full(n, 2, np.uint32), (seq0 + np.arange(n, dtype=np.uint64)).astype(np.uint32), lens, crc], axis=1)
    head[:, :16] = hdr.astype(">u4").view(np.uint8).reshape(n, 16)
    for k in range(7):
        rows = np.flatnonzero(lens > k)
        head[rows, 16 + k] = base[offs[rows] + np.uint64(k)]
    for part in (slice(0, 600), slice(n - 600, n)):
        want, _, want_crc = M.build(base, base.size, offs[part], lens[part], (seq0 + part.start) & M.M32,
                                    np.full(600 * 24, WSENT, np.uint8), 24)
        assert np.array_equal(want.reshape(600, 24), head[part]) and np.array_equal(want_crc, crc[part])
    b = Batch(base, offs, lens)
    whole = Bytes(fill=WSENT, size=n * stride, front=GUARD, back=GUARD, guard=WSENT)
    wl, out = Words(SENT, n), Words(SENT, n)
    W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, whole.t, stride, wl.t, out.t)
    torch.cuda.synchronize()
    slots = whole.payload.view(n, stride)
    assert torch.equal(slots[:, :24], torch.from_numpy(head).cuda())
    assert bool((slots[:, 24:] == WSENT).all())
    whole.check_guards()
    assert np.array_equal(wl.get(), lens + 16) and np.array_equal(out.get(), crc)
    b.check_untouched()
    assert_no_data_error(W)


# ---- optional pointers ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_len,with_crc", [(False, True), (True, False), (False, False)])
def test_optional_outputs(W, with_len, with_crc):
    lens = O.zipf_lengths(100)
    lens[::7] = 2000  # invalid entries, which then nothing reports
    b = Batch(O.synth_fill_np(int(lens.sum())), M.packed_offsets(lens), lens)
    run(W, b, with_len=with_len, with_crc=with_crc)


# ---- 64-bit offsets -------------------------------------------------------------------------------
def test_offsets_above_4_gib(W):
    """Eight payloads just below, across and just above offset 2^32 of a 4 GiB + 64 KiB
    buffer.  The model sees the window [2^32 - 4096, end) with the offsets moved down; the
    low 8 KiB of the buffer hold other bytes, which a truncated offset would pick up."""
    top, tail, win = 1 << 32, 64 << 10, 4096
    big = torch.empty(top + tail + 16, dtype=torch.uint8, device="cuda")
    host = O.synth_fill_np(win + tail, start_byte=123)
    big[top - win:top + tail].copy_(torch.from_numpy(host))
    big[:8192].copy_(torch.from_numpy(O.synth_fill_np(8192, start_byte=999)))
    big[top + tail:] = 0xC3
    offs = np.array([top - 3000, top - 1456, top - 700, top - 1, top, top + 1, top + 5003, top + tail - 100], dtype=np.uint64)
    lens = np.array([1456, 1456, 1456, 5, 1456, 333, 17, 100], dtype=np.uint32)
    n, stride = 8, 1472
    whole = Bytes(fill=WSENT, size=n * stride, front=GUARD, back=GUARD, guard=WSENT)
    wl, crc, dl = Words(SENT, n), Words(SENT, n), Words(lens)
    do = torch.from_numpy(offs.view(np.int64)).cuda()
    W.build_data_packets_var(big, top + tail, do, dl.t, n, 0xFFFFFFFC, whole.t, stride, wl.t, crc.t)
    torch.cuda.synchronize()
    want, want_wl, want_crc = M.build(host, win + tail, offs - np.uint64(top - win), lens, 0xFFFFFFFC,
                                      np.full(n * stride, WSENT, np.uint8), stride)
    assert np.array_equal(whole.get(), want)
    assert np.array_equal(wl.get(), want_wl) and np.array_equal(crc.get(), want_crc) and (want_wl == lens + 16).all()
    assert_no_data_error(W)


# ---- graphs ---------------------------------------------------------------------------------------
def test_graph_replay(W):
    """One call captured with no wtp_init-dependent step (it reads no library table) and
    replayed three times into re-sentinelled outputs; then two more graphs on their own
    streams, all three replayed at once."""
    n, stride = 700, 1472

    class G:
        def __init__(self, salt):
            lens = O.zipf_lengths(n, seed=salt)
            lens[salt::50] = 1500  # a few invalid entries
            self.b = packed(lens, salt=salt)
            self.seq0 = 0xFFFFFF00 + salt
            self.wire = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
            self.wl, self.crc = Words(SENT, n), Words(SENT, n)
            self.reset()
            self.graph, self.stream = capture(self.call)
            self.want = M.build(self.b.host, self.b.base_bytes, self.b.offs, self.b.lens, self.seq0,
                                np.full(n * stride, WSENT, np.uint8), stride)

        def call(self):
            W.build_data_packets_var(self.b.base, self.b.base_bytes, self.b.o, self.b.l.t, n, self.seq0, self.wire, stride,
                                     self.wl.t, self.crc.t)

        def reset(self):
            self.wire.fill_(WSENT)
            self.wl.t.fill_(SENT)
            self.crc.t.fill_(SENT)

        def check(self):
            assert np.array_equal(self.wire.cpu().numpy(), self.want[0])
            assert np.array_equal(self.wl.get(), self.want[1]) and np.array_equal(self.crc.get(), self.want[2])

    replay_each_then_together(G(1), [()] * 3, lambda: (G(2), G(3)), [()] * 3)
    assert_no_data_error(W)


# ---- round trip --------------------------------------------------------------------------------------
def test_round_trip_through_accept_and_concat(W):
    """build_data_packets_var -> accept_data_packets with window = n: the file image holds
    every payload, d_slot_len the lengths, every verdict is ok and the cumulative ACK is seq0 +
    n; crc32_concat over d_crc_out and the lengths is the CRC of the payloads' concatenation."""
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()  # accept and concat, not the builder
    n, stride, seq0 = 2000, 1472, 0xFFFFFC00
    lens = O.zipf_lengths(n, seed=77)
    b = packed(lens, salt=3)
    wire = torch.full((n * stride,), WSENT, dtype=torch.uint8, device="cuda")
    wl, crc = Words(SENT, n), Words(SENT, n)
    W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, wire, stride, wl.t, crc.t)
    img = torch.full((n * MAXP,), 0x3C, dtype=torch.uint8, device="cuda")
    sl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    ack = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.accept_data_packets(wire, stride, wl.t, n, seq0, n, img, sl, ok, None, ack)
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_concat(crc.t, b.l.t, n, out)
    torch.cuda.synchronize()
    assert bool((ok == 1).all())
    assert np.array_equal(u32(sl), lens)
    assert int(u32(ack)[0]) == (seq0 + n) & M.M32
    rows = img.cpu().numpy().reshape(n, MAXP)
    col = np.arange(MAXP)[None, :]
    want = np.full((n, MAXP), 0x3C, dtype=np.uint8)
    mask = col < lens[:, None]
    want[mask] = b.host[:int(lens.sum())]  # packed payloads, row by row
    assert np.array_equal(rows, want)
    assert int(u32(out)[0]) == O.crc32(b.host[:int(lens.sum())])
    assert np.array_equal(wl.get(), lens + 16)
    assert_no_data_error(W)
