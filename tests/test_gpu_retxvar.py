"""GPU tests of wtp_tx_build_retransmit_var: every output is compared element-wise with the
sequential model (tests/retxvar_model.py).  The whole wire ring is pre-filled with a sentinel
(0xA5) and has 64 guard bytes before and after it, d_sel, d_wire_len and d_crc_out hold 12345
and have guard words, d_counts too, and every input is read back, so a byte that must stay
untouched is checkable."""
import itertools

import numpy as np
import pytest

import ack_model as A
import buildvar_model as B
import oracle as O
import retx_model as R
import retxvar_model as M
from gpu_support import W_noinit as W  # noqa: F401 (fixture)
from gpu_support import Batch, Bytes, DevStreamEnd, Words, assert_bytes_equal, assert_no_data_error, capture, dev_s32
from gpu_support import packed, replay_each_then_together, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, STRIDE, M32, SENT, WSENT, GUARD = M.MAXP, M.STRIDE, M.M32, 12345, 0xA5, 64
NOW, TIMEOUT = 10_000, 500
OLD, FRESH = NOW - TIMEOUT - 1, NOW - TIMEOUT  # a timer that is due, and one that is just not
# wtp_txvar.hip: the grid of k_tx_emit_var is one wave per ring entry, m = min(max_sel, inflight)
# of them in workgroups of four, capped at 1280 workgroups = 5120 waves; a wave round is G
# datagrams, the smallest power of two with G * waves >= the emitted count, at most 64.  A grid
# below the cap has waves >= m >= count, so G = 1 whatever the count: the counts up to 4098 below
# all run with G = 1 (more waves than datagrams for max_sel = the window).  With the
# capped grid G changes at count = 5120 * 2^j: 5120 | 5121 (1 -> 2), 10 240 | 10 241 (2 -> 4),
# 20 480 | 20 481 (4 -> 8), 40 960 | 40 961 (8 -> 16), 81 920 | 81 921 (16 -> 32), 163 840 |
# 163 841 (32 -> 64); above 64 * 5120 = 327 680 a wave takes a second round.
CAP_WAVES = 5120
THRESHOLDS = [CAP_WAVES << j for j in range(6)]


def state(n, due, rng=None):
    """(acked, sent_ms) of n slots of which the slots `due` (indices or a bool mask) are due:
    the others are ACKed (with an old timer) or un-ACKed with a timer that is just not due."""
    mask = np.zeros(n, bool)
    mask[due] = True
    rng = rng or np.random.default_rng(n)
    waiting = ~mask & (rng.random(n) < 0.3)
    acked = (~mask & ~waiting).astype(np.uint32) * rng.integers(1, 3, n).astype(np.uint32)
    sent = np.where(waiting, FRESH, OLD).astype(np.uint32)
    return acked, sent


def run(W, b, acked, sent, max_sel, seq0=0, stride=STRIDE, ring_off=0, now=NOW, timeout=TIMEOUT, flags=0, inflight=None,
        outs=(True, True, True), vectorised=True):
    """One wtp_tx_build_retransmit_var over the window whose records are batch `b` into a
    sentinel-filled ring of max_sel slots at byte `ring_off` past a 16-B aligned address;
    asserts every output, every untouched byte and every input against the model; returns the
    model's (wire, sel, wire_len, crc, sent, counts) and the state arrays after the call."""
    inflight = b.n if inflight is None else inflight
    rows = max(max_sel, 1)
    ring = Bytes(fill=WSENT, size=rows * stride, off=ring_off, front=GUARD, back=GUARD, guard=WSENT)
    d_acked, d_sent, counts = Words(acked), Words(sent), Words(SENT, 2)
    d_out = [Words(SENT, rows) if on else None for on in outs]
    work = torch.empty(W.tx_work_bytes(inflight, max_sel), dtype=torch.uint8, device="cuda")
    W.tx_build_retransmit_var(b.base, b.base_bytes, b.o, b.l.t, seq0, inflight, d_acked.t, d_sent.t, now, timeout, flags,
                              ring.t, stride, max_sel, *(w.t if w else None for w in d_out), counts.t,
                              work=work)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == ("k_tx_emit_var" if min(inflight, max_sel) else "k_tx_select")
    prior = [np.full(rows, SENT, np.uint32) if on else None for on in outs]
    want = M.retransmit_var(b.host, b.base_bytes, b.offs, b.lens, seq0, inflight, acked, sent, now, timeout, flags,
                            np.full(rows * stride, WSENT, np.uint8), stride, max_sel, *prior, vectorised=vectorised)
    assert tuple(counts.get().tolist()) == want[5], (counts.get(), want[5])
    got = ring.get()  # nothing outside the ring
    assert_bytes_equal(got, want[0], stride, f"ring entries: emitted {want[5][0]}, max_sel {max_sel}, inflight {inflight}")
    for name, w, x in zip(("sel", "wire_len", "crc_out"), d_out, want[1:4]):
        assert w is None or np.array_equal(w.get(), x), name
    assert np.array_equal(d_sent.get(), want[4]) and np.array_equal(d_acked.get(), acked)
    b.check_untouched()
    assert_no_data_error(W)
    return want, d_sent.get()


# ---- 1. every length, five due patterns, four rings --------------------------------------------------
@pytest.mark.parametrize("pattern", ["none", "one", "tenth", "half", "all"])
def test_every_length_due_patterns_and_rings(W, pattern):
    """A packed window of 1457 records, every length 0 .. 1456 once (all 16 source phases), with
    none, one, about 10 %, 50 % and all of its slots due, into rings of due, due - 1 (then the
    call again for the one left: timers were reset for the emitted slots only), due + 70 and
    inflight entries."""
    n = MAXP + 1
    b = packed(np.arange(n), salt=len(pattern))
    assert b.phases() == set(range(16))
    rng = np.random.default_rng(len(pattern))
    due = {"none": np.zeros(n, bool), "one": np.arange(n) == 777, "tenth": rng.random(n) < 0.1, "half": rng.random(n) < 0.5,
           "all": np.ones(n, bool)}[pattern]
    acked, sent = state(n, due, rng)
    d = int(due.sum())
    for max_sel in sorted({d, max(d - 1, 0), d + 70, n}):
        want, sent_after = run(W, b, acked, sent, max_sel, seq0=0xFFFFFF00)
        assert want[5] == (min(d, max_sel), d)
        if max_sel == d - 1:  # the call again: the last due slot alone
            again, _ = run(W, b, acked, sent_after, max_sel=max(d - 1, 1), seq0=0xFFFFFF00)
            assert again[5] == (1, 1) and again[1][0] == np.flatnonzero(due)[-1]


# ---- 2. emitted counts and round sizes ----------------------------------------------------------------
def _count_case(W, count, window, max_sel, rec_len):
    """`count` due slots spread over a window of `window` records of rec_len bytes each."""
    due = np.round(np.linspace(0, window - 1, count)).astype(np.int64)
    assert np.unique(due).size == count
    acked, sent = state(window, due)
    lens = np.full(window, rec_len, np.uint32)
    want, _ = run(W, packed(lens, salt=count & 0xFF), acked, sent, max_sel, seq0=0xFFFFFFF0 - count)
    assert want[5] == (count, count) and np.array_equal(want[1][:count], due)


@pytest.mark.parametrize("rec_len", [MAXP, 4])
def test_emitted_counts_1_to_70(W, rec_len):
    """Each count in a window five slots larger, with max_sel = the count and = the window."""
    for count in range(1, 71):
        for max_sel in (count, count + 5):
            _count_case(W, count, count + 5, max_sel, rec_len)


@pytest.mark.parametrize("rec_len", [MAXP, 4])
@pytest.mark.parametrize("c0", [255, 1023, 4095])
def test_emitted_counts_around_powers_of_two(W, c0, rec_len):
    for count in range(c0, c0 + 4):
        for max_sel in (count, count + 9):
            _count_case(W, count, count + 9, max_sel, rec_len)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_each_side_of_every_round_size_change(W, threshold):
    """The capped grid (see THRESHOLDS above): `threshold` datagrams run with G, one more with
    2 G.  4-byte records at every threshold; full-size ones where the ring stays below 64 MB."""
    for count in (threshold, threshold + 1):
        _count_case(W, count, count + 9, count + 9, 4)
        if threshold <= 4 * CAP_WAVES:  # both grids are capped: the ring fitted to the count, and full-size records
            _count_case(W, count, count + 9, count, 4)
            _count_case(W, count, count + 9, count + 9, MAXP)


# ---- 3. source and wire alignment ----------------------------------------------------------------------
ALIGN_LENS = [1, 3, 4, 15, 16, 17, 63, 64, 65, 1455, 1456]


@pytest.mark.parametrize("base_off", [0, 1, 4, 5])
def test_every_source_phase(W, base_off):
    """Every source address mod 16 x the lengths around the vector and piece sizes; the first
    record starts at byte 0 of d_base and the last ends at its last byte (the bytewise edges).
    Every other slot and the edge records are due."""
    offs, lens, at = [0], [7], 7
    for ln in ALIGN_LENS:
        for phase in range(16):
            at += (phase - base_off - at) % 16  # allocations are 16-B aligned (checked in Batch)
            offs.append(at)
            lens.append(ln)
            at += ln
    total = at  # the last record laid out (1456 bytes at phase 15) ends the buffer
    offs += [0, total - 3, total - 1455]
    lens += [1456, 3, 1455]
    b = Batch(O.synth_fill_np(total, start_byte=base_off), offs, lens, base_off)
    got = ((b.base.data_ptr() + b.offs[1:177]) % 16).astype(int).reshape(11, 16)
    assert (got == np.arange(16)).all()
    for part in (0, 1):
        due = np.arange(b.n) % 2 == part
        due[[0, 176, b.n - 3, b.n - 2, b.n - 1]] = True
        acked, sent = state(b.n, due)
        run(W, b, acked, sent, b.n, seq0=base_off)


@pytest.mark.parametrize("stride,ring_off", list(itertools.product([1472, 1488, 1473], [0, 4, 1])))
def test_wire_shapes(W, stride, ring_off):
    """The fast path (16-B aligned ring, stride % 16 == 0) and the bytewise one."""
    lens = O.zipf_lengths(300, seed=stride + ring_off)
    acked, sent = state(300, np.random.default_rng(stride).random(300) < 0.7)
    run(W, packed(lens, salt=stride & 0xFF), acked, sent, 300, seq0=5, stride=stride, ring_off=ring_off)


# ---- 4. records and selection ----------------------------------------------------------------------------
def test_falling_order_and_overlapping_records(W):
    lens = O.zipf_lengths(200)
    offs = B.packed_offsets(lens)
    base = O.synth_fill_np(int(lens.sum()) + 3000, start_byte=77)
    acked, sent = state(200, np.random.default_rng(2).random(200) < 0.6)
    run(W, Batch(base, offs[::-1].copy(), lens[::-1].copy()), acked, sent, 200)  # falling offsets
    k = np.arange(100, dtype=np.uint64)
    acked, sent = state(100, np.arange(100) % 3 != 1)
    run(W, Batch(base, np.full(100, 1001, np.uint64), np.full(100, 777, np.uint32)), acked, sent, 100)  # one record, 100 times
    run(W, Batch(base, 13 + k * 7, (1456 - 14 * k).astype(np.uint32)), acked, sent, 100)  # nested ranges
    run(W, Batch(base, 500 + k, np.full(100, 1456, np.uint32)), acked, sent, 100)  # full records sliding by one byte


def test_invalid_records_among_the_due_slots(W):
    """Length 1457, length 0xFFFFFFFF, an offset above base_bytes, and an offset and length that
    run past the end: selected, counted, timers reset, slots untouched, wire_len = crc_out = 0."""
    nb = 6000
    base = O.synth_fill_np(nb + 2000, start_byte=9)  # base_bytes is smaller than the device buffer
    bad = [(0, 1457), (100, 0xFFFFFFFF), (nb + 1, 0), (nb - 5, 6), (1 << 40, 1), (0xFFFFFFFFFFFFFFFF, 1), (nb - 1455, 1456)]
    good = [(nb - 5, 5), (nb - 1456, 1456), (nb, 0), (0, 0), (0, 1456), (nb - 1, 1)]
    rng = np.random.default_rng(11)
    recs = [bad[k % len(bad)] if k % 3 == 1 else good[k % len(good)] if k % 3 == 2 else
            (int(rng.integers(0, nb - 1456)), int(rng.integers(0, 1457))) for k in range(320)]
    b = Batch(base, np.array([r[0] for r in recs], np.uint64), np.array([r[1] for r in recs], np.uint32), base_bytes=nb)
    due = rng.random(320) < 0.8
    acked, sent = state(320, due)
    for stride, ring_off in ((1472, 0), (1473, 0)):
        want, sent_after = run(W, b, acked, sent, 320, seq0=3, stride=stride, ring_off=ring_off)
        e = want[5][0]
        inv = np.array([not B.is_valid(*recs[s], nb) for s in want[1][:e]])
        assert e == int(due.sum()) and inv.sum() > 60 and (sent_after[due] == NOW).all()
        slots = want[0].reshape(320, stride)[:e]
        assert (slots[inv] == WSENT).all() and (want[2][:e][inv] == 0).all() and (want[3][:e][inv] == 0).all()
        assert (want[2][:e][~inv] >= 16).all()


def test_timers_clock_wrap_and_retx_all(W):
    n = 150
    b = packed(O.zipf_lengths(n, seed=8), salt=8)
    rng = np.random.default_rng(8)
    acked = (rng.random(n) < 0.3).astype(np.uint32)
    for now in (NOW, 5, 0xFFFFFFFF):  # 5: the clock has wrapped since every send
        age = rng.integers(0, 3, n) + TIMEOUT - 1  # timeout - 1, timeout (not due), timeout + 1 (due)
        sent = ((now - age) & M32).astype(np.uint32)
        want, _ = run(W, b, acked, sent, n, now=now, vectorised=False)
        assert np.array_equal(want[1][:want[5][0]], np.flatnonzero((acked == 0) & (age == TIMEOUT + 1)))
        want, _ = run(W, b, acked, sent, n, now=now, flags=R.RETX_ALL, vectorised=False)
        assert np.array_equal(want[1][:want[5][0]], np.flatnonzero(acked == 0))


@pytest.mark.parametrize("outs", list(itertools.product([True, False], repeat=3)))
def test_optional_outputs(W, outs):
    lens = O.zipf_lengths(100)
    lens[::7] = 2000  # invalid records, which without d_wire_len nothing reports
    acked, sent = state(100, np.arange(100) % 4 != 0)
    run(W, Batch(O.synth_fill_np(int(lens.sum())), B.packed_offsets(lens), lens), acked, sent, 90, outs=outs)


def test_empty_window_and_empty_ring(W):
    """inflight == 0 and max_sel == 0 still write d_counts; wtp_last_kernel() is k_tx_select
    (asserted in run), nothing else is written."""
    b = packed(O.zipf_lengths(40))
    acked, sent = state(40, np.arange(40) % 2 == 0)
    want, sent_after = run(W, b, acked, sent, 0)
    assert want[5] == (0, 20) and np.array_equal(sent_after, sent)
    want, _ = run(W, b, acked, sent, 10, inflight=0)
    assert want[5] == (0, 0)
    want, _ = run(W, b, acked, sent, 0, inflight=0)
    assert want[5] == (0, 0)
    counts = Words(SENT, 2)
    work = torch.empty(W.tx_work_bytes(0, 0), dtype=torch.uint8, device="cuda")
    W.tx_build_retransmit_var(None, 0, None, None, 0, 0, None, None, 0, 0, 0, None, STRIDE, 0, counts=counts.t, work=work)
    torch.cuda.synchronize()
    assert counts.get().tolist() == [0, 0] and W.LIB.wtp_last_kernel().decode() == "k_tx_select"


# ---- 5. byte-identity with the existing calls ---------------------------------------------------------------
def test_all_due_equals_the_builder(W):
    n = 1000
    lens = O.zipf_lengths(n, seed=3)
    lens[::97] = 1500  # invalid: untouched in both
    b = packed(np.minimum(lens, MAXP), salt=3)
    b = Batch(b.host, b.offs, lens)
    rings = [torch.full((n * 1488,), WSENT, dtype=torch.uint8, device="cuda") for _ in range(2)]
    wl, crc = [Words(SENT, n), Words(SENT, n)], [Words(SENT, n), Words(SENT, n)]
    W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, 0xFFFFFE00, rings[0], 1488, wl[0].t, crc[0].t)
    acked, sent, counts, sel = Words(0, n), Words(7, n), Words(SENT, 2), Words(SENT, n)
    W.tx_build_retransmit_var(b.base, b.base_bytes, b.o, b.l.t, 0xFFFFFE00, n, acked.t, sent.t, 9, 0, R.RETX_ALL, rings[1], 1488,
                              n, sel.t, wl[1].t, crc[1].t, counts.t)
    torch.cuda.synchronize()
    assert torch.equal(rings[0], rings[1]) and bool((rings[0].view(n, 1488)[:, :16] != WSENT).any())
    assert np.array_equal(wl[0].get(), wl[1].get()) and np.array_equal(crc[0].get(), crc[1].get())
    assert counts.get().tolist() == [n, n] and np.array_equal(sel.get(), np.arange(n)) and (sent.get() == 9).all()


@pytest.mark.parametrize("short", [0, 100])
def test_chunked_buffer_equals_the_fixed_call(W, short):
    """A buffer cut into 1456-byte chunks (the last one `short` bytes shorter): wire, sel, timers
    and counts of wtp_tx_build_retransmit, byte for byte."""
    n = 700
    total = n * MAXP - short
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=short + 1)
    offs = np.arange(n, dtype=np.uint64) * MAXP
    lens = np.minimum(MAXP, total - offs.astype(np.int64)).astype(np.uint32)
    due = np.random.default_rng(short).random(n) < 0.4
    due[-1] = True
    acked, sent = state(n, due)
    out = []
    for var in (False, True):
        ring = torch.full((n * STRIDE,), WSENT, dtype=torch.uint8, device="cuda")
        a, s, sel, wl, counts = Words(acked), Words(sent), Words(SENT, n), Words(SENT, n), Words(SENT, 2)
        if var:
            W.tx_build_retransmit_var(src, total, torch.from_numpy(offs.view(np.int64)).cuda(), dev_s32(lens), 0xFFFFFF00, n,
                                      a.t, s.t, NOW, TIMEOUT, 0, ring, STRIDE, n, sel.t, wl.t, None, counts.t)
        else:
            W.tx_build_retransmit(src, total, 0xFFFFFF00, n, a.t, s.t, NOW, TIMEOUT, 0, ring, STRIDE, n, sel.t, wl.t, counts.t)
        torch.cuda.synchronize()
        out.append((ring, s.get(), sel.get(), wl.get(), counts.get()))
    assert torch.equal(out[0][0], out[1][0]) and out[0][4].tolist() == [int(due.sum())] * 2
    assert all(np.array_equal(x, y) for x, y in zip(out[0][1:], out[1][1:]))


# ---- 6. more datagrams than the capped grid takes in one pass ---------------------------------------------------
def test_400000_short_records_all_due(W):
    """400 000 records of at most 8 bytes, all due: G = 64 and 6250 rounds over 5120 waves, so
    waves run their loop a second time or leave it.  Compared on the device with the builder's
    ring over the same records (byte-identity), the sentinel tails, and the oracle's CRCs."""
    n = 400_000
    lens = ((np.arange(n) * 5 + (np.arange(n) >> 8)) % 9).astype(np.uint32)
    offs = B.packed_offsets(lens)
    base = O.synth_fill_np(int(lens.sum()), start_byte=4)
    b = Batch(base, offs, lens)
    seq0 = 0xFFFF0000
    want = torch.full((n * STRIDE,), WSENT, dtype=torch.uint8, device="cuda")
    W.build_data_packets_var(b.base, b.base_bytes, b.o, b.l.t, n, seq0, want, STRIDE)
    whole = Bytes(fill=WSENT, size=n * STRIDE, front=GUARD, back=GUARD, guard=WSENT)
    acked, sent, counts = Words(0, n), Words(OLD, n), Words(SENT, 2)
    sel, wl, crc = Words(SENT, n), Words(SENT, n), Words(SENT, n)
    W.tx_build_retransmit_var(b.base, b.base_bytes, b.o, b.l.t, seq0, n, acked.t, sent.t, NOW, TIMEOUT, 0, whole.t, STRIDE,
                              n, sel.t, wl.t, crc.t, counts.t)
    torch.cuda.synchronize()
    assert torch.equal(whole.payload, want)
    slots = whole.payload.view(n, STRIDE)
    assert bool((slots[:, 24:] == WSENT).all()) and bool((slots[:, 0:4] == torch.tensor([0, 0, 0, 2], device="cuda")).all())
    whole.check_guards()
    assert counts.get().tolist() == [n, n] and np.array_equal(sel.get(), np.arange(n)) and (sent.get() == NOW).all()
    assert np.array_equal(wl.get(), lens + 16) and np.array_equal(crc.get(), O.batch_var(base, offs, lens))
    head = slots[:, :16].cpu().numpy().view(">u4")  # the headers against the oracle
    assert np.array_equal(head[:, 1], (seq0 + np.arange(n)) & M32) and np.array_equal(head[:, 2], lens)
    assert np.array_equal(head[:, 3], crc.get())
    b.check_untouched()


# ---- 7. 64-bit offsets -----------------------------------------------------------------------------------------
def test_offsets_above_4_gib(W):
    """Eight records just below, across and just above offset 2^32 of a 4 GiB + 64 KiB buffer, six
    of them due.  The model sees the window [2^32 - 4096, end) with the offsets moved down; the low
    8 KiB of the buffer hold other bytes, which a truncated offset would pick up."""
    top, tail, win = 1 << 32, 64 << 10, 4096
    big = torch.empty(top + tail + 16, dtype=torch.uint8, device="cuda")
    host = O.synth_fill_np(win + tail, start_byte=123)
    big[top - win:top + tail].copy_(torch.from_numpy(host))
    big[:8192].copy_(torch.from_numpy(O.synth_fill_np(8192, start_byte=999)))
    big[top + tail:] = 0xC3
    offs = np.array([top - 3000, top - 1456, top - 700, top - 1, top, top + 1, top + 5003, top + tail - 100], dtype=np.uint64)
    lens = np.array([1456, 1456, 1456, 5, 1456, 333, 17, 100], dtype=np.uint32)
    n = 8
    acked = np.array([0, 0, 1, 0, 0, 1, 0, 0], np.uint32)
    sent = np.full(n, OLD, np.uint32)
    whole = Bytes(fill=WSENT, size=n * STRIDE, front=GUARD, back=GUARD, guard=WSENT)
    sel, wl, crc, dl, counts = Words(SENT, n), Words(SENT, n), Words(SENT, n), Words(lens), Words(SENT, 2)
    da, ds = Words(acked), Words(sent)
    do = torch.from_numpy(offs.view(np.int64)).cuda()
    W.tx_build_retransmit_var(big, top + tail, do, dl.t, 0xFFFFFFFC, n, da.t, ds.t, NOW, TIMEOUT, 0, whole.t, STRIDE, n,
                              sel.t, wl.t, crc.t, counts.t)
    torch.cuda.synchronize()
    want = M.retransmit_var(host, win + tail, offs - np.uint64(top - win), lens, 0xFFFFFFFC, n, acked, sent, NOW, TIMEOUT, 0,
                            np.full(n * STRIDE, WSENT, np.uint8), STRIDE, n, *(np.full(n, SENT, np.uint32) for _ in range(3)))
    assert np.array_equal(whole.get(), want[0])
    assert np.array_equal(sel.get(), want[1]) and np.array_equal(wl.get(), want[2]) and np.array_equal(crc.get(), want[3])
    assert np.array_equal(ds.get(), want[4]) and tuple(counts.get().tolist()) == want[5] == (6, 6)
    assert want[2][:6].tolist() == [1472, 1472, 21, 1472, 33, 116]
    assert_no_data_error(W)


# ---- 8. graphs ---------------------------------------------------------------------------------------------------
def test_graph_replay(W):
    """ingest -> retransmit_var captured once with no wtp_init before it (neither reads a library
    table) and replayed three times, the ACK ring rewritten on the device between the replays:
    with WTP_RETX_ALL every replay emits what is still un-ACKed.  Then three graphs over three
    windows on three streams at once."""
    n, nack = 600, 64

    class G:
        def __init__(self, salt):
            self.salt, self.seq0 = salt, 0xFFFFFF00 + salt
            lens = O.zipf_lengths(n, seed=salt)
            lens[salt::50] = 1500  # a few invalid records
            b = packed(np.minimum(lens, MAXP), salt=salt)
            self.b = Batch(b.host, b.offs, lens)
            self.acked, self.sent = np.zeros(n, np.uint32), np.full(n, 3, np.uint32)
            self.d_acked, self.d_sent = Words(self.acked), Words(self.sent)
            self.acks = torch.zeros((nack, 16), dtype=torch.uint8, device="cuda")
            self.rl = torch.full((nack,), 16, dtype=torch.int32, device="cuda")
            self.ok = torch.zeros(nack, dtype=torch.uint8, device="cuda")
            self.icounts, self.counts = Words(SENT, 2), Words(SENT, 2)
            self.ring = torch.empty(n * STRIDE, dtype=torch.uint8, device="cuda")
            self.sel, self.wl, self.crc = Words(SENT, n), Words(SENT, n), Words(SENT, n)
            self.work = torch.empty(W.tx_work_bytes(n, n), dtype=torch.uint8, device="cuda")
            # capture's first run outside the capture: the zeroed ring holds no ACK, and every slot is emitted,
            # so every timer becomes 77
            self.graph, self.stream = capture(self.call)
            self.sent[:] = 77

        def call(self):
            W.tx_ingest_acks(self.acks, 16, self.rl, nack, R.SELECTIVE, self.seq0, n, self.d_acked.t, self.ok, None,
                             self.icounts.t)
            W.tx_build_retransmit_var(self.b.base, self.b.base_bytes, self.b.o, self.b.l.t, self.seq0, n, self.d_acked.t,
                                      self.d_sent.t, 77, 0, R.RETX_ALL, self.ring, STRIDE, n, self.sel.t, self.wl.t,
                                      self.crc.t, self.counts.t, work=self.work)

        def reset(self, turn):
            """New ACKs, written by a device-to-device copy, and re-sentinelled outputs."""
            rng = np.random.default_rng(100 * self.salt + turn)
            self.seqs = (self.seq0 + rng.integers(-3, n + 3, nack)) & M32
            self.acks.copy_(torch.from_numpy(A.ack_bytes(self.seqs)).cuda())
            self.ring.fill_(WSENT)
            for w in (self.sel, self.wl, self.crc):
                w.t.fill_(SENT)

        def check(self):
            _, _, self.acked, (lead, newly) = R.ingest(A.ack_bytes(self.seqs).reshape(-1), 16, np.full(nack, 16, np.uint32),
                                                       R.SELECTIVE, self.seq0, n, self.acked)
            want = M.retransmit_var(self.b.host, self.b.base_bytes, self.b.offs, self.b.lens, self.seq0, n, self.acked, self.sent,
                                    77, 0, R.RETX_ALL, np.full(n * STRIDE, WSENT, np.uint8), STRIDE, n,
                                    *(np.full(n, SENT, np.uint32) for _ in range(3)))
            self.sent = want[4]
            assert self.icounts.get().tolist() == [lead, newly] and newly > 0
            assert tuple(self.counts.get().tolist()) == want[5] and np.array_equal(self.ring.cpu().numpy(), want[0])
            assert np.array_equal(self.sel.get(), want[1]) and np.array_equal(self.wl.get(), want[2])
            assert np.array_equal(self.crc.get(), want[3])
            assert np.array_equal(self.d_acked.get(), self.acked) and np.array_equal(self.d_sent.get(), self.sent)
            self.b.check_untouched()

    replay_each_then_together(G(1), [(0,), (1,), (2,)], lambda: (G(2), G(3)), [(7,)] * 3)
    assert_no_data_error(W)


# ---- 9. the sender-window stream loop ------------------------------------------------------------------------------
class DevVarEnd:
    """Both ends of retxvar_model.stream_rounds on the device.  The sender keeps two (acked,
    sent_ms) pairs of `window` entries and the record arrays, and no wire image: a round's ring
    is what wtp_tx_build_retransmit_var built from the records.  The receiver, `rx`, is
    gpu_support's DevStreamEnd over that ring: accept -> ACKs -> deliver -> rx_advance over two
    (img, slot_len) pairs.  Two synchronisations per round: one behind the sender's call, to
    read its counts and selection; one behind the receiver's calls and the sender's ingest ->
    tx_advance that follow them on the stream, to read deliver's counts and the advance (seq0
    and the record cursor are host scalars)."""

    def __init__(self, W, host, total, offs, lens, seq0, window):
        self.W, self.total, self.seq0, self.window = W, total, seq0, window
        z = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        self.base = torch.from_numpy(host).cuda()
        self.o, self.l = torch.from_numpy(offs.view(np.int64)).cuda(), dev_s32(lens)
        fill0 = int(np.array([(M.STREAM_NOW0 - M.STREAM_TIMEOUT - 1) & M32], np.uint32).view(np.int32)[0])
        self.acked, self.sent = [z(window), z(window)], [z(window, fill0), z(window, fill0)]
        self.ring = torch.full((window * STRIDE,), WSENT, dtype=torch.uint8, device="cuda")
        self.sel, self.wl, self.txc, self.adv = z(window), z(window), z(2), z(2)
        self.work = torch.empty(W.tx_work_bytes(window, window), dtype=torch.uint8, device="cuda")
        self.rx = DevStreamEnd(W, self.ring, self.wl, window, STRIDE, seq0, window, total)

    def emit(self, sbase, inflight, now, timeout):
        w = self.window
        self.W.tx_build_retransmit_var(self.base, self.total, self.o[sbase:], self.l[sbase:], (self.seq0 + sbase) & M32, inflight,
                                       self.acked[0], self.sent[0], now, timeout, 0, self.ring, STRIDE, w, self.sel, self.wl,
                                       None, self.txc, work=self.work)
        torch.cuda.synchronize()
        counts = tuple(int(c) for c in u32(self.txc))
        return u32(self.sel[:counts[0]]), counts

    def receive(self, idx, rbase, off, aidx, sbase, inflight, fill_ms):
        W, w, na = self.W, self.window, aidx.size
        aok = torch.zeros(max(na, 1), dtype=torch.uint8, device="cuda")

        def ingest_and_slide():
            pick = torch.from_numpy(aidx.astype(np.int64)).cuda()
            acks = self.rx.ack_ring[pick].contiguous() if na else aok  # na == 0: any pointer
            arl = torch.full((max(na, 1),), 16, dtype=torch.int32, device="cuda")
            W.tx_ingest_acks(acks, 16, arl, na, R.SELECTIVE, (self.seq0 + sbase) & M32, inflight, self.acked[0], aok, None,
                             self.adv)
            W.tx_advance(self.acked[0], self.sent[0], w, self.adv, fill_ms, self.acked[1], self.sent[1])
            self.acked.reverse()
            self.sent.reverse()

        counts = self.rx.round(idx, rbase, off, then=ingest_and_slide)
        assert bool(aok[:na].all())
        return tuple(int(c) for c in counts), int(u32(self.adv)[0])


def test_sender_window_stream_loop(W):
    """2000 packed Zipf records whose sequence numbers wrap, through 5 % loss of DATA and of
    ACKs, between a sender and a receiver of 256 entries of state each: every round's counts on
    both sides and every selection are the model loop's; the delivered stream, offsets and
    lengths are the sender's, its CRC the oracle's."""
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()  # accept's verify and the CRC call, not the sender's calls
    lens, offs, total, host = M.stream_records()
    want = M.stream_rounds(M.ModelEnd(host, total, offs, lens, M.STREAM_SEQ0, M.STREAM_WINDOW))
    end = DevVarEnd(W, host, total, offs, lens, M.STREAM_SEQ0, M.STREAM_WINDOW)
    got = M.stream_rounds(end)
    assert got == want and len(got) == M.STREAM_ROUNDS <= M.STREAM_MAX_ROUNDS
    assert np.array_equal(end.rx.whole.get(), host)  # between 64 guard bytes of 0xA5 on both sides
    assert np.array_equal(np.array(end.rx.offs, np.uint64), offs) and np.array_equal(np.array(end.rx.lens, np.uint32), lens)
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(end.rx.whole.t, total, crc)
    assert int(u32(crc)[0]) == O.crc32(host)
    assert all(t.numel() == M.STREAM_WINDOW for t in end.acked + end.sent + end.rx.sl)
    assert_no_data_error(W)
