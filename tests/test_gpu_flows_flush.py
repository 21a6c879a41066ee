"""GPU tests of the multi-connection flush and slide, wtp_rx_deliver_flows and
wtp_rx_advance_flows: every output of both calls is compared with tests/flows_flush_model.py,
whose two calls are deliver_model.deliver and advance_model.rx_advance per flow, and for one
flow with the single-connection calls on the device.

The sentinel rule of every case: the whole stream buffer holds sentinels, and so do the guards
around it and the regions behind every output array; the image sits between two pages of
sentinel; all inputs are read back unchanged (the states of 2^20 slots by a sum); every
output is compared element-wise against the model.

Section 11 puts every length 0 .. 1456 once through k_dflows_copy (five flows, four phases of
the first delivered byte, an aligned and an unaligned image, a capacity cut inside a full-size
record) and through k_rx_advance_flows (with EMPTY slots and the non-length values, a different
advance per flow, four image pre-fills); the state is tests/flows_cases.py's."""
import numpy as np
import pytest

import flows_cases as C
import flows_flush_model as M
import flows_model as F
import oracle as O
from gpu_support import W, W_noinit  # noqa: F401 (fixtures: W for verify's tables; the graph test takes W_noinit)
from gpu_support import Bytes, Words, assert_bytes_equal, assert_no_data_error, capture, datagram_ring, dev_s32, s32, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, STRIDE, EMPTY, M32 = F.MAXP, F.STRIDE, F.EMPTY, F.M32
PAGE, SENT64, SENT32 = 4096, 0x1122334455667788, 12345
CLAIM = 0x80000005
MODES = [F.SELECTIVE, F.CUMULATIVE]


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class State:
    """A window state of nflows * window slots on the device and its host copy: the image at byte
    `img_off` past a 16-B aligned address between two pages of sentinel, slot_len with guard words."""

    def __init__(self, nflows, window, img, sl, img_off=0):
        self.nflows, self.window, self.slots = nflows, window, nflows * window
        self.h_img, self.h_sl = np.ascontiguousarray(img, dtype=np.uint8), np.ascontiguousarray(sl, dtype=np.uint32)
        assert self.h_img.size == self.slots * MAXP and self.h_sl.size == self.slots
        self.img = Bytes(self.h_img, off=img_off, front=PAGE, back=PAGE)
        self.sl = Words(self.h_sl)

    def check_untouched(self):
        assert np.array_equal(self.img.get(), self.h_img) and np.array_equal(self.sl.get(), self.h_sl)


def random_state(rng, nflows, window, lens, runs, img_off=0, behind=0.4, ends=(EMPTY, 1457, CLAIM)):
    """A State whose flow f has a leading run of runs[f] slots with lengths drawn from `lens` (an
    array that is cycled through), a value of `ends` behind it, and filled slots behind that."""
    slots = nflows * window
    sl = np.full(slots, EMPTY, np.uint32)
    it = 0
    for f in range(nflows):
        r = int(runs[f])
        sl[f * window:f * window + r] = np.take(lens, np.arange(it, it + r), mode="wrap")
        it += r
        if r < window:
            sl[f * window + r] = ends[f % len(ends)]
            tail = np.arange(f * window + r + 1, (f + 1) * window)
            keep = tail[rng.random(tail.size) < behind]
            sl[keep] = np.take(lens, np.arange(it, it + keep.size), mode="wrap")
            it += keep.size
    return State(nflows, window, rng.integers(0, 256, slots * MAXP, dtype=np.uint8), sl, img_off=img_off)


def deliver(W, st, max_slots, cap, off, phase=0, records=True, info=True, work_off=16, tail=40):
    """One wtp_rx_deliver_flows on the device and in the model: stream_bytes = cap, the buffer
    `tail` sentinel bytes longer and at byte `phase` past a 16-B boundary.  Asserts every output
    equal, everything else untouched, and returns the model's result."""
    nf, w, slots = st.nflows, st.window, st.slots
    sbuf = Bytes(fill=0xA5, size=cap + tail, off=phase, front=64, back=64, guard=0xA5)
    offs, lens = Words(77, slots + 2, dtype=np.uint64), Words(77, slots + 2)
    adv, inf, cnt = Words(SENT64, nf, dtype=np.uint64), Words(SENT64, 4 * nf, dtype=np.uint64), Words(SENT64, 4, dtype=np.uint64)
    need = W.rx_deliver_flows_work_bytes(nf, w)
    wk = torch.randint(0, 256, (need + work_off + 16,), dtype=torch.uint8, device="cuda")
    before = wk.clone()
    W.rx_deliver_flows(st.img.t, st.sl.t, nf, w, max_slots, sbuf.t, cap, off, offs.t if records else None,
                       lens.t if records else None, adv.t, inf.t if info else None, cnt.t, work=wk[work_off:work_off + need])
    torch.cuda.synchronize()
    last = "k_dflows_copy" if slots and max_slots else "k_dflows_out" if nf else "k_dflows_mid"
    assert W.LIB.wtp_last_kernel().decode() == last
    want = M.deliver_flows(st.h_img, st.h_sl, nf, w, max_slots, np.full(cap + tail, 0xA5, np.uint8), cap, off,
                           np.full(slots + 2, 77, np.uint64), np.full(slots + 2, 77, np.uint32))
    w_stream, w_offs, w_lens, w_adv, w_info, w_counts = want
    assert cnt.get().tolist() == w_counts.tolist()
    assert adv.get().tolist() == w_adv.tolist()
    assert inf.get().tolist() == (w_info.reshape(-1).tolist() if info else [SENT64] * (4 * nf))
    assert_bytes_equal(sbuf.get(), w_stream, 16, f"stream vector; off {off}, phase {phase}, counts {w_counts.tolist()}")
    assert np.array_equal(offs.get(), w_offs if records else np.full(slots + 2, 77, np.uint64))
    assert np.array_equal(lens.get(), w_lens if records else np.full(slots + 2, 77, np.uint32))
    assert torch.equal(wk[:work_off], before[:work_off]) and torch.equal(wk[work_off + need:], before[work_off + need:])
    st.check_untouched()
    assert_no_data_error(W)
    return want


def advance(W, st, advs, seq0=None, images=True, next_off=0, fill=0xEE):
    """One wtp_rx_advance_flows on the device and in the model into a sentinel-filled second
    state; asserts every output equal and every input untouched; returns the model's (image, slot_len,
    seq0) of that state."""
    nf, w, slots = st.nflows, st.window, st.slots
    h_adv = np.array(advs, dtype=np.uint64)
    adv = Words(h_adv, dtype=np.uint64)
    nimg = Bytes(fill=fill, size=slots * MAXP, off=next_off, front=PAGE, back=PAGE)
    nsl = Words(SENT32, slots)
    sq, nsq = (Words(seq0), Words(SENT32, nf)) if seq0 is not None else (None, Words(SENT32, nf))
    W.rx_advance_flows(st.img.t if images else None, st.sl.t, nf, w, adv.t, sq.t if sq else None, nimg.t if images else None,
                       nsl.t, nsq.t if sq else None)
    torch.cuda.synchronize()
    if slots:
        assert W.LIB.wtp_last_kernel().decode() == "k_rx_advance_flows"
    prior_sq = np.full(nf, SENT32, np.uint32)
    w_img, w_sl, w_sq = M.advance_flows(st.h_img if images else None, st.h_sl, nf, w, h_adv, seq0,
                                        np.full(slots * MAXP, fill, np.uint8) if images else None, np.full(slots, SENT32, np.uint32),
                                        prior_sq if seq0 is not None else None)
    assert np.array_equal(nsl.get(), w_sl)
    assert np.array_equal(nsq.get(), w_sq if seq0 is not None else prior_sq)
    got_img = nimg.get()
    if images:
        assert_bytes_equal(got_img, w_img, MAXP, lambda s: f"flow {s // max(w, 1)} slot {s % max(w, 1)}, slot_len {w_sl[s]:#x}")
    else:
        assert (got_img == fill).all()
    st.check_untouched()
    assert np.array_equal(adv.get(), h_adv) and (sq is None or np.array_equal(sq.get(), np.asarray(seq0, np.uint32)))
    assert_no_data_error(W)
    return w_img, w_sl, w_sq


# ---- 1. edges ------------------------------------------------------------------------------------
EDGE_LENS = (0, 1, 15, 16, 17, 1455, 1456)


@pytest.mark.parametrize("img_off", [0, 1, 4], ids=["vector", "bytewise", "dword"])
def test_edges(W, img_off):
    """3 flows x window 5: the run ends at slot 0 of flow 0, in the middle of flow 1 and nowhere in
    flow 2, whose seven delivered records hold every length of EDGE_LENS; at all 16 destination
    phases, from stream offsets that move with them."""
    rng = np.random.default_rng(0xED6E + img_off)
    for phase in range(16):
        lens = np.roll(EDGE_LENS, phase)
        sl = np.array([EMPTY, 5, 6, 7, 8] + [lens[0], lens[1], (1457, CLAIM, EMPTY)[phase % 3], 16, 3] + list(lens[2:]), np.uint32)
        st = State(3, 5, rng.integers(0, 256, 15 * MAXP, dtype=np.uint8), sl, img_off=img_off)
        total = int(sum(EDGE_LENS))
        off = (phase * 7) % 16 + 16 * (phase % 3)  # stream_off % 16 takes 16 values too
        want = deliver(W, st, 5, off + total + 5, off, phase=(phase * 10) % 16, work_off=(16, 1, 3)[phase % 3])
        assert want[3].tolist() == [0, 2, 5] and want[5].tolist() == [7, 7, total, total]
        if phase in (0, 7):
            advance(W, st, want[3], seq0=[0xFFFFFFFF, 7, 0xFFFFFFFC])
    # the first delivered byte's address mod 16 took every value, and so did stream_off mod 16
    assert {((p * 10) % 16 + (p * 7) % 16) % 16 for p in range(16)} == {(p * 7) % 16 for p in range(16)} == set(range(16))


# ---- 2. flow boundaries inside a vector ---------------------------------------------------------------
def test_one_vector_spans_many_flows(W):
    """40 flows x window 3 of 0- and 1-byte records, several flows empty in a row: 16 stream bytes
    come from up to 16 flows with empty ones in between."""
    rng = np.random.default_rng(40)
    runs = rng.integers(0, 4, 40)
    runs[5:9], runs[20:23], runs[39] = 0, 0, 0
    st = random_state(rng, 40, 3, np.array([1, 0, 1, 1, 0, 1, 1], np.uint32), runs)
    for off, phase in ((0, 0), (5, 3), (17, 15)):
        want = deliver(W, st, 3, 200, off, phase=phase)
        assert 16 < want[5][2] < 100 and want[5][0] == runs.sum()
    advance(W, st, want[3], seq0=np.arange(40) * 1000)


def test_a_round_of_more_records_than_the_staging(W):
    """300 flows x window 3 of 0-, 1- and 2-byte records: one 4-KiB round of the copy holds all
    of them, more than the 256 it keeps in LDS, so it reads its prefix sums from memory; a
    full-size record follows, so a second round is staged."""
    rng = np.random.default_rng(300)
    runs = rng.integers(0, 4, 300)
    runs[-1] = 3
    st = random_state(rng, 300, 3, np.array([1, 2, 0, 1, 1, 2], np.uint32), runs)
    st.h_sl[-3:] = (1456, 1456, 1456)
    st = State(300, 3, st.h_img, st.h_sl)
    want = deliver(W, st, 3, 9000, 3, phase=9)
    assert want[5][0] > 256 + 3 and 4096 < want[5][2] < 9000 - 3 and (want[2][:256] <= 2).all()


# ---- 3. windows that divide neither 64 nor 1024 --------------------------------------------------------
@pytest.mark.parametrize("nflows,window", [(7, 150), (3, 1100)])
def test_windows_that_do_not_divide_the_blocks(W, nflows, window):
    """Mixed Zipf lengths, every flow a run of its own, and an advance by a different a_f per flow:
    deliver's own d_flow_adv, and values around it."""
    rng = np.random.default_rng(nflows * window)
    runs = np.array([window, 0, 1, window - 1, 64, 65, 100]) if nflows == 7 else np.array([1025, 1100, 63])
    assert len(set(runs.tolist())) == nflows
    lens = O.zipf_lengths(4000, seed=window).astype(np.uint32)
    st = random_state(rng, nflows, window, lens, runs, behind=0.3)
    total = int(M.deliver_flows_plan(st.h_sl, nflows, window, window, 1 << 40, 0)[5][2])
    want = deliver(W, st, window, 11 + total, 11, phase=6)
    assert want[3].tolist() == runs.tolist() and want[5][2] == total
    advance(W, st, want[3], seq0=rng.integers(0, 1 << 32, nflows))
    advance(W, st, [(int(r) * 7 + f) % (window + 2) for f, r in enumerate(runs)], seq0=np.full(nflows, 0xFFFFFFFE), next_off=0)
    # a capacity cut in the middle of the second to last flow's bytes: the last flow delivers nothing
    half = int(want[4][nflows - 2][2]) - 11 + int(want[4][nflows - 2][3]) // 2
    cut = deliver(W, st, window, 11 + half, 11, phase=1)
    assert cut[5][0] < want[5][0] and cut[3][nflows - 1] == 0


# ---- 4. states compared on the device --------------------------------------------------------------------
def big_state(rng, nflows, window, full_every=9973):
    """slot_len of a large state: every flow a leading run of random length (about a third of
    them the whole window) of 0-, 1- and 2-byte records with a full slot now and then, an end
    value behind it, and one slot in four filled behind that."""
    slots = nflows * window
    runs = np.where(rng.random(nflows) < 0.35, window, rng.integers(0, window + 1, nflows))
    s = np.tile(np.arange(window), nflows)
    run_of = np.repeat(runs, window)
    sl = rng.integers(0, 3, slots).astype(np.uint32)
    sl[::full_every] = MAXP
    sl[(s > run_of) & (rng.random(slots) < 0.75)] = EMPTY
    sl[s == run_of] = np.where(rng.random(slots) < 0.5, EMPTY, 1457)[s == run_of]
    return sl, runs


def on_device(W, nflows, window, sl, max_slots, room=None, off=5, phase=3):
    """deliver_flows + advance_flows (fed with deliver's d_flow_adv as it is) on a state whose
    image is random device memory; every output is compared with the loop-free plan of the
    model, the stream and the next image on the device.  room None: what all candidates need and
    7 bytes more."""
    slots = nflows * window
    dev = "cuda"
    ibuf = torch.empty(2 * PAGE + slots * MAXP, dtype=torch.uint8, device=dev)
    ibuf[:PAGE], ibuf[PAGE + slots * MAXP:] = 0xC3, 0xC3
    img = ibuf[PAGE:PAGE + slots * MAXP]
    img.random_(0, 256)
    img_sum = int(ibuf.view(torch.int64).sum())
    d_sl = Words(sl)
    if room is None:
        room = int(M.deliver_flows_plan(sl, nflows, window, max_slots, 1 << 40, 0)[5][2]) + 7
    g, Q, ln, w_adv, w_info, w_counts = M.deliver_flows_plan(sl, nflows, window, max_slots, off + room, off)
    K, total = int(w_counts[0]), int(w_counts[2])
    cap = off + room
    sbuf = Bytes(fill=0xA5, size=cap + 40, off=phase, front=64, back=64, guard=0xA5)
    offs, lens = Words(77, slots + 2, dtype=np.uint64), Words(77, slots + 2)
    adv, inf, cnt = Words(SENT64, nflows, dtype=np.uint64), Words(SENT64, 4 * nflows, dtype=np.uint64), Words(SENT64, 4, dtype=np.uint64)
    W.rx_deliver_flows(img, d_sl.t, nflows, window, max_slots, sbuf.t, cap, off, offs.t, lens.t, adv.t, inf.t, cnt.t)
    seq0 = np.random.default_rng(slots).integers(0, 1 << 32, nflows).astype(np.uint32)
    seq0[0] = 0xFFFFFFFF
    nbuf = torch.full((2 * PAGE + slots * MAXP,), 0xEE, dtype=torch.uint8, device=dev)
    nimg = nbuf[PAGE:PAGE + slots * MAXP]
    nsl, sq, nsq = Words(SENT32, slots), Words(seq0), Words(SENT32, nflows)
    W.rx_advance_flows(img, d_sl.t, nflows, window, adv.t, sq.t, nimg, nsl.t, nsq.t)
    torch.cuda.synchronize()
    assert cnt.get().tolist() == w_counts.tolist()
    bad = np.flatnonzero(adv.get() != w_adv)
    assert bad.size == 0, (bad[:5], adv.get()[bad[:5]], w_adv[bad[:5]])
    assert np.array_equal(inf.get().reshape(nflows, 4), w_info)
    assert np.array_equal(offs.get(), np.concatenate([(Q + off).astype(np.uint64), np.full(slots + 2 - K, 77, np.uint64)]))
    assert np.array_equal(lens.get(), np.concatenate([ln, np.full(slots + 2 - K, 77, np.uint32)]))

    def gather(slot, length, first):
        """The image bytes [first, first + length) of the slots `slot`, back to back (device)."""
        length = torch.from_numpy(length.astype(np.int64)).to(dev)
        start = torch.from_numpy(slot.astype(np.int64) * MAXP).to(dev)
        ends = torch.cumsum(length, 0)
        within = torch.arange(int(ends[-1]) if length.numel() else 0, device=dev) - torch.repeat_interleave(ends - length, length)
        return torch.repeat_interleave(start, length) + within + first

    want = img[gather(g, ln, 0)]
    assert want.numel() == total and torch.equal(sbuf.payload[off:off + total], want)
    assert bool((sbuf.payload[:off] == 0xA5).all()) and bool((sbuf.payload[off + total:] == 0xA5).all())
    sbuf.check_guards()
    # the advance: lengths and bases from the model's loop-free form, the image by a gather on the device
    _, w_sl, w_sq = M.advance_flows(None, sl, nflows, window, w_adv, seq0, None, np.full(slots, SENT32, np.uint32),
                                    np.full(nflows, SENT32, np.uint32), fast=True)
    assert np.array_equal(nsl.get(), w_sl) and np.array_equal(nsq.get(), w_sq)
    moved = np.flatnonzero((w_sl <= MAXP) & (w_sl > 0))
    src = moved + np.repeat(np.minimum(w_adv.astype(np.int64), window), window)[moved]
    want_next = torch.full_like(nbuf, 0xEE)
    want_next[PAGE:PAGE + slots * MAXP][gather(moved, w_sl[moved], 0)] = img[gather(src, w_sl[moved], 0)]
    assert torch.equal(nbuf, want_next)
    # the inputs are only read
    assert int(ibuf.view(torch.int64).sum()) == img_sum and bool((ibuf[:PAGE] == 0xC3).all())
    assert np.array_equal(d_sl.get(), sl) and np.array_equal(sq.get(), seq0) and np.array_equal(adv.get(), w_adv)
    assert_no_data_error(W)
    return w_counts, w_adv, moved.size


@pytest.mark.parametrize("nflows,window", [(20_000, 3), (1, 60_000)])
def test_many_small_flows_and_one_big_flow(W, nflows, window):
    rng = np.random.default_rng(nflows)
    sl, runs = big_state(rng, nflows, window)
    if nflows == 1:
        sl[:40_000] = rng.integers(0, 3, 40_000)
        sl[:40_000:9973], sl[40_000] = MAXP, EMPTY
    counts, adv, moved = on_device(W, nflows, window, sl, max_slots=window - 1)
    assert counts[0] > 10_000 and moved > 1000 and counts[0] == adv.sum()
    # and with a capacity cut in the middle of the state
    counts2, adv2, _ = on_device(W, nflows, window, sl, max_slots=window, room=int(counts[2]) // 2, off=0, phase=0)
    assert 0 < counts2[0] < counts[0] and (nflows == 1 or (adv2 == 0).sum() > (adv == 0).sum() + nflows // 4)


# one global slot more than each level of the scan holds: a block (1024), a lane of the middle
# kernel (16 blocks), a wave of it (2^20 slots); and the issue's shape above 2^20
@pytest.mark.parametrize("nflows,window", [(1, 1025), (5, 3277), (17, 61_681), (3, 350_001)])
def test_past_each_level_of_the_scan(W, nflows, window):
    assert nflows * window in (1025, 16385, (1 << 20) + 1, 1_050_003)
    rng = np.random.default_rng(window)
    sl, runs = big_state(rng, nflows, window)
    sl[(nflows - 1) * window:] = rng.integers(0, 3, window)  # the last flow is one run up to the last slot
    sl[-1] = MAXP
    counts, adv, moved = on_device(W, nflows, window, sl, max_slots=window - window // 3)
    assert adv[-1] == window - window // 3 and moved > window // 6
    counts, adv, _ = on_device(W, nflows, window, sl, max_slots=window, off=16, phase=0)
    assert adv[-1] == window and counts[0] == counts[1] >= window


# ---- 5. cuts -------------------------------------------------------------------------------------------
LENS3 = ([10, 0, 20], [0, 30, 0, 40, 5], [7, 1456])


def test_cuts(W):
    rng = np.random.default_rng(3)
    w = 6
    sl = np.full(3 * w, EMPTY, np.uint32)
    for f, lens in enumerate(LENS3):
        sl[f * w:f * w + len(lens)] = lens
    sl[0 * w + 4], sl[2 * w + 3] = 9, 0  # behind the runs' ends
    st = State(3, w, rng.integers(0, 256, 3 * w * MAXP, dtype=np.uint8), sl)
    off = 3
    for room, advs, phase in ((60, [3, 3, 0], 0), (59, [3, 1, 0], 13), (105, [3, 5, 0], 2), (0, [0, 0, 0], 5), (5000, [3, 5, 2], 7)):
        want = deliver(W, st, w, off + room, off, phase=phase)
        assert want[3].tolist() == advs, room
        _, n_sl, _ = advance(W, st, want[3], seq0=[5, 0xFFFFFFFF, 9])
        for f in range(3):
            if advs[f] == 0:  # behind the cut the window does not move: nothing is lost
                assert np.array_equal(n_sl[f * w:(f + 1) * w], sl[f * w:(f + 1) * w])
    for m, advs in ((0, [0, 0, 0]), (1, [1, 1, 1]), (w, [3, 5, 2])):
        want = deliver(W, st, m, off + 5000, off, phase=m)
        assert want[3].tolist() == advs and want[5][1] == 10 and want[4][:, 0].tolist() == [3, 5, 2]


# ---- 6. the advance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("next_off", [0, 3], ids=["vector", "bytewise"])
def test_advance_kinds(W, next_off):
    """a_f of 0, 1, window - 1, window and 2^40 across five flows of 9 slots, 45 slots in one wave
    round; lengths with every tail (v % 16), full slots, claims and holes; bases that wrap."""
    rng = np.random.default_rng(0xAD)
    w = 9
    sl = rng.choice([0, 1, 15, 16, 17, 100, 1455, 1456, EMPTY, CLAIM, 1457], 5 * w).astype(np.uint32)
    sl[4 * w:] = MAXP
    st = State(5, w, rng.integers(0, 256, 5 * w * MAXP, dtype=np.uint8), sl)
    advs = [0, 1, w - 1, w, 1 << 40]
    seq0 = [0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC, 5]
    w_img, w_sl, w_sq = advance(W, st, advs, seq0=seq0, next_off=next_off)
    assert w_sq.tolist() == [0xFFFFFFFD, 0, 6, 5, 14] and (w_sl[3 * w:] == EMPTY).all()
    tails = [s for s in range(2 * w) if w_sl[s] < MAXP]
    assert tails and all((w_img[s * MAXP + int(w_sl[s]):(s + 1) * MAXP] == 0xEE).all() for s in tails)  # bytes [v, 1456) stay
    if next_off == 0:
        advance(W, st, advs, seq0=None)
        advance(W, st, advs, seq0=seq0, images=False)
        advance(W, st, advs, seq0=None, images=False)


def test_advance_into_a_state_that_touches(W):
    """Both states in one allocation each, the second right behind the first: ranges that touch
    are valid, and nothing of the first is written."""
    rng = np.random.default_rng(77)
    nf, w = 4, 11
    slots = nf * w
    sl = rng.choice([0, 7, 16, 333, 1456, EMPTY], slots).astype(np.uint32)
    h_img = rng.integers(0, 256, slots * MAXP, dtype=np.uint8)
    imgs = torch.cat([torch.from_numpy(h_img), torch.full((slots * MAXP,), 0xEE, dtype=torch.uint8)]).cuda()
    sls = torch.cat([torch.from_numpy(s32(sl)), torch.full((slots,), SENT32, dtype=torch.int32)]).cuda()
    seq0 = np.array([1, 2, 0xFFFFFFFF, 4], np.uint32)
    sqs = torch.cat([torch.from_numpy(s32(seq0)), torch.full((nf,), SENT32, dtype=torch.int32)]).cuda()
    advs = np.array([2, 0, 11, 5], np.uint64)
    adv = Words(advs, dtype=np.uint64)
    W.rx_advance_flows(imgs[:slots * MAXP], sls[:slots], nf, w, adv.t, sqs[:nf], imgs[slots * MAXP:], sls[slots:], sqs[nf:])
    torch.cuda.synchronize()
    w_img, w_sl, w_sq = M.advance_flows(h_img, sl, nf, w, advs, seq0, np.full(slots * MAXP, 0xEE, np.uint8),
                                        np.full(slots, SENT32, np.uint32), np.full(nf, SENT32, np.uint32))
    assert np.array_equal(imgs.cpu().numpy(), np.concatenate([h_img, w_img]))
    assert np.array_equal(u32(sls), np.concatenate([sl, w_sl])) and np.array_equal(u32(sqs), np.concatenate([seq0, w_sq]))


# ---- 7. one flow is the single-connection calls ----------------------------------------------------------
@pytest.mark.parametrize("room", [1 << 20, 9_000])
def test_single_flow_identity(W, room):
    """nflows == 1, device against device: stream, record arrays, d_counts, next image and next
    lengths are byte for byte those of wtp_rx_deliver and wtp_rx_advance."""
    rng = np.random.default_rng(room)
    w = 300
    st = random_state(rng, 1, w, O.zipf_lengths(500, seed=5).astype(np.uint32), [211], img_off=0)
    off, cap = 7, 7 + room
    size = min(cap, 7 + 300 * MAXP) + 40
    out = []
    for flows_call in (False, True):
        sbuf = Bytes(fill=0xA5, size=size, off=5, front=64, back=64, guard=0xA5)
        offs, lens, cnt = Words(77, w + 2, dtype=np.uint64), Words(77, w + 2), Words(SENT64, 4, dtype=np.uint64)
        adv = Words(SENT64, 1, dtype=np.uint64)
        nimg, nsl = Bytes(fill=0xEE, size=w * MAXP, front=64, back=64), Words(SENT32, w)
        if flows_call:
            W.rx_deliver_flows(st.img.t, st.sl.t, 1, w, w, sbuf.t, cap, off, offs.t, lens.t, adv.t, None, cnt.t)
            W.rx_advance_flows(st.img.t, st.sl.t, 1, w, adv.t, None, nimg.t, nsl.t, None)
        else:
            W.rx_deliver(st.img.t, st.sl.t, w, w, sbuf.t, cap, off, offs.t, lens.t, cnt.t)
            W.rx_advance(st.img.t, st.sl.t, w, cnt.t, nimg.t, nsl.t)
        torch.cuda.synchronize()
        out.append((sbuf.get().copy(), offs.get(), lens.get(), cnt.get(), nimg.get().copy(), nsl.get()))
        if flows_call:
            assert adv.get()[0] == cnt.get()[0]
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    k, run = int(out[0][3][0]), int(out[0][3][1])
    assert run == 211 and (k == 211 if room > 100_000 else 0 < k < 211)
    st.check_untouched()
    assert_no_data_error(W)


# ---- 8. degenerate shapes ----------------------------------------------------------------------------------
def test_degenerate_shapes(W):
    rng = np.random.default_rng(8)
    none = State(0, 6, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    want = deliver(W, none, 6, 100, 10)
    assert want[5].tolist() == [0, 0, 0, 0]
    advance(W, none, [], seq0=[])
    flat = State(4, 0, np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    want = deliver(W, flat, 3, 100, 100, work_off=1)
    assert want[5].tolist() == [0, 0, 0, 0] and want[3].tolist() == [0] * 4 and want[4][:, 2].tolist() == [100] * 4
    advance(W, flat, [1, 2, 3, 4], seq0=[1, 2, 3, 4])  # no slots: nothing is written, the bases included
    # the optional outputs left out, a 1-B aligned d_work, max_slots == 0 (the runs are still reported)
    st = random_state(rng, 3, 7, np.array([5, 0, 1456, 33], np.uint32), [7, 0, 4])
    deliver(W, st, 7, 30_000, 1, records=False, info=False, work_off=1)
    want = deliver(W, st, 0, 30_000, 1, work_off=1)
    assert want[5][0] == 0 and want[5][1] == 11 and want[5][3] > 0
    want = deliver(W, st, 7, 500, 500)  # stream_off == stream_bytes: the empty record at rank 1 does not pass the first
    assert want[5][0] == 0


# ---- 9. one graph for every round ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_graph_replay(W_noinit, mode):
    """Two consecutive rounds (accept_flows -> acks_flows -> deliver_flows -> advance_flows from
    state A to B, then the same from B to A) captured once with no wtp_init before it and
    replayed twice with the batches rewritten on the device.  The host writes d_seq0 once, before
    the first replay; every round equals the model's."""
    W = W_noinit
    nf, w, n = 3, 40, 200
    slots, cap = nf * w, nf * w * MAXP
    rng = np.random.default_rng(0xF1A5 + mode)
    z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
    img = [torch.full((slots * MAXP,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sl, seq0 = [z(slots) for _ in range(2)], [z(nf) for _ in range(2)]

    class Round:
        def __init__(self):
            self.ring, self.rl, self.flow = z(n * STRIDE, torch.uint8), z(n), z(n)
            self.ok, self.place, self.ack = z(n, torch.uint8), z(n), z(nf)
            self.wire, self.src, self.acnt = z(n * 16, torch.uint8), z(n), z(2)
            self.awork = z(W.rx_ack_flows_work_bytes(n), torch.uint8)
            self.stream = Bytes(fill=0xA5, size=cap, front=64, back=64, guard=0xA5)
            self.offs, self.lens = z(slots, torch.int64), z(slots)
            self.adv, self.info, self.dcnt = z(nf, torch.int64), z(4 * nf, torch.int64), z(4, torch.int64)
            self.dwork = z(W.rx_deliver_flows_work_bytes(nf, w), torch.uint8)

        def load(self, base):
            flow = rng.integers(0, nf + 1, n).astype(np.uint32)  # nf: no connection
            d = []
            for i in range(n):
                ln = int(rng.choice([0, 5, 16, 100, 1456]))
                g = bytearray(O.build_datagram((int(base[min(flow[i], nf - 1)]) + int(rng.integers(-3, w // 2))) & M32,
                                               rng.integers(0, 256, ln, dtype=np.uint8).tobytes()))
                if rng.random() < 0.1:
                    g[12] ^= 0x80
                d.append(bytes(g))
            self.h_ring, self.h_rl = datagram_ring(d, STRIDE)
            self.h_flow = flow
            self.ring.copy_(torch.from_numpy(self.h_ring))
            self.rl.copy_(dev_s32(self.h_rl))
            self.flow.copy_(dev_s32(flow))
            for t, v in ((self.ok, 7), (self.place, SENT32), (self.ack, SENT32), (self.wire, 0xA5), (self.src, SENT32),
                         (self.acnt, 0x77777777), (self.stream.payload, 0xA5), (self.offs, 77), (self.lens, 77), (self.adv, 99),
                         (self.info, 99), (self.dcnt, 99)):
                t.fill_(v)
            self.awork.random_(0, 256)
            self.dwork.random_(0, 256)

    rounds = [Round(), Round()]

    def call():
        for B, (a, b) in zip(rounds, ((0, 1), (1, 0))):
            W.accept_data_packets_flows(B.ring, STRIDE, B.rl, B.flow, n, seq0[a], nf, w, img[a], sl[a], B.ok, B.place, B.ack)
            W.rx_build_acks_flows(B.ring, STRIDE, B.rl, B.flow, n, mode, seq0[a], nf, w, B.ok, B.ack, B.wire, 16, 0, n, B.src,
                                  B.acnt, work=B.awork)
            W.rx_deliver_flows(img[a], sl[a], nf, w, w, B.stream.t, cap, 0, B.offs, B.lens, B.adv, B.info, B.dcnt, work=B.dwork)
            W.rx_advance_flows(img[a], sl[a], nf, w, B.adv, seq0[a], img[b], sl[b], seq0[b])

    h_seq0 = [np.array([0xFFFFFFF0, 7, 7], np.uint32), np.zeros(nf, np.uint32)]
    for B in rounds:
        B.load(h_seq0[0])
    for t in sl:
        t.fill_(-1)
    graph, stream = capture(call)
    # the state the rounds start from: what the capture's own runs left is dropped, and d_seq0 is written for the only time
    h_img = [np.full(slots * MAXP, 0xA5, np.uint8) for _ in range(2)]
    h_sl = [np.full(slots, EMPTY, np.uint32) for _ in range(2)]
    for x in range(2):
        img[x].fill_(0xA5)
        sl[x].fill_(-1)
        seq0[x].copy_(dev_s32(h_seq0[x]))
    delivered = 0
    for rep in range(2):
        # the model first: the second round's batch is made for the bases the first one leaves
        want = []
        for B, (a, b) in zip(rounds, ((0, 1), (1, 0))):
            B.load(h_seq0[a])
            w_ok, w_place, h_img[a], h_sl[a], w_ack = F.accept_flows(B.h_ring, STRIDE, B.h_rl, B.h_flow, h_seq0[a], nf, w, h_img[a],
                                                                     h_sl[a])
            acks = F.build_acks_flows(B.h_ring, STRIDE, B.h_rl, B.h_flow, mode, h_seq0[a], nf, w, w_ok, w_ack)
            dl = M.deliver_flows(h_img[a], h_sl[a], nf, w, w, np.full(cap, 0xA5, np.uint8), cap, 0, np.full(slots, 77, np.uint64),
                                 np.full(slots, 77, np.uint32))
            h_img[b], h_sl[b], h_seq0[b] = M.advance_flows(h_img[a], h_sl[a], nf, w, dl[3], h_seq0[a], h_img[b], h_sl[b], h_seq0[b])
            want.append((w_ok, w_place, w_ack, acks, dl, h_seq0[b].copy()))
            assert ((w_ack.astype(np.int64) - h_seq0[a]) & M32).tolist() == dl[3].tolist()  # deliver's runs are accept's ACKs
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for B, (w_ok, w_place, w_ack, (seq, idx, (e, total)), dl, w_seq0), (a, b) in zip(rounds, want, ((0, 1), (1, 0))):
            assert np.array_equal(B.ok.cpu().numpy(), w_ok) and np.array_equal(u32(B.place), w_place)
            assert np.array_equal(u32(B.ack), w_ack)
            assert tuple(u32(B.acnt)) == (e, total) and e > n // 3
            rows = B.wire.view(n, 16).cpu().numpy()
            assert np.array_equal(rows[:e], F.A.ack_bytes(seq)) and (rows[e:] == 0xA5).all()
            assert np.array_equal(u32(B.src), np.concatenate([idx, np.full(n - e, SENT32, np.uint32)]))
            w_stream, w_offs, w_lens, w_adv, w_info, w_counts = dl
            assert u64(B.dcnt).tolist() == w_counts.tolist() and u64(B.adv).tolist() == w_adv.tolist()
            assert u64(B.info).tolist() == w_info.reshape(-1).tolist()
            assert_bytes_equal(B.stream.get(), w_stream, 16, f"replay {rep}")
            assert np.array_equal(u64(B.offs), w_offs) and np.array_equal(u32(B.lens), w_lens)
            delivered += int(w_counts[0])
        # both states and the bases as the second round left them
        for x in range(2):
            assert np.array_equal(u32(sl[x]), h_sl[x]) and np.array_equal(u32(seq0[x]), h_seq0[x])
            assert_bytes_equal(img[x].cpu().numpy(), h_img[x], MAXP, f"replay {rep}, state {x}")
    assert delivered > 40 and (h_seq0[0] != np.array([0xFFFFFFF0, 7, 7], np.uint32)).any()
    assert_no_data_error(W)


# ---- 10. four connections through one receiver ------------------------------------------------------------
def _flows_end():
    import test_gpu_flows  # the setup of test_transfer_of_four_connections, reused as it is
    return test_gpu_flows.DevFlowsEnd


def make_flush_end(W):
    class DevFlushEnd(_flows_end()):
        """DevFlowsEnd with the flush of a round in one wtp_rx_deliver_flows + wtp_rx_advance_flows:
        all flows' records go to one round stream, the ranges (B_f, bytes_f) of d_flow_info are
        appended to the flows' files on the device, and the bases live in two device arrays that
        only the advance writes after the start."""

        def __init__(self, W):
            super().__init__(W)
            nf, w = self.nflows, self.window
            self.bases = [dev_s32([self.seq(f, 0) for f in range(nf)]), torch.zeros(nf, dtype=torch.int32, device="cuda")]
            self.cap = nf * w * MAXP
            self.rstream = Bytes(fill=0xA5, size=self.cap, front=64, back=64, guard=0xA5)
            self.roffs = torch.zeros(nf * w, dtype=torch.int64, device="cuda")
            self.rlens = torch.zeros(nf * w, dtype=torch.int32, device="cuda")
            self.fadv = torch.zeros(nf, dtype=torch.int64, device="cuda")
            self.finfo = torch.zeros(4 * nf, dtype=torch.int64, device="cuda")
            self.fwork = torch.empty(W.rx_deliver_flows_work_bytes(nf, w), dtype=torch.uint8, device="cuda")
            self.round = None

        def receive(self, gidx, flow, rbase, mode):
            W, w, nf, n = self.W, self.window, self.nflows, gidx.size
            pick = torch.from_numpy(gidx).cuda()
            self.ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
            ring = self.wire[pick].contiguous() if n else self.ok  # n == 0: any pointer
            rl = self.wl[pick].contiguous() if n else self.counts
            d_flow = dev_s32(flow) if n else self.counts
            self.ack_ring = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device="cuda")
            src = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
            W.accept_data_packets_flows(ring, STRIDE, rl, d_flow, n, self.bases[0], nf, w, self.img[0], self.sl[0], self.ok, None,
                                        self.ack)
            W.rx_build_acks_flows(ring, STRIDE, rl, d_flow, n, mode, self.bases[0], nf, w, self.ok, self.ack, self.ack_ring, 16, 0,
                                  n, src, self.counts)
            torch.cuda.synchronize()
            assert u32(self.bases[0]).tolist() == [self.seq(f, rbase[f]) for f in range(nf)]  # moved on the device alone
            e, total = (int(c) for c in u32(self.counts))
            assert bool(self.ok[:n].all()) and e == total == n
            return u32(self.ack), u32(src[:e])

        def flush(self, f, off):
            W, w, nf = self.W, self.window, self.nflows
            if self.round is None:
                W.rx_deliver_flows(self.img[0], self.sl[0], nf, w, w, self.rstream.t, self.cap, 0, self.roffs, self.rlens,
                                   self.fadv, self.finfo, self.dcounts, work=self.fwork)
                W.rx_advance_flows(self.img[0], self.sl[0], nf, w, self.fadv, self.bases[0], self.img[1], self.sl[1],
                                   self.bases[1])
                torch.cuda.synchronize()
                k, run, pk, prun = (int(c) for c in u64(self.dcounts))
                assert k == run and pk == prun  # the round stream holds every run
                self.round = (u64(self.fadv).tolist(), u64(self.finfo).reshape(nf, 4).tolist(), u64(self.roffs[:k]),
                              u32(self.rlens[:k]))
                self.rstream.check_guards()
            adv, info, offs, lens = self.round
            k, (run, R, B, nbytes) = adv[f], info[f]
            self.file[f].payload[off:off + nbytes] = self.rstream.payload[B:B + nbytes]
            self.offs[f] += (offs[R:R + k].astype(np.int64) - B + off).tolist()  # rebased to the flow's own file
            self.lens[f] += lens[R:R + k].tolist()
            return k, nbytes

        def flushed(self):
            super().flushed()
            self.bases.reverse()
            self.round = None

    return DevFlushEnd(W)


@pytest.mark.parametrize("mode", MODES)
def test_transfer_of_four_connections(W, mode):
    """test_gpu_flows' transfer with one deliver_flows + advance_flows per round and the bases
    advanced on the device: every round is the model loop's, and the byte ranges of every round,
    appended per flow, are the sources' bytes, with exact offsets, lengths and CRC."""
    want, stats = F.transfer(F.ModelEnd(), mode)
    assert (stats >= 1).all()
    end = make_flush_end(W)
    got, _ = F.transfer(end, mode)
    assert got == want and len(got) <= F.XFER_MAX_ROUNDS
    for f in range(F.XFER_FLOWS):
        lens, offs, total, host = end.rec[f]
        assert np.array_equal(end.file[f].get(), host)  # between 64 guard bytes on both sides
        assert np.array_equal(np.array(end.offs[f], np.uint64), offs) and np.array_equal(np.array(end.lens[f], np.uint32), lens)
        crc = torch.zeros(1, dtype=torch.int32, device="cuda")
        W.crc32_buffer(end.file[f].t, total, crc)
        assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)


# ---- 11. every length through the copies -------------------------------------------------------------------
# k_dflows_copy and k_rx_advance_flows are this unit's own copies of the single-window bodies:
# the counterparts of test_gpu_deliver.py::test_every_length_once and
# test_gpu_advance.py::test_every_length_once.  The state is flows_cases.flush_state's, whose
# properties tests/test_flows_cases.py asserts on the CPU.
FIRST_BYTE = ((0, 0), (5, 0), (3, 7), (17, 14))  # (stream_off, the buffer's phase): first bytes at 0, 5, 10, 15 mod 16


@pytest.mark.parametrize("img_off", [0, 1], ids=["vector", "bytewise"])
def test_every_length_once(W, img_off):
    """5 flows x window 300 whose leading runs of 300, 290, 280, 300 and 287 slots together hold
    every length 0 .. 1456 once, permuted: at four phases of the first delivered byte, with
    stream_off mod 16 moving as well; then with stream_bytes ending inside the full-size record
    in the middle of flow 2's run, so flows 3 and 4 deliver nothing."""
    img, sl, runs = C.flush_state(img_off)
    nf, w = C.FLUSH_FLOWS, C.FLUSH_WINDOW
    st = State(nf, w, img, sl, img_off=img_off)
    total = MAXP * (MAXP + 1) // 2
    assert {(off + phase) % 16 for off, phase in FIRST_BYTE} == {0, 5, 10, 15} and len({off % 16 for off, _ in FIRST_BYTE}) == 4
    for off, phase in FIRST_BYTE:
        want = deliver(W, st, w, off + total + 5, off, phase=phase)
        assert want[3].tolist() == runs.tolist() and want[5].tolist() == [MAXP + 1, MAXP + 1, total, total]
        assert sorted(want[2][:MAXP + 1].tolist()) == list(range(MAXP + 1))
    at = 2 * w + int(runs[2]) // 2
    before = int(want[1][int(want[4][2][1]) + int(runs[2]) // 2]) - FIRST_BYTE[-1][0]  # the bytes in front of that record
    assert sl[at] == MAXP
    cut = deliver(W, st, w, 9 + before + 700, 9, phase=2)
    assert cut[3].tolist() == [runs[0], runs[1], runs[2] // 2, 0, 0] and int(cut[5][2]) == before


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x3C, 0xA5])
def test_advance_every_length_once(W, fill):
    """The same state: every length once, 40 EMPTY slots, 1457, a claim pattern and 0xFFFFFFFE,
    moved by 0, the window, 2^40, 5 and 290 in the five flows into an image that holds `fill`: a
    copy one byte too long shows as a changed tail byte at one of the four pre-fills.  The next
    image is 16-B aligned for the even fills and one byte off for the odd ones."""
    img, sl, runs = C.flush_state(fill)
    nf, w = C.FLUSH_FLOWS, C.FLUSH_WINDOW
    st = State(nf, w, img, sl)
    advs = [0, w, 1 << 40, 5, 290]
    w_img, w_sl, w_sq = advance(W, st, advs, seq0=[M32 - 2, 7, M32, 0xFFFFFFFC, 9], fill=fill, next_off=fill & 1)
    assert w_sq.tolist() == [M32 - 2, 7 + w, w - 1, 1, 299]
    assert np.array_equal(w_sl[:w], sl[:w]) and (w_sl[w:3 * w] == EMPTY).all() and np.array_equal(w_sl[3 * w:4 * w - 5], sl[3 * w + 5:4 * w])
    short = np.flatnonzero(w_sl < MAXP)
    assert short.size > 500 and all((w_img[s * MAXP + int(w_sl[s]):(s + 1) * MAXP] == fill).all() for s in short.tolist())
