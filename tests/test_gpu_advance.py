"""GPU tests of the window slides, wtp_rx_advance and wtp_tx_advance: every output is compared
element-wise with the sequential models (tests/advance_model.py).  Both images sit in
allocations between two pages of sentinel (0xC3), the destination image is pre-filled with a
second sentinel, d_slot_len_next holds 12345 and has guard words behind it, and every input is
read back, so a byte that must stay untouched is checkable."""
import numpy as np
import pytest

import ack_model as A
import advance_model as M
import oracle as O
import retx_model as R
from gpu_support import W_noinit as W  # noqa: F401 (fixture)
from gpu_support import Bytes, DevBoundedEnd, DevStreamEnd, Words, assert_bytes_equal, assert_no_data_error, capture
from gpu_support import dev_s32, replay_each_then_together, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, EMPTY, SENT, EDGE, PAGE, STRIDE = M.MAXP, M.EMPTY, 12345, 0xC3, 4096, R.STRIDE
# wtp_advance.hip: a wave of k_rx_advance takes 64 destination slots per round, four of them at
# a time (one per 16-lane group), a workgroup has four waves, and the capped grid of 2048
# workgroups takes 2^19 slots per pass
WAVE_SLOTS, STEP_SLOTS, GROUP_SLOTS, PASS_SLOTS = 64, 4, 256, 2048 * 256
A_VALUES = [0, 1, 63, 64, 65, "w-1", "w", "w+1", 1 << 32, (1 << 64) - 1]


def _a(a, window):
    return {"w-1": window - 1, "w": window, "w+1": window + 1}.get(a, a)


def Img(host, off=0, flush=False):
    """An image of `host` bytes on the device, `off` bytes past a page of sentinel at a 16-B
    aligned address, another page behind it; flush: the image ends with its allocation."""
    return Bytes(host, off=off, front=PAGE, back=PAGE, guard=EDGE, flush=flush)


def mixed_lens(n, seed=0):
    """Zipf lengths with empty, full and zero-length slots and EMPTY ones sprinkled in."""
    rng = np.random.default_rng(seed)
    lens = O.zipf_lengths(n, seed=seed + 1).astype(np.uint32)
    kind = rng.random(n)
    lens[kind < 0.25] = EMPTY
    lens[(kind >= 0.25) & (kind < 0.32)] = MAXP
    lens[(kind >= 0.32) & (kind < 0.37)] = 0
    return lens


def run(W, lens, a, salt=0, fill=0x3C, src_off=0, dst_off=0, flush=False, window=None):
    """One wtp_rx_advance of a window whose d_slot_len is `lens` (every slot holds synthetic
    bytes, also behind its length) by `a`; asserts both outputs against the model, every
    untouched byte and every input; returns the model's slot_len_next."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    window = lens.size if window is None else window
    src = Img(O.synth_fill_np(max(lens.size, 1) * MAXP, start_byte=salt)[:lens.size * MAXP], src_off, flush)
    dst = Img(np.full(lens.size * MAXP, fill, np.uint8), dst_off, flush)
    sl, nsl, adv = Words(lens), Words(SENT, lens.size), Words([a], dtype=np.uint64)
    W.rx_advance(src.t, sl.t, window, adv.t, dst.t, nsl.t)
    torch.cuda.synchronize()
    if window:
        assert W.LIB.wtp_last_kernel().decode() == "k_rx_advance"
    want_img, want_sl = M.rx_advance(src.host, lens, window, a, dst.host, np.full(lens.size, SENT, np.uint32))
    assert np.array_equal(nsl.get(), want_sl)
    assert_bytes_equal(dst.get(), want_img, MAXP, f"image slots: window {window}, a {a}, offsets {src_off}, {dst_off}")
    assert np.array_equal(src.get(), src.host) and np.array_equal(sl.get(), lens) and adv.get().tolist() == [a]
    assert_no_data_error(W)
    return want_sl


# ---- 1. every length once ------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x3C, 0xA5])
def test_every_length_once(W, fill):
    """Every length 0 .. 1456 once, in a seeded order, 40 EMPTY slots among them, moved by 5: a
    copy that is one byte too long shows as a changed tail byte at one of the four pre-fills."""
    rng = np.random.default_rng(fill)
    lens = np.concatenate([np.arange(MAXP + 1), np.full(40, EMPTY)]).astype(np.uint32)[rng.permutation(MAXP + 1 + 40)]
    want = run(W, lens, 5, salt=fill, fill=fill)
    assert np.array_equal(want[:-5], lens[5:]) and (want[-5:] == EMPTY).all()


# ---- 2. values of a ------------------------------------------------------------------------------
@pytest.mark.parametrize("a", A_VALUES)
def test_values_of_a(W, a):
    a = _a(a, 130)
    want = run(W, mixed_lens(130, seed=2), a, salt=7)
    assert (want[max(130 - a, 0):] == EMPTY).all()


# ---- 3. window sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_window_sizes_around_the_group_sizes(W, window):
    run(W, mixed_lens(window, seed=window), window // 3, salt=window)


def test_window_size_zero(W):
    """Launches nothing: both outputs stay as they were, with and without pointers."""
    run(W, mixed_lens(10), 3, window=0)
    assert W.LIB.wtp_rx_advance(None, None, 0, None, None, None, None) == 0


# ---- 4. carried values ---------------------------------------------------------------------------
def test_carried_values_land_unchanged(W):
    """EMPTY, 1457, a claim pattern and 0xFFFFFFFE are stored as they are and their destination
    slots stay byte for byte (run compares the whole image with the model, which copies
    nothing for them)."""
    lens = mixed_lens(200, seed=4)
    lens[[3, 64, 65, 66, 130, 199]] = [1457, EMPTY, 0x80000005, 0xFFFFFFFE, 1457, 0x80000005]
    want = run(W, lens, 2, salt=4)
    assert want[[1, 62, 63, 64, 128, 197]].tolist() == [1457, EMPTY, 0x80000005, 0xFFFFFFFE, 1457, 0x80000005]
    lens = np.array([EMPTY, 1457, 0x80000005, 0xFFFFFFFE] * 40, dtype=np.uint32)  # nothing to copy at all
    run(W, lens, 1)


# ---- 5. alignment --------------------------------------------------------------------------------
@pytest.mark.parametrize("src_off,dst_off", [(0, 0), (1, 0), (0, 4), (8, 8), (1, 1)])
def test_image_alignments(W, src_off, dst_off):
    """Only (0, 0) takes 16-B vectors; every other pair moves bytewise, exactly.  Full first and
    last slots, between the sentinel pages and flush against the end of the allocation."""
    lens = np.concatenate([[MAXP, MAXP], mixed_lens(150, seed=5), [MAXP, 1455, MAXP]]).astype(np.uint32)
    for flush in (False, True):
        run(W, lens, 0, salt=src_off, src_off=src_off, dst_off=dst_off, flush=flush)  # the last slot stays the last
        run(W, lens, 2, salt=dst_off, src_off=src_off, dst_off=dst_off, flush=flush)


def test_images_and_states_that_touch(W):
    """The second image starts at the byte after the first one's last, and so do the states."""
    w = 70
    lens = mixed_lens(w, seed=6)
    host = O.synth_fill_np(w * MAXP, start_byte=6)
    both = torch.full((2 * w * MAXP,), 0x3C, dtype=torch.uint8, device="cuda")
    both[:w * MAXP].copy_(torch.from_numpy(host))
    sls = dev_s32(np.concatenate([lens, np.full(w, SENT, np.uint32)]))
    adv = Words([9], dtype=np.uint64)
    W.rx_advance(both, sls, w, adv.t, both[w * MAXP:], sls[w:])
    torch.cuda.synchronize()
    want_img, want_sl = M.rx_advance(host, lens, w, 9, np.full(w * MAXP, 0x3C, np.uint8), np.full(w, SENT, np.uint32))
    got, gsl = both.cpu().numpy(), u32(sls)
    assert np.array_equal(got[:w * MAXP], host) and np.array_equal(got[w * MAXP:], want_img)
    assert np.array_equal(gsl[:w], lens) and np.array_equal(gsl[w:], want_sl)


# ---- 6. state only -------------------------------------------------------------------------------
def test_state_only_at_the_largest_window(W):
    """Both images NULL: only d_slot_len moves, any contents."""
    w, a = W.RX_MAX_WINDOW, 300001
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
    valid = rng.random(w) < 0.3
    lens[valid] = rng.integers(0, MAXP + 1, int(valid.sum()))  # valid lengths too
    sl, nsl, adv = Words(lens), Words(SENT, w), Words([a], dtype=np.uint64)
    W.rx_advance(None, sl.t, w, adv.t, None, nsl.t)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == "k_rx_advance"
    _, want = M.rx_advance_fast(None, lens, w, a, None, np.full(w, SENT, np.uint32))
    assert np.array_equal(nsl.get(), want) and np.array_equal(sl.get(), lens)
    assert (want[w - a:] == EMPTY).all() and np.array_equal(want[:w - a], lens[a:])


# ---- 7. more rounds than workgroups, and than the capped grid takes in one pass --------------------
def device_expect(src, lens, a, window, fill):
    """The destination image after the call, computed on the device without a loop."""
    am = min(a, window)
    v = np.full(window, EMPTY, np.int64)
    v[:window - am] = lens[am:window]
    vt = torch.from_numpy(np.where(v <= MAXP, v, 0)).cuda()
    shifted = torch.full((window, MAXP), fill, dtype=torch.uint8, device="cuda")
    shifted[:window - am] = src.view(window, MAXP)[am:]
    mask = torch.arange(MAXP, device="cuda")[None, :] < vt[:, None]
    return shifted.masked_fill_(~mask, fill).view(-1), v.astype(np.uint32)


def big(W, lens, a, fill=0x3C, seed=0xB16):
    """A window too large to compare on the host: the images are made and compared on the
    device (torch.equal), the states and a sample of slots on the host."""
    w = lens.size
    src = torch.full((PAGE + w * MAXP + PAGE,), EDGE, dtype=torch.uint8, device="cuda")
    W.synth_fill(src[PAGE:PAGE + w * MAXP], seed=seed)
    before = src.clone()
    dst = torch.full((PAGE + w * MAXP + PAGE,), EDGE, dtype=torch.uint8, device="cuda")
    dst[PAGE:PAGE + w * MAXP] = fill
    sl, nsl, adv = Words(lens), Words(SENT, w), Words([a], dtype=np.uint64)
    W.rx_advance(src[PAGE:], sl.t, w, adv.t, dst[PAGE:], nsl.t)
    torch.cuda.synchronize()
    want, want_sl = device_expect(src[PAGE:PAGE + w * MAXP], lens, a, w, fill)
    assert np.array_equal(nsl.get(), want_sl) and np.array_equal(sl.get(), lens)
    assert torch.equal(dst[PAGE:PAGE + w * MAXP], want)
    assert bool((dst[:PAGE] == EDGE).all()) and bool((dst[PAGE + w * MAXP:] == EDGE).all()) and torch.equal(src, before)
    rows_s, rows_d = src[PAGE:PAGE + w * MAXP].view(w, MAXP), dst[PAGE:PAGE + w * MAXP].view(w, MAXP)
    for s in np.random.default_rng(seed).integers(0, w - a, 50).tolist() + [0, w - a - 1, w - 1]:
        got, v = rows_d[s].cpu().numpy(), int(want_sl[s])
        v = v if v <= MAXP else 0
        assert np.array_equal(got[:v], rows_s[min(s + a, w - 1)].cpu().numpy()[:v]) and (got[v:] == fill).all(), s
    assert_no_data_error(W)


def test_70000_zipf_slots(W):
    """Every slot filled, moved by one: 1094 rounds over 274 workgroups."""
    assert (70000 + WAVE_SLOTS - 1) // WAVE_SLOTS == 1094 and (70000 + GROUP_SLOTS - 1) // GROUP_SLOTS == 274
    big(W, O.zipf_lengths(70000).astype(np.uint32), 1)


def test_more_slots_than_the_capped_grid_takes_in_one_pass(W):
    """2^19 + 3 rounds + 1 slots, one in a hundred filled, a full one at each end: waves run
    their grid-stride loop a second time or leave it."""
    w = PASS_SLOTS + 3 * WAVE_SLOTS + 1
    rng = np.random.default_rng(19)
    lens = np.where(rng.random(w) < 0.01, O.zipf_lengths(w, seed=19), EMPTY).astype(np.uint32)
    lens[[1, PASS_SLOTS - 1, PASS_SLOTS, PASS_SLOTS + 1, w - 1]] = MAXP
    big(W, lens, 1)


# ---- 8. graphs -------------------------------------------------------------------------------------
def test_graph_replay(W):
    """One call captured with no wtp_init before it (it reads no library table) and replayed at
    three values of *d_adv written on the device between the replays: the advance is not
    baked into the graph.  Then three graphs over three windows on three streams at once."""
    n = 1500

    class G:
        def __init__(self, salt):
            self.lens = mixed_lens(n, seed=salt)
            self.src = Img(O.synth_fill_np(n * MAXP, start_byte=salt))
            self.dst = Img(np.full(n * MAXP, 0x3C, np.uint8))
            self.sl, self.nsl, self.adv = Words(self.lens), Words(SENT, n), Words([salt], dtype=np.uint64)
            self.graph, self.stream = capture(self.call)

        def call(self):
            W.rx_advance(self.src.t, self.sl.t, n, self.adv.t, self.dst.t, self.nsl.t)

        def reset(self, a):
            self.a = a
            self.adv.t.fill_(a)
            self.dst.t[:n * MAXP].fill_(0x3C)
            self.nsl.t.fill_(SENT)

        def check(self):
            want_img, want_sl = M.rx_advance(self.src.host, self.lens, n, self.a, self.dst.host, np.full(n, SENT, np.uint32))
            assert np.array_equal(self.nsl.get(), want_sl) and np.array_equal(self.dst.get(), want_img)
            assert np.array_equal(self.src.get(), self.src.host) and np.array_equal(self.sl.get(), self.lens)
            assert self.adv.get().tolist() == [self.a]

    replay_each_then_together(G(1), [(0,), (7,), (n,)], lambda: (G(2), G(3)), [(11,), (600,), (1499,)])
    assert_no_data_error(W)


# ---- 9. bounded-window streaming round trip ------------------------------------------------------
def test_bounded_window_streaming_round_trip(W):
    """2000 packed Zipf records whose sequence numbers wrap, through 5 % loss and a receiver of
    two 256-slot window states: the delivered stream, offsets and lengths are the sender's,
    its CRC the oracle's, and every round's counts the model loop's."""
    import buildvar_model as B
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()  # accept's verify and the CRC call, not the slides
    n, seq0, window, stride = M.STREAM_RECORDS, M.STREAM_SEQ0, M.STREAM_WINDOW, STRIDE
    lens = O.zipf_lengths(n, seed=77)
    lens[5:9] = [0, 1456, 0, 1]
    offs = B.packed_offsets(lens)
    total = int(lens.sum())
    host = O.synth_fill_np(total, start_byte=3)
    # the model loop: the builder's model gives its datagrams
    m_wire, m_wl, _ = B.build(host, total, offs, lens, seq0, np.zeros(n * stride, np.uint8), stride)
    want = M.stream_rounds(M.ModelStreamEnd(m_wire, m_wl, stride, seq0, window, total))
    # the device loop: the builder gives them
    wire = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    wl = dev_s32(np.zeros(n))
    W.build_data_packets_var(torch.from_numpy(host).cuda(), total, torch.from_numpy(offs.view(np.int64)).cuda(),
                             dev_s32(lens), n, seq0, wire, stride, wl, None)
    end = DevStreamEnd(W, wire, wl, n, stride, seq0, window, total)
    got = M.stream_rounds(end)
    assert got == want and len(got) <= M.STREAM_MAX_ROUNDS
    assert np.array_equal(end.whole.get(), host)  # between 64 guard bytes of 0xA5 on both sides
    assert np.array_equal(np.array(end.offs, np.uint64), offs) and np.array_equal(np.array(end.lens, np.uint32), lens)
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(end.whole.t, total, crc)
    assert int(u32(crc)[0]) == O.crc32(host)
    assert all(t.numel() == window * MAXP for t in end.img) and all(t.numel() == window for t in end.sl)
    assert_no_data_error(W)


# ---- 10. the sender's slide ------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 64, 65, 1024, 1025, 1 << 20])
def test_tx_advance(W, slots):
    assert slots <= W.TX_MAX_INFLIGHT
    rng = np.random.default_rng(slots)
    acked = (rng.random(slots) < 0.6).astype(np.uint32) * rng.integers(1, 3, slots).astype(np.uint32)
    sent = rng.integers(0, 1 << 32, slots, dtype=np.uint64).astype(np.uint32)
    da, ds = Words(acked), Words(sent)
    fill = 0xFFFFFFF3  # a clock about to wrap
    for a in sorted(set(min(_a(x, slots), M.M32) for x in A_VALUES)):
        na, ns, adv = Words(SENT, slots), Words(SENT, slots), Words([a])
        W.tx_advance(da.t, ds.t, slots, adv.t, fill, na.t, ns.t)
        torch.cuda.synchronize()
        assert W.LIB.wtp_last_kernel().decode() == "k_tx_advance"
        model = M.tx_advance if slots <= 1025 else M.tx_advance_fast
        want_a, want_s = model(acked, sent, slots, a, fill, np.full(slots, SENT, np.uint32), np.full(slots, SENT, np.uint32))
        assert np.array_equal(na.get(), want_a) and np.array_equal(ns.get(), want_s), (slots, a)
        assert np.array_equal(da.get(), acked) and np.array_equal(ds.get(), sent) and adv.get().tolist() == [a]
    assert W.LIB.wtp_tx_advance(None, None, 0, None, 0, None, None, None) == 0  # no slots: nothing launched


@pytest.mark.parametrize("mode,seq_base", [(A.SELECTIVE, 0), (A.SELECTIVE, 0xFFFFFF80), (A.CUMULATIVE, 0),
                                           (A.CUMULATIVE, 0xFFFFFF80)])
def test_end_to_end_transfer_in_two_windows_of_state(W, mode, seq_base):
    """The transfer of tests/test_gpu_ack.py with both windows bounded and slid on the device:
    the same rounds and retransmit sets as the model's endpoints, whose state is sized by the
    transfer; an exact file and whole-file CRC at the receiver."""
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    nchunks, window = R.E2E_CHUNKS, R.E2E_WINDOW
    total = nchunks * MAXP - R.E2E_SHORT
    host = O.synth_fill_np(total, seed=R.E2E_SEED)
    want_rounds, want_sets = A.transfer(A.ModelEnd(host, nchunks, window, seq_base), nchunks, window, seq_base, mode,
                                        R.E2E_SEED, R.E2E_LOSS)
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=R.E2E_SEED)
    end = DevBoundedEnd(W, src, total, nchunks, window, seq_base)
    rounds, sets = A.transfer(end, nchunks, window, seq_base, mode, R.E2E_SEED, R.E2E_LOSS)
    assert rounds == want_rounds and sets == want_sets
    assert end.off == total and torch.equal(end.file[:total], src) and bool((end.file[total:] == 0xA5).all())
    assert all(t.numel() == window for t in end.acked + end.sent + end.slot_len)
    crc = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(end.file, total, crc)
    assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)
