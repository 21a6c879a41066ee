"""GPU tests of the in-order flush, wtp_rx_deliver: every output is compared element-wise
with the sequential model (tests/deliver_model.py).  The whole stream buffer is pre-filled
with a sentinel (0xA5) and has 64 guard bytes before and after it, d_offsets_out,
d_lengths_out and d_counts hold 12345 and have guard words, the image sits between two
pages of sentinel, and the inputs are read back, so a byte that must stay untouched is
checkable."""
import numpy as np
import pytest

import deliver_model as M
import oracle as O
from gpu_support import W_noinit as W  # noqa: F401 (fixture)
from gpu_support import Bytes, Words, assert_bytes_equal, assert_no_data_error, capture, dev_s32, replay_each_then_together
from gpu_support import u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, EMPTY, SENT, WSENT, GUARD, PAGE = M.MAXP, M.EMPTY, 12345, 0xA5, 64, 4096
# wtp_deliver.hip: a wave of k_deliver_copy takes 256 vectors (4 KiB) per round, a workgroup
# four of them, and the capped grid of 2048 workgroups 32 MiB of the stream per pass; a wave
# keeps up to 256 prefix sums of a round in LDS
WAVE_BYTES, GROUP_BYTES, PASS_BYTES, STAGED = 4096, 16384, 2048 * 16384, 256


class Win:
    """The device copy of a window: the image at byte `img_off` past a page of sentinel in its
    allocation (another page after it), and slot_len."""

    def __init__(self, img, slot_len, img_off=0):
        self.host = np.ascontiguousarray(img, dtype=np.uint8)
        self.sl_host = np.ascontiguousarray(slot_len, dtype=np.uint32)
        self.window = self.sl_host.size
        assert self.host.size == self.window * MAXP
        self.mem = Bytes(self.host, off=img_off, front=PAGE, back=PAGE)  # the pages hold 0xC3
        self.img = self.mem.t
        self.sl = Words(self.sl_host)

    def check_untouched(self):
        assert np.array_equal(self.mem.get(), self.host)
        assert np.array_equal(self.sl.get(), self.sl_host)


def window_of(lens, salt=0, img_off=0):
    """A window whose every slot holds synthetic bytes (also behind the stored length) and
    whose d_slot_len is `lens` (values above 1456 included as they are)."""
    lens = np.asarray(lens, dtype=np.uint32)
    return Win(O.synth_fill_np(max(lens.size, 1) * MAXP, start_byte=salt)[:lens.size * MAXP], lens, img_off)


def run(W, w, max_slots=None, cap=None, off=0, phase=0, with_offs=True, with_lens=True, work_off=0, window=None):
    """One wtp_rx_deliver of window `w` into a sentinel-filled stream buffer of `cap` bytes
    (default: what the whole run needs past `off`) that starts `phase` bytes past a 16-B
    aligned address; asserts every output and every untouched byte against the model;
    returns (counts, stream) of the model."""
    window = w.window if window is None else window
    max_slots = window if max_slots is None else max_slots
    valid = w.sl_host[:window].astype(np.int64)
    if cap is None:
        cap = off + int(valid[valid <= MAXP].sum())
    stream = Bytes(fill=WSENT, size=cap, off=phase, front=GUARD, back=GUARD, guard=WSENT)
    offs, lens, counts = Words(SENT, window, np.uint64), Words(SENT, window), Words(SENT, 4, np.uint64)
    need = W.rx_deliver_work_bytes(window)
    work = torch.full((work_off + need,), 0xEE, dtype=torch.uint8, device="cuda")[work_off:]  # arbitrary contents
    W.rx_deliver(w.img, w.sl.t, window, max_slots, stream.t, cap, off, offs.t if with_offs else None,
                 lens.t if with_lens else None, counts.t, work=work)
    torch.cuda.synchronize()
    copied = window > 0 and max_slots > 0
    assert W.LIB.wtp_last_kernel().decode() == ("k_deliver_copy" if copied else "k_deliver_scan")
    want, want_offs, want_lens, want_counts = M.deliver(w.host, w.sl_host, window, max_slots, np.full(cap, WSENT, np.uint8),
                                                        cap, off, np.full(window, SENT, np.uint64),
                                                        np.full(window, SENT, np.uint32))
    assert counts.get().tolist() == want_counts.tolist()
    got = stream.get()  # nothing outside the buffer
    assert_bytes_equal(got, want, 1, f"stream bytes: off {off}, phase {phase}, delivered {int(want_counts[2])} bytes of "
                                     f"{int(want_counts[0])} records")
    assert np.array_equal(offs.get(), want_offs if with_offs else np.full(window, SENT, np.uint64))
    assert np.array_equal(lens.get(), want_lens if with_lens else np.full(window, SENT, np.uint32))
    w.check_untouched()
    assert_no_data_error(W)
    return want_counts, want


# ---- 1. every length once ----------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1, 7, 15])
def test_every_length_once(W, off):
    """1457 slots, every length 0 .. 1456 once, at four phases of the first delivered byte."""
    counts, _ = run(W, window_of(np.arange(1457), salt=off), off=off)
    assert counts.tolist() == [1457, 1457, 1456 * 1457 // 2, 1456 * 1457 // 2]


# ---- 2. boundary vectors -----------------------------------------------------------------------
EDGE_LENS = [0, 1, 2, 3, 15, 16, 17, 31, 63, 64, 65, 1455, 1456]


@pytest.mark.parametrize("phase", range(16))
def test_boundary_vectors(W, phase):
    """Lengths around the vector size in random order, with runs of 25 one-byte and 25 empty
    records (one destination vector spans more than two records; an empty record sits at a
    vector's edge), for each of the 16 destination phases, given half by the buffer's address
    and half by stream_off."""
    rng = np.random.default_rng(phase)
    lens = rng.choice(EDGE_LENS, 120).tolist()
    lens[30:30] = [1] * 25 + [16] + [0] * 25 + [1] * 7 + [0] * 3 + [15]
    lens[100:100] = [0] * 21 + [1] * 21
    lens = [16 - phase if phase else 16] + lens + [1456, 0]  # the second record starts on a vector's edge
    run(W, window_of(lens, salt=phase), off=phase // 2, phase=phase - phase // 2)
    run(W, window_of(lens[::-1], salt=phase + 100), off=32 + phase, phase=0)


# ---- 3. run endings ------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [EMPTY, 1457, 0x80000005])
def test_run_ends_in_the_middle(W, bad):
    """Slots after the end hold valid lengths and are not delivered."""
    lens = O.zipf_lengths(1500, seed=3)
    lens[1100] = bad
    counts, _ = run(W, window_of(lens, salt=1), off=3)  # room for every valid length, also behind the end
    assert counts[0] == counts[1] == 1100


def test_run_ends_at_slot_0_and_nowhere(W):
    lens = O.zipf_lengths(300, seed=4)
    counts, _ = run(W, window_of(lens), off=9)
    assert counts[0] == counts[1] == 300
    lens[0] = EMPTY
    counts, stream = run(W, window_of(lens), off=9, cap=5000)
    assert counts.tolist() == [0, 0, 0, 0] and (stream == WSENT).all()


# ---- 4. cuts ---------------------------------------------------------------------------------------
def test_max_slots_cuts(W):
    lens = O.zipf_lengths(1300, seed=5)
    lens[1200] = EMPTY
    w = window_of(lens, salt=2)
    for m in (0, 1, 1199, 1200, 1205):
        counts, _ = run(W, w, max_slots=m, off=5, cap=5 + int(lens[:1200].sum()))
        assert counts[0] == min(m, 1200) and counts[1] == 1200


def test_capacity_cuts(W):
    """stream_bytes exactly at a record boundary in the middle of a scan block, and one byte
    less; stream_off == stream_bytes; empty records at the cut."""
    lens = O.zipf_lengths(2500, seed=6)
    lens[1498:1503] = [0, 0, 40, 0, 0]  # P_1501 is the boundary: records 1501, 1502 are empty and fit too
    w = window_of(lens, salt=3)
    at = int(lens[:1501].sum())
    counts, _ = run(W, w, off=11, cap=11 + at)
    assert counts.tolist()[:3] == [1503, 2500, at]
    counts, _ = run(W, w, off=11, cap=11 + at - 1)
    assert counts.tolist()[:3] == [1500, 2500, at - 40]  # the empty records before the 40-byte one still fit
    counts, stream = run(W, w, off=77, cap=77)
    assert counts.tolist() == [0, 2500, 0, int(lens.sum())] and (stream == WSENT).all()
    w0 = window_of([0, 0, 0, 5, 0], salt=4)
    assert run(W, w0, off=8, cap=8)[0].tolist() == [3, 5, 0, 5]
    assert run(W, w0, off=0, cap=0)[0].tolist() == [3, 5, 0, 5]
    assert run(W, w0, max_slots=2)[0].tolist() == [2, 5, 0, 5]


# ---- 5. window sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_window_sizes_around_the_group_sizes(W, n):
    run(W, window_of(O.zipf_lengths(n, seed=n), salt=n), off=n % 16)
    run(W, window_of(np.full(n, 1456), salt=n), off=1)  # full slots, none empty behind them


def test_stream_sizes_around_the_copy_kernels_groups(W):
    """Delivered byte counts one below, at and above a vector, a wave's and a workgroup's round."""
    for total in (15, 16, 17, WAVE_BYTES - 1, WAVE_BYTES, WAVE_BYTES + 1, GROUP_BYTES - 1, GROUP_BYTES, GROUP_BYTES + 1):
        lens = [1456] * (total // 1456) + [total % 1456]
        for off in (0, 5):
            assert run(W, window_of(lens, salt=total), off=off)[0][2] == total


def test_window_size_zero(W):
    w = window_of(O.zipf_lengths(10))
    assert run(W, w, window=0, cap=100, off=7)[0].tolist() == [0, 0, 0, 0]
    whole = Words(SENT, 4, np.uint64)
    work = torch.empty(W.rx_deliver_work_bytes(0), dtype=torch.uint8, device="cuda")
    W.rx_deliver(None, None, 0, 5, None, 0, 0, None, None, whole.t, work=work)  # no pointer but d_counts and d_work
    torch.cuda.synchronize()
    assert whole.get().tolist() == [0, 0, 0, 0] and W.LIB.wtp_last_kernel().decode() == "k_deliver_scan"


def test_70000_zipf_slots(W):
    """More than one block at each scan level."""
    counts, _ = run(W, window_of(O.zipf_lengths(70000), salt=7), off=13)
    assert counts[0] == 70000


def test_more_bytes_than_the_capped_grid_takes_in_one_pass(W):
    """24 000 full slots and a Zipf tail: every wave of the copy kernel runs its grid-stride
    loop a second time or leaves it."""
    lens = np.concatenate([np.full(24000, 1456), O.zipf_lengths(500, seed=12)])
    assert 24000 * 1456 > PASS_BYTES + GROUP_BYTES
    counts, _ = run(W, window_of(lens, salt=8), off=6)
    assert counts[0] == 24500


def test_rounds_of_many_tiny_records(W):
    """More records in a wave's 4-KiB round than it keeps prefix sums for in LDS: lengths 0, 1
    and 2 by the thousand, between ordinary records, and around that limit."""
    rng = np.random.default_rng(21)
    tiny = rng.integers(0, 3, 9000)
    lens = np.concatenate([O.zipf_lengths(40, seed=13), tiny, [1456, 700], np.zeros(600), [5], np.ones(STAGED * 16),
                           O.zipf_lengths(40, seed=14)])
    run(W, window_of(lens, salt=9), off=3)
    for first in (16, 32, 48):  # then 16-byte records: the first round needs STAGED + 1, STAGED, STAGED - 1 sums
        assert (WAVE_BYTES - 1 - first) // 16 + 1 + 2 == STAGED + 2 - first // 16
        run(W, window_of([first] + [16] * 400, salt=first), off=0)


# ---- 6. the image's and the work buffer's edges ---------------------------------------------------
@pytest.mark.parametrize("img_off", [0, 1, 4])
def test_image_at_its_allocations_edges(W, img_off):
    """Full-length first and last slots of an image between two pages of sentinel; the image 1
    and 4 bytes past an aligned address (bytewise and dword paths); a 1-B aligned d_work."""
    lens = np.concatenate([[1456, 1456], O.zipf_lengths(200, seed=8), [1456, 1455, 1456]])
    for off in (0, 1, 2, 3, 9):  # every source phase mod 4 of the last slot's widened loads
        run(W, window_of(lens, salt=img_off, img_off=img_off), off=off, work_off=1)
    run(W, window_of([1456], salt=1, img_off=img_off), off=3, work_off=3)


# ---- 7. optional outputs -------------------------------------------------------------------------
@pytest.mark.parametrize("with_offs,with_lens", [(False, True), (True, False), (False, False)])
def test_optional_outputs(W, with_offs, with_lens):
    run(W, window_of(O.zipf_lengths(1100, seed=9)), off=2, with_offs=with_offs, with_lens=with_lens)


# ---- 8. graphs -------------------------------------------------------------------------------------
def test_graph_replay(W):
    """One call captured with no wtp_init before it (it reads no library table) and replayed
    three times into re-sentinelled outputs; then two more graphs on their own streams with
    their own work buffers, all three replayed at once."""
    n = 1500

    class G:
        def __init__(self, salt):
            lens = O.zipf_lengths(n, seed=salt)
            lens[n - 50 * salt] = EMPTY
            self.w = window_of(lens, salt=salt)
            self.off, self.max_slots = salt, n - 7 * salt
            self.cap = self.off + int(lens[:n - 60 * salt].sum())  # the capacity cuts before max_slots and the run do
            self.stream_buf = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
            self.offs, self.lens, self.counts = Words(SENT, n, np.uint64), Words(SENT, n), Words(SENT, 4, np.uint64)
            self.work = torch.full((W.rx_deliver_work_bytes(n),), 0xEE, dtype=torch.uint8, device="cuda")
            self.reset()
            self.graph, self.stream = capture(self.call)
            self.want = M.deliver(self.w.host, self.w.sl_host, n, self.max_slots, np.full(self.cap, WSENT, np.uint8), self.cap,
                                  self.off, np.full(n, SENT, np.uint64), np.full(n, SENT, np.uint32))
            assert 0 < self.want[3][0] < min(self.max_slots, self.want[3][1])

        def call(self):
            W.rx_deliver(self.w.img, self.w.sl.t, n, self.max_slots, self.stream_buf, self.cap, self.off, self.offs.t,
                         self.lens.t, self.counts.t, work=self.work)

        def reset(self):
            self.stream_buf.fill_(WSENT)
            self.offs.t.fill_(SENT)
            self.lens.t.fill_(SENT)
            self.counts.t.fill_(SENT)
            self.work.fill_(0x11)

        def check(self):
            assert np.array_equal(self.stream_buf.cpu().numpy(), self.want[0])
            assert np.array_equal(self.offs.get(), self.want[1]) and np.array_equal(self.lens.get(), self.want[2])
            assert self.counts.get().tolist() == self.want[3].tolist()

    for x in replay_each_then_together(G(1), [()] * 3, lambda: (G(2), G(3)), [()] * 3):
        x.w.check_untouched()
    assert_no_data_error(W)


# ---- 9, 10. round trips ---------------------------------------------------------------------------
class Sender:
    """2000 packed Zipf records built into datagrams by wtp_build_data_packets_var."""

    def __init__(self, W, n=2000, seq0=0xFFFFFC00, stride=1472):
        import buildvar_model as B
        self.n, self.seq0, self.stride = n, seq0, stride
        self.lens = O.zipf_lengths(n, seed=77)
        self.lens[5:9] = [0, 1456, 0, 1]
        self.offs = B.packed_offsets(self.lens)
        self.total = int(self.lens.sum())
        self.host = O.synth_fill_np(self.total, start_byte=3)
        self.wire = torch.full((n * stride,), WSENT, dtype=torch.uint8, device="cuda")
        self.wl, self.crc = dev_s32(np.zeros(n)), dev_s32(np.zeros(n))
        W.build_data_packets_var(torch.from_numpy(self.host).cuda(), self.total,
                                 torch.from_numpy(self.offs.view(np.int64)).cuda(), dev_s32(self.lens), n, seq0, self.wire,
                                 stride, self.wl, self.crc)

    def pick(self, idx):
        """The ring and lengths of datagrams `idx`, in that order."""
        sel = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
        return self.wire.view(self.n, self.stride)[sel].contiguous().view(-1), self.wl[sel].contiguous()


def test_round_trip_one_batch(W):
    """packed records -> build_data_packets_var -> a permutation of the datagrams ->
    accept_data_packets -> rx_deliver: the sender's stream, offsets and lengths, and the CRC
    calls apply to the delivered stream directly."""
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()  # accept and the CRC calls, not deliver
    s = Sender(W)
    n = s.n
    ring, wl = s.pick(np.random.default_rng(9).permutation(n))
    img = torch.full((n * MAXP,), 0x3C, dtype=torch.uint8, device="cuda")
    sl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    W.accept_data_packets(ring, s.stride, wl, n, s.seq0, n, img, sl, ok)
    whole = Bytes(fill=WSENT, size=s.total, front=GUARD, back=GUARD, guard=WSENT)
    offs, lens, counts = Words(SENT, n, np.uint64), Words(SENT, n), Words(SENT, 4, np.uint64)
    W.rx_deliver(img, sl, n, n, whole.t, s.total, 0, offs.t, lens.t, counts.t)
    crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    W.crc32_batch_packed(whole.t, s.total, offs.t, lens.t, n, crc)
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(whole.t, s.total, one)
    torch.cuda.synchronize()
    assert bool((ok == 1).all())
    assert counts.get().tolist() == [n, n, s.total, s.total]
    assert np.array_equal(whole.get(), s.host)
    assert np.array_equal(offs.get(), s.offs) and np.array_equal(lens.get(), s.lens)
    assert torch.equal(crc, s.crc) and np.array_equal(u32(crc), O.batch_var(s.host, s.offs, s.lens))
    assert int(u32(one)[0]) == O.crc32(s.host)
    assert_no_data_error(W)


def test_round_trip_two_rounds_with_a_loss(W):
    """Three datagrams are lost: the first deliver stops at the first hole, the host advances
    both windows by d_counts[0] and stream_off by d_counts[2], the missing datagrams arrive and
    the second deliver completes the stream."""
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    s = Sender(W)
    n, lost = s.n, [300, 301, 1500]
    first = [i for i in np.random.default_rng(10).permutation(n).tolist() if i not in lost]
    img = torch.full((n * MAXP,), 0x3C, dtype=torch.uint8, device="cuda")
    sl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    whole = Bytes(fill=WSENT, size=s.total, front=GUARD, back=GUARD, guard=WSENT)
    offs, lens = Words(SENT, n, np.uint64), Words(SENT, n)
    c1, c2 = Words(SENT, 4, np.uint64), Words(SENT, 4, np.uint64)
    ring, wl = s.pick(first)
    ok = torch.zeros(len(first), dtype=torch.uint8, device="cuda")
    W.accept_data_packets(ring, s.stride, wl, len(first), s.seq0, n, img, sl, ok)
    W.rx_deliver(img, sl, n, n, whole.t, s.total, 0, offs.t, lens.t, c1.t)
    torch.cuda.synchronize()
    k, run_, pk, prun = c1.get().tolist()
    assert bool((ok == 1).all()) and k == run_ == 300 and pk == prun == int(s.lens[:300].sum())
    got = whole.get()
    assert np.array_equal(got[:pk], s.host[:pk]) and (got[pk:] == WSENT).all()
    # the window moves by k: the image, slot_len and the metadata arrays from slot k on
    ring, wl = s.pick(lost[::-1])
    ok = torch.zeros(3, dtype=torch.uint8, device="cuda")
    W.accept_data_packets(ring, s.stride, wl, 3, s.seq0 + k, n - k, img[k * MAXP:], sl[k:], ok)
    W.rx_deliver(img[k * MAXP:], sl[k:], n - k, n - k, whole.t, s.total, pk, offs.t[k:], lens.t[k:], c2.t)
    torch.cuda.synchronize()
    assert bool((ok == 1).all()) and c2.get().tolist() == [n - k, n - k, s.total - pk, s.total - pk]
    assert np.array_equal(whole.get(), s.host)
    assert np.array_equal(offs.get(), s.offs) and np.array_equal(lens.get(), s.lens)
    assert_no_data_error(W)
