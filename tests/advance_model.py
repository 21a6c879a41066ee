"""Sequential models of wtp_rx_advance and wtp_tx_advance (include/wtp_crc32.h), written from
the header's semantics: one slot at a time.  The caller's arrays are never modified: copies
are returned.

It also holds the bounded-window streaming loop of the advance tests: a receiver whose whole
state is two windows' worth of slots takes a stream of any length, one round per call of
`end.round`, which tests/test_advance_model.py drives over the models and
tests/test_gpu_advance.py over the device calls, with the same seeds and so the same
decisions."""
import numpy as np

MAXP = 1456
EMPTY = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def rx_advance(img, slot_len, window, adv, img_next, slot_len_next):
    """Returns (img_next, slot_len_next) after the call; `img` / `img_next` may both be None
    (then only slot_len moves and None is returned for the image)."""
    assert (img is None) == (img_next is None)
    assert len(slot_len) >= window and len(slot_len_next) >= window
    out = None if img_next is None else np.array(img_next, dtype=np.uint8, copy=True)
    sl = np.array(slot_len_next, dtype=np.uint32, copy=True)
    a = min(int(adv), window)
    for s in range(window):
        t = s + a
        v = int(slot_len[t]) if t < window else EMPTY
        sl[s] = v
        if v <= MAXP and out is not None:
            out[s * MAXP:s * MAXP + v] = img[t * MAXP:t * MAXP + v]
    return out, sl


def rx_advance_fast(img, slot_len, window, adv, img_next, slot_len_next):
    """The same without a loop over the empty slots, for large windows."""
    out = None if img_next is None else np.array(img_next, dtype=np.uint8, copy=True)
    sl = np.array(slot_len_next, dtype=np.uint32, copy=True)
    a = min(int(adv), window)
    sl[:window - a] = slot_len[a:window]
    sl[window - a:window] = EMPTY
    if out is not None:
        for s in np.flatnonzero(sl[:window] <= MAXP).tolist():
            v, t = int(sl[s]), s + a
            out[s * MAXP:s * MAXP + v] = img[t * MAXP:t * MAXP + v]
    return out, sl


def tx_advance(acked, sent_ms, slots, adv, fill_ms, acked_next, sent_ms_next):
    """Returns (acked_next, sent_ms_next) after the call."""
    assert min(len(acked), len(sent_ms), len(acked_next), len(sent_ms_next)) >= slots
    ak = np.array(acked_next, dtype=np.uint32, copy=True)
    sm = np.array(sent_ms_next, dtype=np.uint32, copy=True)
    a = min(int(adv), slots)
    for s in range(slots):
        t = s + a
        ak[s] = acked[t] if t < slots else 0
        sm[s] = sent_ms[t] if t < slots else fill_ms & M32
    return ak, sm


def tx_advance_fast(acked, sent_ms, slots, adv, fill_ms, acked_next, sent_ms_next):
    """The same without a loop, for windows of 2^20 entries."""
    ak = np.array(acked_next, dtype=np.uint32, copy=True)
    sm = np.array(sent_ms_next, dtype=np.uint32, copy=True)
    a = min(int(adv), slots)
    ak[:slots - a], ak[slots - a:slots] = acked[a:slots], 0
    sm[:slots - a], sm[slots - a:slots] = sent_ms[a:slots], fill_ms & M32
    return ak, sm


# ---- the bounded-window streaming loop --------------------------------------------------------
# 2000 packed records through a receiver of 256 slots: each round the sender offers the
# datagrams of [base, base + 256) that have not been delivered, through a seeded permutation
# with 5 % loss.  Slots that arrived behind a hole stay in the window and are offered again
# (accept drops the duplicates), so a round delivers up to the first slot that is still
# missing: the base stalls when slot `base` is lost again (one round in twenty) and otherwise
# moves by tens to hundreds of slots.  The loop is deterministic for a seed: with the one
# below it takes 19 rounds, two of which deliver nothing; tests/test_advance_model.py runs it
# on the models and holds it to STREAM_MAX_ROUNDS, twice that, which the device loop then
# inherits (it makes the same draws, so it takes the same 19).
STREAM_RECORDS, STREAM_SEQ0, STREAM_WINDOW, STREAM_LOSS, STREAM_SEED = 2000, 0xFFFFFC00, 256, 0.05, 0xAD7
STREAM_MAX_ROUNDS = 40


def stream_rounds(end, n=STREAM_RECORDS, window=STREAM_WINDOW, loss=STREAM_LOSS, seed=STREAM_SEED,
                  max_rounds=STREAM_MAX_ROUNDS):
    """Drives `end.round(idx, base, stream_off)` until n records are delivered: idx = the
    record numbers that arrive this round, in arrival order; it returns deliver's counts (k,
    run, P_k, P_run) after accept -> ACKs -> deliver -> advance and the swap of the two
    window states.  Returns the list of every round's counts; raises at max_rounds."""
    rng = np.random.default_rng(seed)
    base = off = 0
    rounds = []
    while base < n:
        if len(rounds) == max_rounds:
            raise AssertionError(f"stream not delivered after {max_rounds} rounds (base {base} of {n})")
        offered = np.arange(base, min(base + window, n))
        keep = rng.random(offered.size) >= loss
        idx = offered[rng.permutation(offered.size)]
        idx = idx[keep[idx - base]]
        k, run, pk, prun = (int(c) for c in end.round(idx, base, off))
        assert k == run and pk == prun  # the stream buffer holds the whole transfer
        rounds.append((k, run, pk, prun))
        base += k
        off += pk
    return rounds


class ModelStreamEnd:
    """The receiver of stream_rounds on the models: accept_model, deliver_model and rx_advance
    over two (img, slot_len) pairs of `window` slots."""

    def __init__(self, wire, wire_len, stride, seq0, window, total):
        """wire / wire_len: every record's datagram as buildvar_model.build made it."""
        self.wire, self.wl, self.stride, self.seq0, self.window = wire, wire_len, stride, seq0, window
        self.img = [np.full(window * MAXP, 0x3C, np.uint8) for _ in range(2)]
        self.sl = [np.full(window, EMPTY, np.uint32) for _ in range(2)]
        self.stream = np.full(total, 0xA5, np.uint8)
        self.offs, self.lens = [], []

    def round(self, idx, base, off):
        import accept_model
        import deliver_model
        w, st = self.window, self.stride
        ring = np.concatenate([self.wire[i * st:(i + 1) * st] for i in idx]) if idx.size else np.zeros(st, np.uint8)
        rl = self.wl[idx] if idx.size else np.zeros(0, np.uint32)
        ok, _, self.img[0], self.sl[0], _ = accept_model.accept(ring, st, rl, (self.seq0 + base) & M32, w, self.img[0],
                                                                self.sl[0])
        assert ok.all()
        self.stream, offs, lens, counts = deliver_model.deliver(self.img[0], self.sl[0], w, w, self.stream, self.stream.size,
                                                                off, np.zeros(w, np.uint64), np.zeros(w, np.uint32))
        k = int(counts[0])
        self.offs += offs[:k].tolist()
        self.lens += lens[:k].tolist()
        self.img[1], self.sl[1] = rx_advance(self.img[0], self.sl[0], w, k, self.img[1], self.sl[1])
        self.img.reverse()
        self.sl.reverse()
        return counts
