"""Sequential model of wtp_tx_build_retransmit_var (include/wtp_crc32.h), written from the
header's semantics: retx_model.retransmit's selection (the window state is the fixed call's,
and the selection does not look at the records), then oracle.build_datagram per emitted entry
under buildvar_model's validity rule.  The caller's arrays are never modified: copies are
returned.

It also holds the sender-window stream loop of the retransmit tests: records of mixed length
cross two lossy channels between a sender and a receiver that each keep `window` entries of
state, with no wire image kept anywhere: what is lost is built again from the records.
tests/test_retxvar_model.py drives it over the models and tests/test_gpu_retxvar.py over the
device calls, with the same seed and so the same decisions."""
import numpy as np

import ack_model as A
import advance_model as V
import buildvar_model as B
import oracle as O
import retx_model as R

MAXP, HDR, M32 = 1456, 16, 0xFFFFFFFF
STRIDE = MAXP + HDR
RETX_ALL = R.RETX_ALL


def retransmit_var(base, base_bytes, offsets, lengths, seq0, inflight, acked, sent_ms, now_ms, timeout_ms, flags, wire,
                   wire_stride, max_sel, sel=None, wire_len=None, crc_out=None, vectorised=False):
    """Returns (wire, sel, wire_len, crc_out, sent_ms, (emitted, due)) after the call.  `wire`
    is the prior image of the ring (max_sel slots or more); `sel`, `wire_len` and `crc_out` are
    the prior contents of the optional outputs, None for a NULL pointer (None comes back).
    `offsets` / `lengths` are the window's: entry s is slot s."""
    base = np.asarray(base, dtype=np.uint8)
    assert base_bytes <= base.size
    picked, _, sent, (emitted, due) = R.retransmit(None, 0, seq0, inflight, acked, sent_ms, now_ms, timeout_ms, flags,
                                                   max_sel, build=False, vectorised=vectorised)
    wire = np.array(wire, dtype=np.uint8, copy=True)
    assert wire.size >= emitted * wire_stride
    outs = [None if a is None else np.array(a, dtype=np.uint32, copy=True) for a in (sel, wire_len, crc_out)]
    for k, s in enumerate(int(x) for x in picked):
        off, ln = int(offsets[s]), int(lengths[s])
        length = crc = 0
        if B.is_valid(off, ln, base_bytes):
            payload = base[off:off + ln].tobytes()
            d = O.build_datagram((seq0 + s) & M32, payload)
            wire[k * wire_stride:k * wire_stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
            length, crc = len(d), O.crc32(payload)
        for a, v in zip(outs, (s, length, crc)):
            if a is not None:
                a[k] = v
    return (wire, *outs, sent, (emitted, due))


# ---- the sender-window stream loop -----------------------------------------------------------
# 2000 packed Zipf records (lengths 0, 1456, 0, 1 planted) whose sequence numbers wrap, a sender
# and a receiver of 256 slots each, 5 % loss of DATA and 5 % loss of ACKs from one generator,
# selective ACKs, timeout 1 ms and a clock that advances 1 per round and wraps on the way.
# A round is, in stream order,
#   sender    wtp_tx_build_retransmit_var over the window at `sbase`: first transmissions and
#             retransmissions in one ordered selection (new slots enter the window due)
#   channel   the emitted datagrams, dropped and permuted by ring position
#   receiver  accept -> selective ACKs (one per arrival: every datagram of the sender's window is
#             inside the receiver's or below it) -> deliver -> rx_advance
#   channel   the ACKs, dropped and permuted
#   sender    ingest -> tx_advance with fill_ms = (the next round's now) - timeout - 1, so that
#             the entries behind the shifted ones are due at the next round's call
# A packet sent in round t is not due in round t + 1 (age 1 = timeout) and is due in round t + 2:
# its ACK, if it survives, is ingested before round t + 1's selection.  With the seed below the
# models take STREAM_ROUNDS rounds; the loop is held to twice that.
STREAM_RECORDS, STREAM_SEQ0, STREAM_WINDOW, STREAM_LOSS, STREAM_SEED = 2000, 0xFFFFFC00, 256, 0.05, 0x5E7D
STREAM_TIMEOUT, STREAM_NOW0 = 1, 0xFFFFFFF0
STREAM_ROUNDS = 37
STREAM_MAX_ROUNDS = 2 * STREAM_ROUNDS


def stream_records():
    """(lengths, offsets, total, host bytes) of the stream loop's records."""
    lens = O.zipf_lengths(STREAM_RECORDS, seed=77)
    lens[5:9] = [0, 1456, 0, 1]
    total = int(lens.sum())
    return lens, B.packed_offsets(lens), total, O.synth_fill_np(total, start_byte=3)


def stream_rounds(end, n=STREAM_RECORDS, window=STREAM_WINDOW, loss=STREAM_LOSS, seed=STREAM_SEED,
                  timeout=STREAM_TIMEOUT, now0=STREAM_NOW0, max_rounds=STREAM_MAX_ROUNDS):
    """Drives `end` until the sender's window has passed record n:
      end.emit(sbase, inflight, now, timeout) -> (sel, (emitted, due)): the sender's call
      end.receive(idx, rbase, off, aidx, sbase, inflight, fill_ms) -> ((k, run, P_k, P_run), adv):
        the receiver's round over ring positions idx (arrival order), then the sender's ingest of
        the ACKs aidx (positions in the receiver's ACK ring, arrival order) and its slide.
    Returns every round's (emitted, due, sel, k, run, P_k, P_run, adv); raises at max_rounds."""
    rng = np.random.default_rng(seed)
    sbase = rbase = off = 0
    now = now0
    log = []
    while sbase < n:
        if len(log) == max_rounds:
            raise AssertionError(f"stream not acknowledged after {max_rounds} rounds (sender base {sbase} of {n})")
        inflight = min(window, n - sbase)
        sel, (emitted, due) = end.emit(sbase, inflight, now, timeout)
        assert emitted == due == len(sel)  # the ring holds a whole window
        idx = rng.permutation(emitted)
        idx = idx[rng.random(emitted)[idx] >= loss]
        aidx = rng.permutation(idx.size)
        aidx = aidx[rng.random(idx.size)[aidx] >= loss]
        now = (now + 1) & M32
        (k, run, pk, prun), adv = end.receive(idx, rbase, off, aidx, sbase, inflight, (now - timeout - 1) & M32)
        assert k == run and pk == prun  # the stream buffer holds the whole transfer
        log.append((emitted, due, [int(s) for s in sel], int(k), int(run), int(pk), int(prun), int(adv)))
        rbase += int(k)
        off += int(pk)
        sbase += int(adv)
        assert sbase <= rbase
    return log


class ModelEnd:
    """Both ends on the models: retransmit_var, retx_model.ingest and advance_model.tx_advance
    over two (acked, sent_ms) pairs of `window` entries; accept_model, deliver_model and
    rx_advance over two (img, slot_len) pairs (advance_model.ModelStreamEnd)."""

    def __init__(self, host, total, offs, lens, seq0, window, now0=STREAM_NOW0, timeout=STREAM_TIMEOUT):
        self.host, self.total, self.offs, self.lens, self.seq0, self.window = host, total, offs, lens, seq0, window
        self.acked = [np.zeros(window, np.uint32) for _ in range(2)]
        self.sent = [np.full(window, (now0 - timeout - 1) & M32, np.uint32) for _ in range(2)]  # all due at once
        self.rx = V.ModelStreamEnd(None, None, STRIDE, seq0, window, total)

    def emit(self, sbase, inflight, now, timeout):
        w = self.window
        self.ring, sel, self.wl, _, self.sent[0], counts = retransmit_var(
            self.host, self.total, self.offs[sbase:], self.lens[sbase:], (self.seq0 + sbase) & M32, inflight, self.acked[0],
            self.sent[0], now, timeout, 0, np.full(w * STRIDE, 0xA5, np.uint8), STRIDE, w, np.zeros(w, np.uint32),
            np.zeros(w, np.uint32))
        self.sel = sel[:counts[0]]
        return self.sel, counts

    def receive(self, idx, rbase, off, aidx, sbase, inflight, fill_ms):
        self.rx.wire, self.rx.wl = self.ring, self.wl
        counts = self.rx.round(idx, rbase, off)
        seqs = (self.seq0 + sbase + self.sel[idx].astype(np.int64)) & M32  # one ACK per arrival
        d = (seqs - ((self.seq0 + rbase) & M32)) & M32
        assert ((d < self.window) | (d >= 0x80000000)).all()
        acks = A.ack_bytes(seqs[aidx]).reshape(-1) if aidx.size else np.zeros(16, np.uint8)
        _, _, self.acked[0][:inflight], (adv, _) = R.ingest(acks, 16, np.full(aidx.size, 16, np.uint32), R.SELECTIVE,
                                                             (self.seq0 + sbase) & M32, inflight, self.acked[0][:inflight])
        self.acked[1], self.sent[1] = V.tx_advance(self.acked[0], self.sent[0], self.window, adv, fill_ms, self.acked[1],
                                                   self.sent[1])
        self.acked.reverse()
        self.sent.reverse()
        return counts, adv
