"""Sequential models of the multi-connection flush and slide (include/wtp_crc32.h:
wtp_rx_deliver_flows, wtp_rx_advance_flows), built on deliver_model.deliver and
advance_model.rx_advance: one flow after the other, in flow order.  The caller's arrays are
never modified: copies are returned.

It also holds FlushEnd, the model end of flows_model.transfer that flushes all flows with one
call pair per round and keeps the window bases as the advance leaves them;
tests/test_flows_flush_model.py holds it to flows_model.ModelEnd's rounds and
tests/test_gpu_flows_flush.py runs the device calls behind the same interface."""
import numpy as np

import advance_model as V
import deliver_model
import flows_model as F

MAXP, EMPTY, M32 = F.MAXP, F.EMPTY, F.M32


def deliver_flows(img, slot_len, nflows, window, max_slots, stream, stream_bytes, stream_off, offsets_out=None,
                  lengths_out=None):
    """Returns (stream, offsets_out, lengths_out, flow_adv[nflows], flow_info[nflows, 4], counts)
    after the call; counts = (K, sum of runs, Q_K, bytes all runs need), flow_info[f] = (run_f,
    R_f, B_f, bytes_f).  offsets_out / lengths_out: the prior arrays, or None."""
    assert stream_off <= stream_bytes <= len(stream)
    stream = np.array(stream, dtype=np.uint8, copy=True)
    offs = None if offsets_out is None else np.array(offsets_out, dtype=np.uint64, copy=True)
    lens = None if lengths_out is None else np.array(lengths_out, dtype=np.uint32, copy=True)
    adv, info = np.zeros(nflows, np.uint64), np.zeros((nflows, 4), np.uint64)
    K, at, runs, need, cut = 0, stream_off, 0, 0, False
    for f in range(nflows):
        sub_img, sub_sl = img[f * window * MAXP:(f + 1) * window * MAXP], slot_len[f * window:(f + 1) * window]
        # behind the cut nothing is delivered, whatever would still fit: max_slots 0 reports the run alone
        stream, o, ln, c = deliver_model.deliver(sub_img, sub_sl, window, 0 if cut else max_slots, stream, stream_bytes, at,
                                                 np.zeros(window, np.uint64), np.zeros(window, np.uint32))
        k, run, pk, prun = (int(v) for v in c)
        if offs is not None:
            offs[K:K + k] = o[:k]
        if lens is not None:
            lens[K:K + k] = ln[:k]
        adv[f], info[f] = k, (run, K, at, pk)
        cut = cut or k < min(run, max_slots)
        K, at, runs, need = K + k, at + pk, runs + run, need + prun
    return stream, offs, lens, adv, info, np.array([K, runs, at - stream_off, need], dtype=np.uint64)


def deliver_flows_plan(slot_len, nflows, window, max_slots, stream_bytes, stream_off):
    """deliver_flows without the bytes and without a loop, for states of 2^20 slots: (slots, Q,
    lens, flow_adv, flow_info, counts), where slots[r], Q[r] and lens[r] are the global slot, the
    bytes before it and the length of the delivered record of rank r."""
    sl = np.asarray(slot_len[:nflows * window], dtype=np.int64).reshape(nflows, window)
    run = np.cumprod(sl <= MAXP, axis=1).sum(axis=1)
    s = np.arange(window)[None, :]
    inrun = s < run[:, None]
    cand = inrun & (s < max_slots)
    g = np.flatnonzero(cand.reshape(-1))
    ln = sl.reshape(-1)[g]
    Q = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    K = int(np.searchsorted(Q[1:], stream_bytes - stream_off, side="right"))  # the records whose end still fits
    c = cand.sum(axis=1)
    first = np.concatenate([[0], np.cumsum(c)])[:-1].astype(np.int64)
    adv = np.clip(K - first, 0, c)
    R = np.minimum(first, K)
    info = np.stack([run, R, stream_off + Q[R], Q[R + adv] - Q[R]], axis=1).astype(np.uint64).reshape(nflows, 4)
    counts = np.array([K, run.sum(), Q[K], (sl * inrun).sum()], dtype=np.uint64)
    return g[:K], Q[:K], ln[:K].astype(np.uint32), adv.astype(np.uint64), info, counts


def advance_flows(img, slot_len, nflows, window, flow_adv, seq0, img_next, slot_len_next, seq0_next, fast=False):
    """Returns (img_next, slot_len_next, seq0_next) after the call; the images, or the seq0
    arrays, may both be None (then None is returned for them).  fast: advance_model's loop-free
    form, for large windows."""
    assert (img is None) == (img_next is None) and (seq0 is None) == (seq0_next is None)
    out = None if img_next is None else np.array(img_next, dtype=np.uint8, copy=True)
    sl = np.array(slot_len_next, dtype=np.uint32, copy=True)
    sq = None if seq0_next is None else np.array(seq0_next, dtype=np.uint32, copy=True)
    one = V.rx_advance_fast if fast else V.rx_advance
    for f in range(nflows if window else 0):  # no slots: nothing is written
        lo, hi = f * window, (f + 1) * window
        a = int(flow_adv[f])
        o, sl[lo:hi] = one(None if img is None else img[lo * MAXP:hi * MAXP], slot_len[lo:hi], window, a,
                           None if out is None else out[lo * MAXP:hi * MAXP], sl[lo:hi])
        if out is not None:
            out[lo * MAXP:hi * MAXP] = o
        if sq is not None:
            sq[f] = (int(seq0[f]) + min(a, window)) & M32
    return out, sl, sq


class FlushEnd(F.ModelEnd):
    """flows_model.ModelEnd with the whole flush of a round in one deliver_flows + advance_flows:
    all flows' records go to one round stream (its capacity the bytes all runs need, so nothing
    is cut), the ranges (B_f, bytes_f) of flow_info are appended to the flows' own streams, and
    the bases the next receive uses are those advance_flows left (transfer's rbase is only
    compared with them)."""

    def __init__(self, nflows=F.XFER_FLOWS, window=F.XFER_WINDOW):
        super().__init__(nflows, window)
        self.seq0 = [np.array([self.seq(f, 0) for f in range(nflows)], dtype=np.uint32) for _ in range(2)]
        self.round = None

    def receive(self, gidx, flow, rbase, mode):
        assert self.seq0[0].tolist() == [self.seq(f, rbase[f]) for f in range(self.nflows)]  # moved by the advance alone
        return super().receive(gidx, flow, rbase, mode)

    def flush_all(self):
        """-> (round stream, offsets, lengths, flow_adv, flow_info, counts); swaps nothing."""
        w, nf = self.window, self.nflows
        cap = nf * w * MAXP
        res = deliver_flows(self.img[0], self.sl[0], nf, w, w, np.full(cap, 0xA5, np.uint8), cap, 0, np.zeros(nf * w, np.uint64),
                            np.zeros(nf * w, np.uint32))
        self.img[1], self.sl[1], self.seq0[1] = advance_flows(self.img[0], self.sl[0], nf, w, res[3], self.seq0[0], self.img[1],
                                                              self.sl[1], self.seq0[1])
        return res

    def flush(self, f, off):
        if self.round is None:
            self.round = self.flush_all()
        stream, offs, lens, adv, info, counts = self.round
        assert counts[0] == counts[1] and counts[2] == counts[3]  # the round stream holds every run
        run, R, B, nbytes = (int(v) for v in info[f])
        k = int(adv[f])
        self.stream[f][off:off + nbytes] = stream[B:B + nbytes]
        self.offs[f] += (offs[R:R + k].astype(np.int64) - B + off).tolist()  # rebased to the flow's own stream
        self.lens[f] += lens[R:R + k].tolist()
        return k, nbytes

    def flushed(self):
        super().flushed()
        self.seq0.reverse()
        self.round = None
