"""Models of the multi-connection receive (include/wtp_crc32.h: wtp_accept_data_packets_flows,
wtp_rx_build_acks_flows).

accept_flows is, by definition, accept_model.accept per flow on the subsequence of that flow's
datagrams against the flow's sub-window.  build_acks_flows is written directly from the
header.  ok comes from oracle.verify_datagrams, pinned to the reference.

It also holds the fuzz corpus of the flows tests (each flow's arrivals from
accept_model.fuzz_batch, interleaved by a seeded shuffle that keeps every flow's order) and
the multi-flow transfer driver, which tests/test_flows_model.py runs over the models and
tests/test_gpu_flows.py over the device calls, with the same seed and so the same decisions."""
import numpy as np

import accept_model
import ack_model as A
import advance_model as V
import buildvar_model as B
import deliver_model
import oracle as O
import retx_model as R
import retxvar_model as RV

MAXP, EMPTY, NOT_PLACED, M32 = 1456, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
STRIDE = MAXP + 16
SELECTIVE, CUMULATIVE = 0, 1
NO_FLOW = 0xFFFFFFFF


def rows(ring, stride, idx):
    """The ring slots `idx`, back to back."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    n = ring.size // stride
    return ring[:n * stride].reshape(n, stride)[idx].reshape(-1)


def accept_flows(ring, stride, recv_len, flow, seq0, nflows, window, out, slot_len):
    """Returns (ok, place, out, slot_len, ack[nflows]); `out` / `slot_len` are the state of all
    flows on entry (not modified: copies are returned)."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    flow = np.ascontiguousarray(flow, dtype=np.uint32)
    n = recv_len.size
    assert flow.size == n and len(seq0) >= nflows
    out, slot_len = np.array(out, dtype=np.uint8, copy=True), np.array(slot_len, dtype=np.uint32, copy=True)
    ok = O.verify_datagrams(ring, stride, recv_len)[0] if n else np.zeros(0, np.uint8)
    place = np.full(n, NOT_PLACED, dtype=np.uint32)
    ack = np.zeros(nflows, dtype=np.uint32)
    for f in range(nflows):
        idx = np.flatnonzero(flow == f)
        lo, hi = f * window, (f + 1) * window
        ok_f, place[idx], out[lo * MAXP:hi * MAXP], slot_len[lo:hi], ack[f] = accept_model.accept(
            rows(ring, stride, idx) if idx.size else np.zeros(0, np.uint8), stride, recv_len[idx], int(seq0[f]), window,
            out[lo * MAXP:hi * MAXP], slot_len[lo:hi])
        assert np.array_equal(ok_f, ok[idx])
    return ok, place, out, slot_len, ack


def build_acks_flows(ring, stride, recv_len, flow, mode, seq0, nflows, window, ok, flow_ack=None, skip=0, max_acks=None):
    """Returns (ack_seq, src, (emitted, eligible)): the seqNum and the datagram index of every
    emitted ACK, in order.  `ok` / `flow_ack`: accept_flows' outputs."""
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    n = recv_len.size
    seqs_out, src = [], []
    total = 0
    hi = skip + (n if max_acks is None else max_acks)
    for i in range(n):
        f = int(flow[i])
        if not ok[i] or f >= nflows:
            continue
        h = ring[i * stride:i * stride + 8]
        ptype, seq = int.from_bytes(h[0:4].tobytes(), "big"), int.from_bytes(h[4:8].tobytes(), "big")
        d = (seq - int(seq0[f])) & M32
        if ptype != 2 or int(recv_len[i]) - 16 > MAXP or not (d < window or d >= 0x80000000):
            continue
        if skip <= total < hi:
            seqs_out.append(seq if mode == SELECTIVE else int(flow_ack[f]))
            src.append(i)
        total += 1
    return np.array(seqs_out, dtype=np.uint32), np.array(src, dtype=np.uint32), (len(src), total)


def interleave(rng, counts):
    """A seeded arrival order for counts[f] datagrams of flow f that keeps every flow's own
    order: (label of every arrival, its index within its flow)."""
    labels = np.repeat(np.arange(len(counts)), counts)
    labels = labels[rng.permutation(labels.size)]
    within = np.zeros(labels.size, dtype=np.int64)
    for f in range(len(counts)):
        at = np.flatnonzero(labels == f)
        within[at] = np.arange(at.size)
    return labels, within


def reinterleave(rng, flow):
    """A permutation of the datagrams that keeps every flow's order (datagrams of unknown flows
    count as one more flow): new position j holds old datagram perm[j]."""
    flow = np.asarray(flow)
    ids, inv = np.unique(flow, return_inverse=True)
    labels, within = interleave(rng, np.bincount(inv, minlength=ids.size))
    per_flow = [np.flatnonzero(inv == k) for k in range(ids.size)]
    return np.array([per_flow[k][w] for k, w in zip(labels, within)], dtype=np.int64)


# ---- the corpus of the randomised differential test -------------------------------------------
FUZZ_SEEDS = range(12)
FUZZ_BASE = 0xF10E5
FUZZ_CALLS = 2


def fuzz_case(seed):
    """(rng, nflows, window, seq0[nflows], stride, ring_off, out_off) of one seed: FUZZ_CALLS
    successive calls on one state.  Seeds divisible by 3 give flows 0 and 1 the same base (the
    same seqNums in two flows), odd seeds put flow 0 within 3 of the 2^32 wrap."""
    rng = np.random.default_rng(FUZZ_BASE + seed)
    nflows = int(rng.integers(2, 6))
    window = int(rng.integers(3, 90))
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    if seed % 2:
        seq0[0] = (1 << 32) - 1 - int(rng.integers(3))
    if seed % 3 == 0:
        seq0[1] = seq0[0]
    stride = accept_model.FUZZ_STRIDES[seed % len(accept_model.FUZZ_STRIDES)]
    ring_off = (0, 0, 1, 8)[int(rng.integers(4))]
    out_off = (0, 0, 4)[int(rng.integers(3))]
    return rng, nflows, window, seq0, stride, ring_off, out_off


def fuzz_batch(rng, seq0, nflows, window, stride, state):
    """(ring, recv_len, flow, kinds) of one batch: 17 .. 60 datagrams per flow from
    accept_model.fuzz_batch against that flow's sub-window (so every kind of
    accept_model.fuzz_kinds(stride) is dealt to a datagram of every flow), and as many for no
    connection (made for flow 0's window, labelled nflows or 0xFFFFFFFF), interleaved.  kinds[i]
    is the datagram's set of kinds."""
    parts = []
    for f in list(range(nflows)) + [0]:
        parts.append(accept_model.fuzz_batch(rng, int(seq0[f]), window, stride, state[f * window:(f + 1) * window],
                                             n=int(rng.integers(17, 61))))
    labels, within = interleave(rng, [p[1].size for p in parts])
    n = labels.size
    ring = np.zeros(n * stride, dtype=np.uint8)
    recv_len, flow, kinds = np.zeros(n, np.uint32), np.zeros(n, np.uint32), []
    for i, (k, w) in enumerate(zip(labels, within)):
        ring[i * stride:(i + 1) * stride] = parts[k][0][w * stride:(w + 1) * stride]
        recv_len[i] = parts[k][1][w]
        flow[i] = k if k < nflows else (nflows, NO_FLOW)[int(rng.integers(2))]
        kinds.append(parts[k][2][w])
    return ring, recv_len, flow, kinds


def fuzz_calls(seed):
    """Every call of one seed with the model's verdicts: a list of dicts (ring, rl, flow, kinds,
    out0, sl0: the state on entry; want: accept_flows' result), then the case's parameters."""
    rng, nflows, window, seq0, stride, ring_off, out_off = fuzz_case(seed)
    out = np.full(nflows * window * MAXP, 0xA5, np.uint8)
    sl = np.full(nflows * window, EMPTY, np.uint32)
    calls = []
    for _ in range(FUZZ_CALLS):
        ring, rl, flow, kinds = fuzz_batch(rng, seq0, nflows, window, stride, sl)
        want = accept_flows(ring, stride, rl, flow, seq0, nflows, window, out, sl)
        calls.append(dict(ring=ring, rl=rl, flow=flow, kinds=kinds, out0=out, sl0=sl, want=want))
        out, sl = want[2], want[3]
    return calls, (nflows, window, seq0, stride, ring_off, out_off)


# ---- a transfer of several connections through one receiver ------------------------------------
# XFER_FLOWS senders of XFER_RECORDS mixed-length records each, a sender window and a receiver
# window of XFER_WINDOW slots per connection.  A round is, in stream order,
#   senders   wtp_tx_build_retransmit_var per sender over its window: first transmissions and
#             retransmissions (timeout 1, a clock that advances 1 per round and wraps)
#   channel   per sender, every emitted datagram is lost (XFER_LOSS), doubled (XFER_DUP) and
#             permuted; the survivors of all senders are interleaved in one arrival order
#   receiver  one accept_flows + one acks_flows over all arrivals, then per connection the
#             existing deliver -> rx_advance on its sub-window, and its base moves
#   channel   the ACK ring, lossy and permuted; the ACKs of a connection go to its sender
#   senders   wtp_tx_ingest_acks -> wtp_tx_advance per sender
# Connection 1's sequence numbers wrap 2^32; connections 2 and 3 use the same numbers.
XFER_FLOWS, XFER_RECORDS, XFER_WINDOW, XFER_LOSS, XFER_DUP, XFER_SEED = 4, 40, 8, 0.15, 0.15, 0xF70
XFER_SEQ = (1000, 0xFFFFFFF0, 77777, 77777)
XFER_TIMEOUT, XFER_NOW0 = 1, 0xFFFFFFFA
XFER_MAX_ROUNDS = 60


def xfer_records(f):
    """(lengths, offsets, total, host bytes) of sender f's records."""
    lens = O.zipf_lengths(XFER_RECORDS, seed=900 + f)
    lens[3 + f:7 + f] = [0, 1456, 1, 17]
    total = int(lens.sum())
    return lens, B.packed_offsets(lens), total, O.synth_fill_np(total, start_byte=11 * f + 1)


def transfer(end, mode, nflows=XFER_FLOWS, nrec=XFER_RECORDS, window=XFER_WINDOW, loss=XFER_LOSS, dup=XFER_DUP,
             seed=XFER_SEED, max_rounds=XFER_MAX_ROUNDS):
    """Drives `end` until every sender's window has passed its last record:
      end.emit(f, sbase, inflight, now, timeout) -> sel: sender f's call; its ring entries are
        entries f*window + k of the wire
      end.receive(gidx, flow, rbase, mode) -> (flow_ack, src): one accept_flows + acks_flows over
        wire entries gidx (arrival order); src = the datagram index of every ACK in the ring
      end.flush(f, off) -> (k, bytes): deliver -> rx_advance of flow f; end.flushed() after all
      end.ingest(f, aidx, mode, sbase, inflight, fill_ms) -> adv: ingest ring entries aidx, slide
    Returns (log, stats): every round's decisions and results, and per flow the number of lost,
    doubled and out-of-order arrivals."""
    rng = np.random.default_rng(seed)
    sbase, rbase, off = [0] * nflows, [0] * nflows, [0] * nflows
    now = XFER_NOW0
    log, stats = [], np.zeros((nflows, 3), dtype=np.int64)
    while any(s < nrec for s in sbase):
        if len(log) == max_rounds:
            raise AssertionError(f"transfer not finished after {max_rounds} rounds (sender bases {sbase} of {nrec})")
        inflight = [min(window, nrec - s) for s in sbase]
        sent, lists = [], []
        for f in range(nflows):
            sel = [int(s) for s in end.emit(f, sbase[f], inflight[f], now, XFER_TIMEOUT)] if inflight[f] else []
            m = len(sel)
            keep, twice = rng.random(m) >= loss, rng.random(m) < dup
            ks = np.array([k for k in range(m) if keep[k] for _ in range(2 if twice[k] else 1)], dtype=np.int64)
            ks = ks[rng.permutation(ks.size)]
            arrived = [sel[k] for k in ks]
            stats[f] += (m - int(keep.sum()), int((keep & twice).sum()),
                         sum(1 for a, b in zip(arrived, arrived[1:]) if b < a))
            sent.append(sel)
            lists.append(f * window + ks)
        labels, within = interleave(rng, [x.size for x in lists])
        gidx = np.array([lists[f][w] for f, w in zip(labels, within)], dtype=np.int64)
        now = (now + 1) & M32
        flow_ack, src = end.receive(gidx, labels.astype(np.uint32), rbase, mode)
        flushed = []
        for f in range(nflows):
            k, nbytes = end.flush(f, off[f])
            assert (int(flow_ack[f]) - XFER_SEQ[f] - rbase[f]) & M32 == k  # deliver's run is the flow's ACK
            rbase[f] += k
            off[f] += nbytes
            flushed.append((k, nbytes))
        end.flushed()
        nack = len(src)
        aidx = rng.permutation(nack)
        aidx = aidx[rng.random(nack)[aidx] >= loss]
        advs = []
        for f in range(nflows):
            mine = np.array([a for a in aidx if labels[src[a]] == f], dtype=np.int64)
            adv = end.ingest(f, mine, mode, sbase[f], inflight[f], (now - XFER_TIMEOUT - 1) & M32) if inflight[f] else 0
            sbase[f] += adv
            assert sbase[f] <= rbase[f]
            advs.append(adv)
        log.append((sent, gidx.tolist(), [int(a) for a in flow_ack], [int(s) for s in src], flushed, advs))
    return log, stats


class ModelEnd:
    """Every connection's two ends on the models: retxvar_model.retransmit_var, retx_model.ingest
    and advance_model.tx_advance per sender; accept_flows and build_acks_flows over all of them;
    deliver_model.deliver and advance_model.rx_advance per flow on its sub-window."""

    def __init__(self, nflows=XFER_FLOWS, window=XFER_WINDOW):
        self.nflows, self.window = nflows, window
        self.rec = [xfer_records(f) for f in range(nflows)]
        w = window
        self.acked = [[np.zeros(w, np.uint32) for _ in range(2)] for _ in range(nflows)]
        self.sent = [[np.full(w, (XFER_NOW0 - XFER_TIMEOUT - 1) & M32, np.uint32) for _ in range(2)] for _ in range(nflows)]
        self.wire = np.full(nflows * w * STRIDE, 0xA5, np.uint8)
        self.wl = np.zeros(nflows * w, np.uint32)
        self.img = [np.full(nflows * w * MAXP, 0x3C, np.uint8) for _ in range(2)]
        self.sl = [np.full(nflows * w, EMPTY, np.uint32) for _ in range(2)]
        self.stream = [np.full(r[2], 0xA5, np.uint8) for r in self.rec]
        self.offs, self.lens = [[] for _ in range(nflows)], [[] for _ in range(nflows)]

    def seq(self, f, chunk):
        return (XFER_SEQ[f] + chunk) & M32

    def emit(self, f, sbase, inflight, now, timeout):
        w = self.window
        lens, offs, total, host = self.rec[f]
        ring, sel, wl, _, self.sent[f][0], counts = RV.retransmit_var(
            host, total, offs[sbase:], lens[sbase:], self.seq(f, sbase), inflight, self.acked[f][0], self.sent[f][0], now,
            timeout, 0, self.wire[f * w * STRIDE:(f + 1) * w * STRIDE], STRIDE, w, np.zeros(w, np.uint32),
            self.wl[f * w:(f + 1) * w])
        self.wire[f * w * STRIDE:(f + 1) * w * STRIDE], self.wl[f * w:(f + 1) * w] = ring, wl
        return sel[:counts[0]]

    def receive(self, gidx, flow, rbase, mode):
        w, F = self.window, self.nflows
        seq0 = np.array([self.seq(f, rbase[f]) for f in range(F)], dtype=np.uint32)
        ring = rows(self.wire, STRIDE, gidx) if gidx.size else np.zeros(0, np.uint8)
        rl = self.wl[gidx]
        ok, _, self.img[0], self.sl[0], ack = accept_flows(ring, STRIDE, rl, flow, seq0, F, w, self.img[0], self.sl[0])
        assert ok.all()
        self.ack_seq, src, (emitted, total) = build_acks_flows(ring, STRIDE, rl, flow, mode, seq0, F, w, ok, ack)
        assert emitted == total == gidx.size  # every arrival is inside its flow's window or below it
        return ack, src

    def flush(self, f, off):
        w = self.window
        img, sl = self.img[0][f * w * MAXP:(f + 1) * w * MAXP], self.sl[0][f * w:(f + 1) * w]
        self.stream[f], offs, lens, counts = deliver_model.deliver(img, sl, w, w, self.stream[f], self.stream[f].size, off,
                                                                   np.zeros(w, np.uint64), np.zeros(w, np.uint32))
        k = int(counts[0])
        assert counts[0] == counts[1] and counts[2] == counts[3]  # the stream buffer holds the whole transfer
        self.offs[f] += offs[:k].tolist()
        self.lens[f] += lens[:k].tolist()
        self.img[1][f * w * MAXP:(f + 1) * w * MAXP], self.sl[1][f * w:(f + 1) * w] = V.rx_advance(
            img, sl, w, k, self.img[1][f * w * MAXP:(f + 1) * w * MAXP], self.sl[1][f * w:(f + 1) * w])
        return k, int(counts[2])

    def flushed(self):
        self.img.reverse()
        self.sl.reverse()

    def ingest(self, f, aidx, mode, sbase, inflight, fill_ms):
        w = self.window
        acks = A.ack_bytes(self.ack_seq[aidx]).reshape(-1) if aidx.size else np.zeros(16, np.uint8)
        _, _, self.acked[f][0][:inflight], (adv, _) = R.ingest(acks, 16, np.full(aidx.size, 16, np.uint32), mode,
                                                                self.seq(f, sbase), inflight, self.acked[f][0][:inflight])
        self.acked[f][1], self.sent[f][1] = V.tx_advance(self.acked[f][0], self.sent[f][0], w, adv, fill_ms,
                                                         self.acked[f][1], self.sent[f][1])
        self.acked[f].reverse()
        self.sent[f].reverse()
        return int(adv)
