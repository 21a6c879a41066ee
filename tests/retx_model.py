"""Sequential model of the device-side sender window (include/wtp_crc32.h:
wtp_tx_ingest_acks, wtp_tx_build_retransmit), written from the header's semantics: one
datagram, then one slot, at a time over a window the caller owns.  ok comes from
oracle.verify_datagrams, pinned to the reference, cut at the kernels' payload limit
(verify_limited).  Entry state is never modified: copies are returned.  A vectorised numpy
path gives the same results for windows of 2^20 slots (tests/test_retx_model.py checks it
against the literal loops)."""
import numpy as np

import oracle as O

MAXP = 1456
NOT_PLACED = 0xFFFFFFFF
M32 = 0xFFFFFFFF
SELECTIVE, CUMULATIVE = 0, 1
RETX_ALL = 1


def ack_datagram(seq, ptype=3, checksum=0, payload=b""):
    """The 16-byte header htonl{type, seq, len(payload), checksum} || payload."""
    h = np.array([ptype, seq & M32, len(payload), checksum & M32], dtype=">u4").tobytes()
    return h + bytes(payload)


MAX_KERNEL_LEN = 4096  # WTP_MAX_KERNEL_LEN


def verify_limited(ring, stride, recv_len):
    """(ok, crc) as wtp_crc32_verify_batch writes them: the oracle's verdict (the reference
    has no length limit), except that a payload above WTP_MAX_KERNEL_LEN is not ok and gets
    crc 0.  The one place where the models take the limit from."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    if recv_len.size == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    ok, crc = O.verify_datagrams(ring, stride, recv_len)
    within = recv_len.astype(np.int64) - 16 <= MAX_KERNEL_LEN
    return (ok * within).astype(np.uint8), (crc * within).astype(np.uint32)


def headers(ring, stride, n):
    """(type, seqNum) of n datagrams as uint32 arrays (whatever bytes are there)."""
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    idx = (np.arange(n, dtype=np.int64) * stride)[:, None] + np.arange(8)
    h = np.ascontiguousarray(ring[idx]).view(">u4")
    return h[:, 0].astype(np.uint32), h[:, 1].astype(np.uint32)


def ingest(ring, stride, recv_len, mode, seq0, inflight, acked, vectorised=False):
    """Returns (ok, hit, acked, (advance, newly))."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    n = recv_len.size
    acked = np.array(acked, dtype=np.uint32, copy=True)
    ok = verify_limited(ring, stride, recv_len)[0]
    if vectorised:
        return (ok,) + _ingest_vectorised(ring, stride, n, ok, mode, seq0, inflight, acked)
    hit = np.full(n, NOT_PLACED, dtype=np.uint32)
    newly = 0
    for i in range(n):
        if not ok[i]:
            continue
        h = ring[i * stride:i * stride + 16].tobytes()
        if int.from_bytes(h[0:4], "big") != 3:
            continue
        d = (int.from_bytes(h[4:8], "big") - seq0) & M32
        if mode == SELECTIVE:
            if d < inflight:
                hit[i] = d
                newly += int(acked[d] == 0)
                acked[d] = max(int(acked[d]), 1)
        elif 0 < d <= inflight:
            hit[i] = d
            for s in range(d):
                if acked[s] == 0:
                    acked[s] = 1
                    newly += 1
    lead = 0
    while lead < inflight and acked[lead] != 0:
        lead += 1
    return ok, hit, acked, (lead, newly)


def _ingest_vectorised(ring, stride, n, ok, mode, seq0, inflight, acked):
    """The loop above without a loop: the batch's marks are a set (selective) or a prefix
    (cumulative), so their order only matters for d_hit, which is per datagram."""
    types, seqs = headers(ring, stride, n)
    d = (seqs.astype(np.int64) - seq0) & M32
    counts = (ok != 0) & (types == 3) & ((d < inflight) if mode == SELECTIVE else ((d > 0) & (d <= inflight)))
    hit = np.where(counts, d, NOT_PLACED).astype(np.uint32)
    if mode == SELECTIVE:
        marks = np.unique(d[counts])
    else:
        marks = np.arange(int(d[counts].max()) if counts.any() else 0)
    newly = int((acked[marks] == 0).sum())
    acked[marks] = np.maximum(acked[marks], 1)
    zeros = np.flatnonzero(acked[:inflight] == 0)
    return hit, acked, (int(zeros[0]) if zeros.size else inflight, newly)


def slot_len(s, total_bytes):
    return min(MAXP, total_bytes - s * MAXP)


def retransmit(payloads, total_bytes, seq0, inflight, acked, sent_ms, now_ms, timeout_ms, flags, max_sel, build=True,
               vectorised=False):
    """Returns (sel, dgrams, sent_ms, (emitted, due)): sel the emitted slots in order, dgrams
    their datagrams as bytes (left empty with build=False, for windows whose bytes the
    caller compares by other means)."""
    sent_ms = np.array(sent_ms, dtype=np.uint32, copy=True)
    if vectorised:
        age = (now_ms - sent_ms[:inflight].astype(np.int64)) & M32
        is_due = (np.asarray(acked)[:inflight] == 0) & (bool(flags & RETX_ALL) | (age > timeout_ms))
        sel = np.flatnonzero(is_due)
        due, sel = sel.size, sel[:max_sel]
        sent_ms[sel] = now_ms & M32
        dgrams = [O.build_datagram((seq0 + int(s)) & M32, bytes(payloads[int(s) * MAXP:int(s) * MAXP + slot_len(int(s), total_bytes)]))
                  for s in sel] if build else []  # over the emitted datagrams, not the window
        return sel.astype(np.uint32), dgrams, sent_ms, (int(sel.size), int(due))
    sel, dgrams, due = [], [], 0
    for s in range(inflight):
        if acked[s] != 0:
            continue
        if not (flags & RETX_ALL) and ((now_ms - int(sent_ms[s])) & M32) <= timeout_ms:
            continue
        due += 1
        if len(sel) < max_sel:
            ln = slot_len(s, total_bytes)
            sel.append(s)
            if build:
                dgrams.append(O.build_datagram((seq0 + s) & M32, bytes(payloads[s * MAXP:s * MAXP + ln])))
            sent_ms[s] = now_ms & M32
    return np.array(sel, dtype=np.uint32), dgrams, sent_ms, (len(sel), due)


# ---- datagrams around the kernels' payload limit ---------------------------------------------
def limit_corpus(stride, ptype, count, seed, window, over=True):
    """`count` datagrams of type `ptype` with valid checksums whose payload lengths cycle
    through 0, 1, 3, 4, 255, 1456, 1457, 4095, 4096, 4097 and stride - 16 (`over` False: only
    those of at most WTP_MAX_KERNEL_LEN bytes, in the same order), in seeded random order,
    plus one datagram with a flipped payload bit for each length above 1456.  seqNums are
    below `window`: payloads of at most 1456 bytes in its lower half, each seqNum once,
    longer ones in its upper half.  Returns (dgrams, payload lengths)."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 3, 4, 255, MAXP, MAXP + 1, 4095, 4096, 4097, stride - 16]
    pick = [lens[i % len(lens)] for i in range(count)] + [-ln for ln in lens if ln > MAXP]
    pick = [pick[i] for i in rng.permutation(len(pick))]
    low = iter(rng.permutation(window // 2).tolist())
    dgrams, out = [], []
    for k, ln in enumerate(pick):
        corrupt, ln = ln < 0, abs(ln)
        seq = next(low) if ln <= MAXP else window // 2 + int(rng.integers(0, window - window // 2))
        d = bytearray(O.build_datagram(seq, O.synth_fill_np(ln, start_byte=97 * k, seed=seed).tobytes(), ptype))
        if corrupt:
            d[16 + int(rng.integers(0, ln))] ^= 0x04
        if over or ln <= MAX_KERNEL_LEN:
            dgrams.append(bytes(d))
            out.append(ln)
    return dgrams, np.array(out, dtype=np.int64)


# ---- a whole transfer between two windows ------------------------------------------------
STRIDE = MAXP + 16
EMPTY = 0xFFFFFFFF
# the end-to-end case of tests/test_gpu_retx.py and tests/test_retx_model.py: 300 chunks, the
# last one 456 bytes, window 64, each channel drops 30 %
E2E_CHUNKS, E2E_SHORT, E2E_WINDOW, E2E_LOSS, E2E_SEED = 300, 1000, 64, 0.3, 0xE2E


def make_ring(dgrams, stride):
    ring = np.zeros(max(len(dgrams), 1) * stride, dtype=np.uint8)
    rl = np.zeros(len(dgrams), dtype=np.uint32)
    for i, d in enumerate(dgrams):
        ring[i * stride:i * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
        rl[i] = len(d)
    return ring, rl


def transfer(end, nchunks, window, seq_base, mode, seed, loss, max_rounds=40):
    """Drives one transfer over two lossy, reordering channels between the sender window and
    the receiver window of `end` (ModelEnd below, or the device endpoint of
    tests/test_gpu_retx.py: the same calls, the same seeds, so the same decisions).

    Per round: build the new chunks the window admits; they and the previous round's
    retransmissions cross the data channel (drop and permute by datagram index); accept;
    ACKs cross the second channel; ingest; the clock advances 600 ms; build-retransmit with
    timeout 500 (selective) or WTP_RETX_ALL (cumulative); both windows move by their
    advance.  Selective mode ACKs every intact DATA datagram inside the receiver's window
    or below it (a packet whose ACK was lost is re-sent after the receiver has moved on, and
    must be ACKed again or the sender never finishes); cumulative mode sends accept's
    cumulative ACK once per delivered datagram.  Returns (rounds, [retransmit set of each
    round as absolute chunk numbers]); raises if `max_rounds` is reached."""
    data_rng, ack_rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    sbase = rbase = nxt = 0
    now = 0xFFFFFE00 if seq_base else 1000  # the clock wraps with the sequence numbers
    sets = []
    for rnd in range(1, max_rounds + 1):
        top = min(sbase + window, nchunks)
        m = end.send(nxt, top - nxt, now)
        nxt = top
        keep = data_rng.random(m) >= loss
        idx = data_rng.permutation(m)
        idx = idx[keep[idx]]
        ok, types, seqs, ack = end.accept(idx, rbase)
        if mode == SELECTIVE:
            d = (seqs.astype(np.int64) - ((seq_base + rbase) & M32)) & M32
            inwin = (ok != 0) & (types == 2) & ((d < window) | (d >= (1 << 31)))
            acks = [ack_datagram(int(s)) for s in seqs[inwin]]
        else:
            acks = [ack_datagram(ack)] * idx.size
        akeep = ack_rng.random(len(acks)) >= loss
        aidx = ack_rng.permutation(len(acks))
        acks = [acks[i] for i in aidx if akeep[i]]
        inflight = nxt - sbase
        adv = end.ingest(acks, mode, sbase, inflight)
        now = (now + 600) & M32
        sel = end.retransmit(sbase, inflight, now, 500, RETX_ALL if mode == CUMULATIVE else 0, window)
        sets.append([sbase + int(s) for s in sel])
        sbase += adv
        rbase = (ack - seq_base) & M32
        if sbase == nchunks:
            return rnd, sets
    raise AssertionError(f"transfer not finished after {max_rounds} rounds (sender base {sbase} of {nchunks})")


class ModelEnd:
    """Both windows on the CPU: the models above plus accept_model.accept."""

    def __init__(self, src, nchunks, window, seq_base):
        self.src, self.total, self.window, self.seq_base = src, src.size, window, seq_base
        self.acked = np.zeros(nchunks + window, dtype=np.uint32)
        self.sent = np.zeros(nchunks + window, dtype=np.uint32)
        self.img = np.full((nchunks + window) * MAXP, 0xA5, dtype=np.uint8)
        self.slot_len = np.full(nchunks + window, EMPTY, dtype=np.uint32)
        self.retx = []

    def seq(self, chunk):
        return (self.seq_base + chunk) & M32

    def send(self, c0, cnt, now):
        new = [O.build_datagram(self.seq(c), self.src[c * MAXP:(c + 1) * MAXP].tobytes()) for c in range(c0, c0 + cnt)]
        self.sent[c0:c0 + cnt] = now
        self.wire = new + self.retx
        return len(self.wire)

    def accept(self, idx, rbase):
        import accept_model
        ring, rl = make_ring([self.wire[i] for i in idx], STRIDE)
        w = self.window
        ok, _, out, sl, ack = accept_model.accept(ring, STRIDE, rl, self.seq(rbase), w,
                                                  self.img[rbase * MAXP:(rbase + w) * MAXP], self.slot_len[rbase:rbase + w])
        self.img[rbase * MAXP:(rbase + w) * MAXP], self.slot_len[rbase:rbase + w] = out, sl
        hdr = ring[:rl.size * STRIDE].reshape(rl.size, STRIDE)[:, :8].copy().view(">u4")
        return ok, hdr[:, 0].astype(np.uint32), hdr[:, 1].astype(np.uint32), ack

    def ingest(self, acks, mode, sbase, inflight):
        ring, rl = make_ring(acks, 16)
        _, _, a, (adv, _) = ingest(ring, 16, rl, mode, self.seq(sbase), inflight, self.acked[sbase:sbase + inflight])
        self.acked[sbase:sbase + inflight] = a
        return adv

    def retransmit(self, sbase, inflight, now, timeout, flags, max_sel):
        sel, self.retx, sent, _ = retransmit(self.src[sbase * MAXP:], self.total - sbase * MAXP, self.seq(sbase), inflight,
                                             self.acked[sbase:sbase + inflight], self.sent[sbase:sbase + inflight], now,
                                             timeout, flags, max_sel)
        self.sent[sbase:sbase + inflight] = sent
        return sel
