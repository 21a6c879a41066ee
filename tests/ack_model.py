"""Sequential model of the device-side ACK generation (include/wtp_crc32.h:
wtp_rx_build_acks), written from the header's semantics: one datagram at a time over a
window that is fixed for the batch.  ok comes from oracle.verify_datagrams, pinned to the
reference, unless the caller passes its own.  A vectorised numpy path gives the same
result for large windows (tests/test_ack_model.py checks it against the literal loop).

It also holds the transfer driver of the ACK tests: the loop of retx_model.transfer with
the host's ACK construction replaced by `end.build_acks`, which returns the emitted ring."""
import numpy as np

import oracle as O
import retx_model as R

MAXP = 1456
EMPTY = 0xFFFFFFFF
NOT_PLACED = 0xFFFFFFFF
M32 = 0xFFFFFFFF
SELECTIVE, CUMULATIVE = 0, 1


def headers(ring, stride, n):
    """(type, seqNum) of n datagrams as uint32 arrays (whatever bytes are there)."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    idx = (np.arange(n, dtype=np.int64) * stride)[:, None] + np.arange(8)
    h = np.ascontiguousarray(ring[idx]).view(">u4")
    return h[:, 0].astype(np.uint32), h[:, 1].astype(np.uint32)


def eligible(ring, stride, recv_len, seq0, window, ok):
    """The eligibility predicate per datagram (bool array) and the seqNums."""
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    types, seqs = headers(ring, stride, recv_len.size)
    d = (seqs.astype(np.int64) - seq0) & M32
    ln = (recv_len.astype(np.int64) - 16) & M32
    return (np.asarray(ok) != 0) & (types == 2) & (ln <= MAXP) & ((d < window) | (d >= 0x80000000)), seqs


def build_acks(ring, stride, recv_len, mode, seq0, window, place=None, slot_len=None, ok=None, skip=0, max_acks=None,
               vectorised=False):
    """Returns (ack_seq, src, (emitted, eligible)): the seqNum and the datagram index of every
    emitted ACK, in order.  `place` / `slot_len`: accept's output and the window after it."""
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    n = recv_len.size
    if ok is None:
        ok = O.verify_datagrams(np.ascontiguousarray(ring, dtype=np.uint8), stride, recv_len)[0] if n else np.zeros(0, np.uint8)
    ans, seqs = eligible(ring, stride, recv_len, seq0, window, ok)
    if mode == SELECTIVE:
        run = seqs.astype(np.int64)
    elif vectorised:
        never = n + 1
        ft = np.where(np.asarray(slot_len[:window]) != EMPTY, 0, never).astype(np.int64)  # 0: before the batch
        p = np.asarray(place[:n]).astype(np.int64)
        j = np.flatnonzero(p < window)
        named = np.full(window, never, dtype=np.int64)
        np.minimum.at(named, p[j], j + 1)
        ft = np.where(named != never, named, ft)
        T = np.maximum.accumulate(ft) if window else ft
        run = seq0 + np.searchsorted(T, np.arange(n) + 1, side="right")
    else:
        named = set(int(s) for s in place[:n] if s < window)
        filled = set(s for s in range(window) if slot_len[s] != EMPTY and s not in named)
        lead, run = 0, np.zeros(n, dtype=np.int64)
        for i in range(n):
            if place[i] < window:
                filled.add(int(place[i]))  # the lowest index naming a slot fills it
            while lead < window and lead in filled:
                lead += 1
            run[i] = seq0 + lead
    src = np.flatnonzero(ans)
    total = src.size
    src = src[skip:] if max_acks is None else src[skip:skip + max_acks]
    return (run[src] & M32).astype(np.uint32), src.astype(np.uint32), (src.size, total)


def ack_bytes(seqs):
    """The wire image of ACKs with these seqNums: 16 bytes each, as retx_model.ack_datagram."""
    h = np.zeros((len(seqs), 4), dtype=">u4")
    h[:, 0] = 3
    h[:, 1] = seqs
    return h.view(np.uint8).reshape(len(seqs), 16)


# ---- seeded traces: every kind of datagram a receive ring can hold ---------------------------
def prefilled(rng, window):
    """A window state with a leading run and some scattered slots filled before the batch."""
    sl = np.where(rng.random(window) < 0.15, rng.integers(0, MAXP + 1, window), EMPTY).astype(np.uint32)
    sl[:int(rng.integers(0, window // 3 + 1))] = MAXP
    return sl


def trace(rng, n, seq0, window, slot_len, stride):
    """n datagrams in a seeded random mix.  Returns (dgrams, facts): facts[i] = (intact,
    type, seqNum, payload bytes) as the generator made them, for a literal receiver that
    does not parse the ring.  Kinds: 0-2 intact DATA inside the window, 3 a corrupt
    checksum, 4 a 12-byte runt, 5 a payload of 1457-1484 B (intact only where the slot
    holds it), 6 a non-DATA type, 7 below the window, 8 at or above its end, 9 a duplicate
    of an earlier datagram of the batch, 10 a duplicate of a slot filled before."""
    full = np.flatnonzero(slot_len != EMPTY)
    dgrams, facts = [], []
    for i in range(n):
        kind = int(rng.integers(0, 11))
        ptype, plen = 2, int(rng.choice([0, 1, 17, 40, MAXP], p=[0.1, 0.3, 0.3, 0.25, 0.05]))
        seq = seq0 + int(rng.integers(0, max(window, 1)))
        if kind == 5:
            plen = int(rng.integers(MAXP + 1, MAXP + 29))
        elif kind == 6:
            ptype = int(rng.choice([0, 1, 3]))
        elif kind == 7:
            seq = seq0 - int(rng.integers(1, 50))
        elif kind == 8:
            seq = seq0 + window + int(rng.integers(0, 50))
        elif kind == 9 and facts:
            seq = facts[int(rng.integers(0, len(facts)))][2]
        elif kind == 10 and full.size:
            seq = seq0 + int(rng.choice(full))
        seq &= M32
        d = O.build_datagram(seq, O.synth_fill_np(plen, start_byte=7 * i).tobytes(), ptype)
        if kind == 3:
            d = d[:12] + bytes([d[12] ^ 0x40]) + d[13:]
        elif kind == 4:
            d = d[:12]
        dgrams.append(d)
        facts.append((kind not in (3, 4) and len(d) <= stride, ptype, seq, plen))
    return dgrams, facts


# ---- a whole transfer with device-side ACKs ------------------------------------------------
def transfer(end, nchunks, window, seq_base, mode, seed, loss, max_rounds=40):
    """retx_model.transfer with the receiver's ACKs built by `end.build_acks(mode, rbase)`
    for the batch just accepted, which returns the number of ACKs in its ring; the lossy,
    reordering ACK channel is the index list `end.ingest_ring(sel, ...)` takes (the ring
    itself stays where `end` keeps it).  Same seeds and draws as retx_model.transfer, so
    selective mode makes the same decisions; cumulative mode sends the running ACK of each
    datagram instead of the batch's final one.  Returns (rounds, retransmit sets)."""
    data_rng, ack_rng = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    sbase = rbase = nxt = 0
    now = 0xFFFFFE00 if seq_base else 1000
    sets = []
    for rnd in range(1, max_rounds + 1):
        top = min(sbase + window, nchunks)
        m = end.send(nxt, top - nxt, now)
        nxt = top
        keep = data_rng.random(m) >= loss
        idx = data_rng.permutation(m)
        idx = idx[keep[idx]]
        ack = end.accept(idx, rbase)
        nack = end.build_acks(mode, rbase)
        akeep = ack_rng.random(nack) >= loss
        aidx = ack_rng.permutation(nack)
        aidx = aidx[akeep[aidx]]
        inflight = nxt - sbase
        adv = end.ingest_ring(aidx, mode, sbase, inflight)
        now = (now + 600) & M32
        sel = end.retransmit(sbase, inflight, now, 500, R.RETX_ALL if mode == CUMULATIVE else 0, window)
        sets.append([sbase + int(s) for s in sel])
        sbase += adv
        rbase = (ack - seq_base) & M32
        if sbase == nchunks:
            return rnd, sets
    raise AssertionError(f"transfer not finished after {max_rounds} rounds (sender base {sbase} of {nchunks})")


class ModelEnd(R.ModelEnd):
    """retx_model.ModelEnd with the receiver's reply ring from build_acks above."""

    def accept(self, idx, rbase):
        import accept_model
        self.ring, self.rl = R.make_ring([self.wire[i] for i in idx], R.STRIDE)
        w = self.window
        _, self.place, out, sl, ack = accept_model.accept(self.ring, R.STRIDE, self.rl, self.seq(rbase), w,
                                                          self.img[rbase * MAXP:(rbase + w) * MAXP],
                                                          self.slot_len[rbase:rbase + w])
        self.img[rbase * MAXP:(rbase + w) * MAXP], self.slot_len[rbase:rbase + w] = out, sl
        return ack

    def build_acks(self, mode, rbase):
        w = self.window
        self.ack_seq, _, _ = build_acks(self.ring, R.STRIDE, self.rl, mode, self.seq(rbase), w, self.place,
                                        self.slot_len[rbase:rbase + w])
        return self.ack_seq.size

    def ingest_ring(self, aidx, mode, sbase, inflight):
        return self.ingest([R.ack_datagram(int(s)) for s in self.ack_seq[aidx]], mode, sbase, inflight)
