"""Models of the multi-connection sender (include/wtp_crc32.h: wtp_tx_ingest_acks_flows,
wtp_tx_advance_flows, wtp_tx_build_retransmit_var_flows).

Each is, by definition, the per-flow composition of the single-window model: retx_model.ingest
on the subsequence of a flow's datagrams against the flow's sub-array, advance_model.tx_advance
per sub-window, retxvar_model.retransmit_var per flow.  What is new is written directly from
the header: inflight_f, the bases, the r < nrec rule and the flow-major selection with its
max_sel cut (flow f gets the ring entries the flows before it left).  The caller's arrays are
never modified: copies are returned.

It also holds the fuzz corpus of the sender-flows tests and the whole-transfer driver whose
round is seven library calls whatever the number of connections; tests/test_txflows_model.py
runs both on the models and tests/test_gpu_txflows.py on the device calls, with the same seeds
and so the same decisions."""
import numpy as np

import ack_model as A
import advance_model as V
import flows_flush_model as FF
import flows_model as F
import oracle as O
import retx_model as R
import retxvar_model as RV

MAXP, M32, NOT_PLACED, EMPTY = 1456, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
STRIDE = MAXP + 16
SELECTIVE, CUMULATIVE, RETX_ALL = R.SELECTIVE, R.CUMULATIVE, R.RETX_ALL
NO_FLOW = 0xFFFFFFFF
INVALID_LEN = MAXP + 1  # what the model shows retransmit_var for a record at or above nrec


def inflight_of(rec0, rec_end, f, window):
    """The header's window rule: the slots of flow f that hold a record."""
    a, e = int(rec0[f]), int(rec_end[f])
    return min(window, e - a) if e > a else 0


def inflight_all(rec0, rec_end, nflows, window):
    """inflight_of for every flow at once, as int64."""
    a, e = np.asarray(rec0[:nflows], dtype=np.int64), np.asarray(rec_end[:nflows], dtype=np.int64)
    return np.where(e > a, np.minimum(window, e - a), 0)


def ingest_flows(ring, stride, recv_len, flow, mode, seq0, rec0, rec_end, nflows, window, acked, fast=False):
    """Returns (ok, hit, acked, flow_adv[nflows], flow_fresh[nflows]).  fast: the same without a
    loop over flows or datagrams, for batches of tens of thousands (tests/test_txflows_model.py
    holds it to the per-flow path, which is the definition)."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    flow = np.ascontiguousarray(flow, dtype=np.uint32)
    n = recv_len.size
    assert flow.size == n
    acked = np.array(acked, dtype=np.uint32, copy=True)
    ok = R.verify_limited(ring, stride, recv_len)[0]
    if fast:
        return (ok,) + _ingest_flows_fast(ring, stride, n, ok, flow, mode, seq0, rec0, rec_end, nflows, window, acked)
    hit = np.full(n, NOT_PLACED, dtype=np.uint32)
    adv, fresh = np.zeros(nflows, np.uint32), np.zeros(nflows, np.uint32)
    for f in range(nflows):
        idx = np.flatnonzero(flow == f)
        lo, inf = f * window, inflight_of(rec0, rec_end, f, window)
        sub = F.rows(ring, stride, idx) if idx.size else np.zeros(0, np.uint8)
        ok_f, hit[idx], acked[lo:lo + inf], (adv[f], fresh[f]) = R.ingest(sub, stride, recv_len[idx], mode, int(seq0[f]), inf,
                                                                           acked[lo:lo + inf])
        assert np.array_equal(ok_f, ok[idx])
    return ok, hit, acked, adv, fresh


def _ingest_flows_fast(ring, stride, n, ok, flow, mode, seq0, rec0, rec_end, nflows, window, acked):
    """A batch's marks are a set of global slots (selective) or a prefix per flow (cumulative),
    so the order of the datagrams only matters for hit, which is per datagram."""
    S = nflows * window
    infl = inflight_all(rec0, rec_end, nflows, window)
    types, seqs = R.headers(ring, stride, n)
    known = flow < nflows
    f = np.where(known, flow, 0).astype(np.int64)
    if nflows == 0:
        return np.full(n, NOT_PLACED, np.uint32), acked, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    d = (seqs.astype(np.int64) - np.asarray(seq0, dtype=np.int64)[f]) & M32
    counts = (ok != 0) & (types == 3) & known & ((d < infl[f]) if mode == SELECTIVE else ((d > 0) & (d <= infl[f])))
    hit = np.where(counts, d, NOT_PLACED).astype(np.uint32)
    slot = np.arange(S, dtype=np.int64) % max(window, 1)
    if mode == SELECTIVE:
        marks = np.unique(f[counts] * window + d[counts])
    else:
        top = np.zeros(nflows, np.int64)
        np.maximum.at(top, f[counts], d[counts])
        marks = np.flatnonzero(slot < np.repeat(top, window))
    new = marks[acked[marks] == 0]
    fresh = np.bincount(new // max(window, 1), minlength=nflows).astype(np.uint32)
    acked[new] = 1
    is_open = ((acked[:S] == 0) & (slot < np.repeat(infl, window))).reshape(nflows, window)
    adv = np.where(is_open.any(axis=1), is_open.argmax(axis=1), infl) if window else np.zeros(nflows, np.int64)
    return hit, acked, adv.astype(np.uint32), fresh


def advance_flows(acked, sent_ms, nflows, window, flow_adv, fill_ms, seq0, rec0, acked_next, sent_ms_next, seq0_next,
                  rec0_next, fast=False):
    """Returns (acked_next, sent_ms_next, seq0_next, rec0_next) after the call; the four base
    arrays may all be None (None comes back for the two outputs).  fast: advance_model's
    loop-free form per flow, for windows of 2^18 slots."""
    assert (seq0 is None) == (rec0 is None) == (seq0_next is None) == (rec0_next is None)
    ak = np.array(acked_next, dtype=np.uint32, copy=True)
    sm = np.array(sent_ms_next, dtype=np.uint32, copy=True)
    sq = None if seq0_next is None else np.array(seq0_next, dtype=np.uint32, copy=True)
    rc = None if rec0_next is None else np.array(rec0_next, dtype=np.uint32, copy=True)
    for f in range(nflows if window else 0):  # no slots: nothing is written
        lo, hi = f * window, (f + 1) * window
        a = min(int(flow_adv[f]), window)
        one = V.tx_advance_fast if fast else V.tx_advance
        ak[lo:hi], sm[lo:hi] = one(acked[lo:hi], sent_ms[lo:hi], window, a, fill_ms, ak[lo:hi], sm[lo:hi])
        if sq is not None:
            sq[f], rc[f] = (int(seq0[f]) + a) & M32, (int(rec0[f]) + a) & M32
    return ak, sm, sq, rc


def retransmit_var_flows(base, base_bytes, offsets, lengths, nrec, seq0, rec0, rec_end, nflows, window, acked, sent_ms,
                         now_ms, timeout_ms, flags, wire, wire_stride, max_sel, sel=None, wire_len=None, crc_out=None, fast=False):
    """Returns (wire, sel, wire_len, crc_out, sent_ms, (emitted, due)) after the call; `sel`,
    `wire_len`, `crc_out`: the prior contents of the optional outputs, None for a NULL pointer
    (None comes back).  sel[k] is the global slot f * window + s.  fast: the same with one
    selection over all global slots and a loop over the emitted datagrams only, for states of
    2^20 slots and rings of 10^5 entries (tests/test_txflows_model.py holds it to the per-flow
    path, which is the definition)."""
    wire = np.array(wire, dtype=np.uint8, copy=True)
    sent = np.array(sent_ms, dtype=np.uint32, copy=True)
    outs = [None if a is None else np.array(a, dtype=np.uint32, copy=True) for a in (sel, wire_len, crc_out)]
    if fast:
        return _retransmit_var_flows_fast(base, base_bytes, offsets, lengths, nrec, seq0, rec0, rec_end, nflows, window, acked,
                                          sent, now_ms, timeout_ms, flags, wire, wire_stride, max_sel, outs)
    emitted = due = 0
    for f in range(nflows):
        lo, inf = f * window, inflight_of(rec0, rec_end, f, window)
        recs = [(int(rec0[f]) + s) & M32 for s in range(inf)]
        offs_f = np.array([int(offsets[r]) if r < nrec else 0 for r in recs], dtype=np.uint64)
        lens_f = np.array([int(lengths[r]) if r < nrec else INVALID_LEN for r in recs], dtype=np.uint32)
        room, k0 = max_sel - emitted, emitted  # the cut: the flows before this one come first
        z = lambda: np.zeros(room, np.uint32)  # noqa: E731
        w_f, sel_f, wl_f, crc_f, sent[lo:lo + inf], (e, d) = RV.retransmit_var(
            base, base_bytes, offs_f, lens_f, int(seq0[f]), inf, acked[lo:lo + inf], sent[lo:lo + inf], now_ms, timeout_ms,
            flags, wire[k0 * wire_stride:], wire_stride, room, z(), z(), z())
        wire[k0 * wire_stride:] = w_f
        for a, v in zip(outs, (sel_f + np.uint32(lo), wl_f, crc_f)):
            if a is not None:
                a[k0:k0 + e] = v[:e]
        emitted, due = emitted + e, due + d
    return (wire, *outs, sent, (emitted, due))


def _retransmit_var_flows_fast(base, base_bytes, offsets, lengths, nrec, seq0, rec0, rec_end, nflows, window, acked, sent,
                               now_ms, timeout_ms, flags, wire, wire_stride, max_sel, outs):
    """`wire`, `sent` and `outs` are the copies the caller made, written in place.  CRCs from
    oracle.batch_var, the header words laid out as oracle.build_datagram lays them out."""
    S = nflows * window
    base = np.asarray(base, dtype=np.uint8)
    g = np.arange(S, dtype=np.int64)
    infl = inflight_all(rec0, rec_end, nflows, window)
    age = (now_ms - sent[:S].astype(np.int64)) & M32
    is_due = ((g % max(window, 1)) < np.repeat(infl, window)) & (np.asarray(acked)[:S] == 0) & \
        (bool(flags & RETX_ALL) | (age > timeout_ms))
    picked = np.flatnonzero(is_due)
    due, picked = int(picked.size), picked[:max_sel]
    e = int(picked.size)
    sent[picked] = now_ms & M32
    f, s = picked // max(window, 1), picked % max(window, 1)
    rec = (np.asarray(rec0, dtype=np.int64)[f] + s) & M32
    seq = (np.asarray(seq0, dtype=np.int64)[f] + s) & M32
    there = rec < nrec
    at = np.where(there, rec, 0)
    tab_o, tab_l = np.asarray(offsets, dtype=np.uint64), np.asarray(lengths, dtype=np.uint32)
    if nrec == 0:  # no record is looked up
        tab_o, tab_l = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    offs = np.where(there, tab_o[at], 0).astype(np.uint64)
    lens = np.where(there, tab_l[at], INVALID_LEN).astype(np.int64)
    valid = (lens <= MAXP) & (offs <= np.uint64(base_bytes))
    valid[valid] = lens[valid] <= base_bytes - offs[valid].astype(np.int64)
    v = np.flatnonzero(valid)
    crc, wl = np.zeros(e, np.uint32), np.zeros(e, np.uint32)
    crc[v] = O.batch_var(base, offs[v], lens[v].astype(np.uint32))
    wl[v] = 16 + lens[v]
    head = np.stack([np.full(v.size, 2), seq[v], lens[v], crc[v]], axis=1).astype(">u4").view(np.uint8).reshape(v.size, 16)
    assert wire.size >= e * wire_stride
    slots = wire[:e * wire_stride].reshape(e, wire_stride)
    slots[v, :16] = head
    src = offs[v].astype(np.int64)
    for n in np.unique(lens[v]).tolist():  # the payloads, one length at a time, 4096 datagrams at a time
        same = np.flatnonzero(lens[v] == n)
        for a in range(0, same.size if n else 0, 4096):
            part = same[a:a + 4096]
            slots[v[part], 16:16 + n] = base[src[part][:, None] + np.arange(n)]
    for a, x in zip(outs, (picked, wl, crc)):
        if a is not None:
            a[:e] = x
    return (wire, *outs, sent, (e, due))


# ---- the corpus of the randomised differential test -------------------------------------------
FUZZ_SEEDS = range(12)
FUZZ_BASE = 0x7F10E5
FUZZ_CALLS = 2
ROLES = ("short", "empty", "past")  # inflight_f < window; rec0 == rec_end; rec0 > rec_end
ACK_KINDS = ("ack", "dup", "corrupt", "nonack", "payload", "runt", "long", "noflow_n", "noflow_m", "a0", "a_in", "a_in1")
REC_KINDS = ("len0", "len1", "len17", "len1456", "len1457", "off_past", "last_byte", "past_nrec", "plain")
FUZZ_STRIDES = (20, 24, 64)
FUZZ_TIMEOUT = 500


def fuzz_case(seed):
    """The fixed part of one seed: a dict with nflows (2 .. 5), window (3 .. 90), stride, the
    initial seq0 / rec0, the constant rec_end, every flow's role and the record table (base,
    base_bytes, offs, lens with nrec entries, rec_kind for every index the flows name).  Odd
    seeds put flow 0's seq0 within 3 of the 2^32 wrap; seeds divisible by 3 give flows 0 and 1
    the same seq0.  The last flow is "short" (fewer records than slots) and its last records
    lie at or above nrec; the flows before it take "empty" and "past" as far as there are
    flows, flow 0 always has more records than slots."""
    rng = np.random.default_rng(FUZZ_BASE + seed)
    nflows, window = int(rng.integers(2, 6)), int(rng.integers(3, 91))
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    if seed % 2:
        seq0[0] = (1 << 32) - 1 - int(rng.integers(3))
    if seed % 3 == 0:
        seq0[1] = seq0[0]
    roles = ["full"] * nflows
    for j, role in enumerate(("short",) + (("empty", "past") if seed % 2 else ("past", "empty"))):
        if j < nflows - 1:
            roles[nflows - 1 - j] = role
    rec0, rec_end = np.zeros(nflows, np.uint32), np.zeros(nflows, np.uint32)
    at, tail_recs = 0, []
    for f in sorted(range(nflows), key=lambda x: roles[x] == "short"):  # the short flow's records come last
        count = {"full": window + int(rng.integers(1, window + 1)), "short": int(rng.integers(1, window)), "empty": 0,
                 "past": 0}[roles[f]]
        rec0[f], rec_end[f] = at + (int(rng.integers(1, 6)) if roles[f] == "past" else 0), at + count
        if roles[f] == "full":
            tail_recs += [at + 1, at + window + 1]  # in the first window, and in any window two or more slots on
        at += count
    total_rec = at
    nrec = total_rec - min(2, int(rec_end[nflows - 1]) - int(rec0[nflows - 1]))
    lens, kinds = np.zeros(nrec, np.uint32), []
    planted = (("len0", 0), ("len1", 1), ("len17", 17), ("len1456", MAXP), ("len1457", MAXP + 1), ("off_past", 3))
    for r in range(nrec):
        if r in tail_recs:
            kind, ln = "last_byte", int(rng.integers(1, 40))
        elif rng.random() < 0.45:
            kind, ln = planted[int(rng.integers(len(planted)))]
        else:
            kind, ln = "plain", int(rng.integers(2, 200) if rng.random() < 0.8 else rng.integers(200, MAXP))
        kinds.append(kind)
        lens[r] = ln
    packed = np.where(np.array([k in ("off_past", "last_byte") for k in kinds]), 0, lens).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(packed)[:-1]]).astype(np.uint64)
    base_bytes = int(packed.sum()) + 40
    for r, k in enumerate(kinds):
        if k == "off_past":
            offs[r] = base_bytes + 1 + r % 5
        elif k == "last_byte":
            offs[r] = base_bytes - int(lens[r])  # these overlap each other: records may
    base = O.synth_fill_np(base_bytes, start_byte=seed + 1)
    return dict(rng=rng, nflows=nflows, window=window, stride=FUZZ_STRIDES[seed % len(FUZZ_STRIDES)], seq0=seq0, rec0=rec0,
                rec_end=rec_end, roles=roles, nrec=nrec, base=base, base_bytes=base_bytes, offs=offs, lens=lens,
                rec_kind=kinds + ["past_nrec"] * (total_rec - nrec), wire_stride=STRIDE + 16 * (seed % 2))


def _ack(seq, ptype=3, payload=b"", damage=False):
    d = bytearray(R.ack_datagram(seq, ptype, O.crc32(payload) if payload else 0, payload))
    if damage:
        d[12 + (len(d) - 12) // 2] ^= 0x10  # the checksum, or a payload byte
    return bytes(d)


def fuzz_acks(rng, mode, seq0, infl, nflows, stride, everything):
    """(ring, recv_len, flow, kinds) of one ACK batch: for every flow a few ACKs for slots of
    its window (cumulative: low values of a, so that windows stay partly open), and the kinds of
    ACK_KINDS: all of them for the flow `everything`, each with probability 1/3 for the others.
    Every flow's own order is kept by the interleaving."""
    lists = []
    for f in range(nflows):
        s0, inf = int(seq0[f]), infl[f]
        some = [int(rng.integers(0, max(inf // 2, 1))) for _ in range(int(rng.integers(1, 4 + inf // 3)))]
        some += [t for t in (0, 1) if rng.random() < 0.6]
        dg = [("ack", _ack(s0 + t + (mode == CUMULATIVE)), None) for t in some]
        want = lambda: f == everything or rng.random() < 1 / 3  # noqa: E731
        if want():
            dg.append(("dup", dg[int(rng.integers(len(dg)))][1], None))
        if want():
            dg.append(("corrupt", _ack(s0 + 1, damage=True), None))
        if want():
            dg.append(("nonack", _ack(s0 + 1, ptype=int(rng.integers(0, 3))), None))
        if want():
            p = O.synth_fill_np(int(rng.integers(1, stride - 15)), start_byte=f).tobytes()
            dg.append(("payload", _ack(s0 + min(2, inf), payload=p), None))
        if want():
            dg.append(("runt", _ack(s0 + 1), int(rng.integers(0, 16))))
        if want():
            dg.append(("long", _ack(s0 + 1), stride + int(rng.integers(1, 6))))
        for kind, a in (("a0", 0), ("a_in", inf), ("a_in1", inf + 1)):
            if f == everything or rng.random() < 0.15:
                dg.append((kind, _ack(s0 + a), None))
        order = rng.permutation(len(dg))
        lists.append([(f,) + dg[i] for i in order])
    s0 = int(seq0[0])
    lists.append([(nflows, "noflow_n", _ack(s0), None), (NO_FLOW, "noflow_m", _ack(s0 + 1), None),
                  (nflows, "noflow_n", _ack(s0 + 1, damage=True), None)])
    labels, within = F.interleave(rng, [len(x) for x in lists])
    n = labels.size
    ring = rng.integers(0, 256, n * stride, dtype=np.uint8)
    rl, flow, kinds = np.zeros(n, np.uint32), np.zeros(n, np.uint32), []
    for i, (k, w) in enumerate(zip(labels, within)):
        f, kind, d, length = lists[k][w]
        cut = min(len(d), stride)
        ring[i * stride:i * stride + cut] = np.frombuffer(d[:cut], dtype=np.uint8)
        rl[i], flow[i] = (len(d) if length is None else length), f
        kinds.append(kind)
    return ring, rl, flow, kinds


def fuzz_calls(seed, mode):
    """(calls, case): FUZZ_CALLS successive rounds on one state.  A round is ingest (state
    `acked0`) -> advance into buffers that hold 0x77777777 -> build on the slid state, with
    timers in selective mode and WTP_RETX_ALL in cumulative mode; the first round's ring holds
    every slot, the second is cut at a third of the slots.  Every call's inputs and the models'
    results are in the round's dict."""
    case = fuzz_case(seed)
    rng, nf, w = case["rng"], case["nflows"], case["window"]
    S = nf * w
    seq0, rec0, rec_end = case["seq0"].copy(), case["rec0"].copy(), case["rec_end"]
    now = 0xFFFFFF00 if seed % 2 else 100000 + seed
    acked = (rng.random(S) < 0.3).astype(np.uint32) * rng.choice(np.array([1, 1, 7], np.uint32), S)
    sent = ((now - rng.integers(0, 2 * FUZZ_TIMEOUT, S)) & M32).astype(np.uint32)
    calls = []
    for c in range(FUZZ_CALLS):
        infl = [inflight_of(rec0, rec_end, f, w) for f in range(nf)]
        ring, rl, flow, kinds = fuzz_acks(rng, mode, seq0, infl, nf, case["stride"], (seed + c) % nf)
        ing = ingest_flows(ring, case["stride"], rl, flow, mode, seq0, rec0, rec_end, nf, w, acked)
        now = (now + 300) & M32
        fill = (now - FUZZ_TIMEOUT - 1) & M32
        junk = np.full(S, 0x77777777, np.uint32)
        adv = advance_flows(ing[2], sent, nf, w, ing[3], fill, seq0, rec0, junk, junk, junk[:nf], junk[:nf])
        max_sel = S if c == 0 else S // 3 + 1
        flags = RETX_ALL if mode == CUMULATIVE else 0
        prior = (np.full(max_sel * case["wire_stride"], 0xA5, np.uint8), np.full(max_sel, 0x5E1, np.uint32),
                 np.full(max_sel, 0x1E4, np.uint32), np.full(max_sel, 0xC4C, np.uint32))
        bld = retransmit_var_flows(case["base"], case["base_bytes"], case["offs"], case["lens"], case["nrec"], adv[2], adv[3],
                                   rec_end, nf, w, adv[0], adv[1], now, FUZZ_TIMEOUT, flags, prior[0], case["wire_stride"],
                                   max_sel, *prior[1:])
        calls.append(dict(seq0=seq0, rec0=rec0, infl=infl, acked0=acked, sent0=sent, ring=ring, rl=rl, flow=flow, kinds=kinds,
                          ingest=ing, fill=fill, advance=adv, now=now, flags=flags, max_sel=max_sel, build=bld))
        acked, sent, seq0, rec0 = adv[0], bld[4], adv[2], adv[3]
    return calls, case


# ---- a transfer of several connections with seven calls per round ------------------------------
# flows_model's transfer (XFER_FLOWS senders of XFER_RECORDS records, window XFER_WINDOW, loss
# and duplication 0.15, the same records and sequence numbers) with both ends batched.  All
# senders' records sit in one table, flow f's at indices [f * XFER_RECORDS, (f + 1) * XFER_RECORDS).
# A round is, in stream order,
#   build_flows -> channel -> accept_flows -> acks_flows -> deliver_flows -> rx_advance_flows ->
#   channel -> ingest_flows -> tx_advance_flows
# with every base (the receiver's seq0, the sender's seq0 and rec0) moved by the advance calls
# alone.  The channels draw from the generator in flows_model.transfer's order, so the rounds
# are that loop's rounds.
def xfer_table(nflows=F.XFER_FLOWS):
    """(base, base_bytes, offs, lens, rec0, rec_end, per-flow records) of the one table."""
    recs = [F.xfer_records(f) for f in range(nflows)]
    starts = np.concatenate([[0], np.cumsum([r[2] for r in recs])]).astype(np.uint64)
    base = np.concatenate([r[3] for r in recs])
    offs = np.concatenate([r[1] + starts[f] for f, r in enumerate(recs)]).astype(np.uint64)
    lens = np.concatenate([r[0] for r in recs]).astype(np.uint32)
    rec0 = (np.arange(nflows) * F.XFER_RECORDS).astype(np.uint32)
    return base, int(base.size), offs, lens, rec0, rec0 + np.uint32(F.XFER_RECORDS), recs


def transfer(end, mode, nflows=F.XFER_FLOWS, nrec=F.XFER_RECORDS, window=F.XFER_WINDOW, loss=F.XFER_LOSS, dup=F.XFER_DUP,
             seed=F.XFER_SEED, max_rounds=F.XFER_MAX_ROUNDS):
    """Drives `end` until every sender's window has passed its last record:
      end.build(now, timeout) -> sel: the emitted global slots of all flows, ring entry k = sel[k]
      end.receive(gidx, flow, mode) -> (flow_ack, src): accept_flows + acks_flows over ring
        entries gidx (arrival order), then deliver_flows + rx_advance_flows; src = the datagram
        index of every ACK
      end.flushed() -> [(k, bytes)] per flow of that flush
      end.ingest(aidx, aflow, mode, fill_ms) -> [adv] per flow: ingest_flows over ACK ring
        entries aidx with their flows, then tx_advance_flows
    Returns (log, stats) as flows_model.transfer does."""
    rng = np.random.default_rng(seed)
    sbase, rbase = [0] * nflows, [0] * nflows
    now = F.XFER_NOW0
    log, stats = [], np.zeros((nflows, 3), dtype=np.int64)
    while any(s < nrec for s in sbase):
        if len(log) == max_rounds:
            raise AssertionError(f"transfer not finished after {max_rounds} rounds (sender bases {sbase} of {nrec})")
        sel = [int(g) for g in end.build(now, F.XFER_TIMEOUT)]
        assert sel == sorted(sel)  # flow-major, then slot-major
        sent, lists = [], []
        for f in range(nflows):
            ring_at = [k for k, g in enumerate(sel) if g // window == f]
            mine = [sel[k] - f * window for k in ring_at]
            assert all(s < min(window, nrec - sbase[f]) for s in mine)
            m = len(mine)
            keep, twice = rng.random(m) >= loss, rng.random(m) < dup
            ks = np.array([k for k in range(m) if keep[k] for _ in range(2 if twice[k] else 1)], dtype=np.int64)
            ks = ks[rng.permutation(ks.size)]
            arrived = [mine[k] for k in ks]
            stats[f] += (m - int(keep.sum()), int((keep & twice).sum()), sum(1 for a, b in zip(arrived, arrived[1:]) if b < a))
            sent.append(mine)
            lists.append(np.array([ring_at[k] for k in ks], dtype=np.int64))
        labels, within = F.interleave(rng, [x.size for x in lists])
        gidx = np.array([lists[f][w] for f, w in zip(labels, within)], dtype=np.int64)
        now = (now + 1) & M32
        flow_ack, src = end.receive(gidx, labels.astype(np.uint32), mode)
        flushed = [(int(k), int(b)) for k, b in end.flushed()]
        for f in range(nflows):
            assert (int(flow_ack[f]) - F.XFER_SEQ[f] - rbase[f]) & M32 == flushed[f][0]  # deliver's run is the flow's ACK
            rbase[f] += flushed[f][0]
        nack = len(src)
        aidx = rng.permutation(nack)
        aidx = aidx[rng.random(nack)[aidx] >= loss]
        # flows_model.transfer hands sender f its ACKs in arrival order; here they stay one batch
        advs = [int(a) for a in end.ingest(aidx, labels[np.asarray(src, dtype=np.int64)[aidx]].astype(np.uint32), mode,
                                           (now - F.XFER_TIMEOUT - 1) & M32)]
        for f in range(nflows):
            sbase[f] += advs[f]
            assert sbase[f] <= rbase[f]
        log.append((sent, gidx.tolist(), [int(a) for a in flow_ack], [int(s) for s in src], flushed, advs))
    return log, stats


class ModelEnd:
    """Both ends of `transfer` on the models: the three models above for all senders, and
    flows_model.accept_flows / build_acks_flows and flows_flush_model.deliver_flows /
    advance_flows for the receiver.  Every base is moved by the advance models alone."""

    def __init__(self, nflows=F.XFER_FLOWS, window=F.XFER_WINDOW):
        self.nflows, self.window = nflows, window
        S = nflows * window
        self.base, self.base_bytes, self.offs, self.lens, rec0, self.rec_end, self.rec = xfer_table(nflows)
        seq0 = np.array(F.XFER_SEQ[:nflows], dtype=np.uint32)
        self.tseq, self.trec = [seq0.copy(), np.zeros(nflows, np.uint32)], [rec0, np.zeros(nflows, np.uint32)]
        self.acked = [np.zeros(S, np.uint32) for _ in range(2)]
        self.sent = [np.full(S, (F.XFER_NOW0 - F.XFER_TIMEOUT - 1) & M32, np.uint32) for _ in range(2)]
        self.rseq = [seq0.copy(), np.zeros(nflows, np.uint32)]
        self.img = [np.full(S * MAXP, 0x3C, np.uint8) for _ in range(2)]
        self.sl = [np.full(S, EMPTY, np.uint32) for _ in range(2)]
        self.stream = [np.full(r[2], 0xA5, np.uint8) for r in self.rec]
        self.off = [0] * nflows
        self.offs_got, self.lens_got = [[] for _ in range(nflows)], [[] for _ in range(nflows)]

    def build(self, now, timeout):
        S = self.nflows * self.window
        self.wire, sel, self.wl, _, self.sent[0], counts = retransmit_var_flows(
            self.base, self.base_bytes, self.offs, self.lens, self.lens.size, self.tseq[0], self.trec[0], self.rec_end,
            self.nflows, self.window, self.acked[0], self.sent[0], now, timeout, 0, np.full(S * STRIDE, 0xA5, np.uint8), STRIDE,
            S, np.zeros(S, np.uint32), np.zeros(S, np.uint32))
        assert counts[0] == counts[1]  # the ring holds every slot
        return sel[:counts[0]]

    def receive(self, gidx, flow, mode):
        w, nf = self.window, self.nflows
        ring = F.rows(self.wire, STRIDE, gidx) if gidx.size else np.zeros(0, np.uint8)
        rl = self.wl[gidx]
        ok, _, self.img[0], self.sl[0], ack = F.accept_flows(ring, STRIDE, rl, flow, self.rseq[0], nf, w, self.img[0], self.sl[0])
        assert ok.all()
        self.ack_seq, src, (emitted, total) = F.build_acks_flows(ring, STRIDE, rl, flow, mode, self.rseq[0], nf, w, ok, ack)
        assert emitted == total == gidx.size  # every arrival is inside its flow's window or below it
        cap = nf * w * MAXP
        stream, offs, lens, adv, info, counts = FF.deliver_flows(self.img[0], self.sl[0], nf, w, w, np.full(cap, 0xA5, np.uint8),
                                                                 cap, 0, np.zeros(nf * w, np.uint64), np.zeros(nf * w, np.uint32))
        assert counts[0] == counts[1] and counts[2] == counts[3]  # the round stream holds every run
        self.img[1], self.sl[1], self.rseq[1] = FF.advance_flows(self.img[0], self.sl[0], nf, w, adv, self.rseq[0], self.img[1],
                                                                 self.sl[1], self.rseq[1])
        for x in (self.img, self.sl, self.rseq):
            x.reverse()
        self.last = []
        for f in range(nf):
            k, (_, R_, B, nbytes) = int(adv[f]), (int(v) for v in info[f])
            self.stream[f][self.off[f]:self.off[f] + nbytes] = stream[B:B + nbytes]
            self.offs_got[f] += (offs[R_:R_ + k].astype(np.int64) - B + self.off[f]).tolist()
            self.lens_got[f] += lens[R_:R_ + k].tolist()
            self.off[f] += nbytes
            self.last.append((k, nbytes))
        return ack, src

    def flushed(self):
        return self.last

    def ingest(self, aidx, aflow, mode, fill_ms):
        nf, w = self.nflows, self.window
        acks = A.ack_bytes(self.ack_seq[aidx]).reshape(-1) if aidx.size else np.zeros(0, np.uint8)
        ok, _, self.acked[0], adv, _ = ingest_flows(acks, 16, np.full(aidx.size, 16, np.uint32), aflow, mode, self.tseq[0],
                                                    self.trec[0], self.rec_end, nf, w, self.acked[0])
        assert ok.all()
        self.acked[1], self.sent[1], self.tseq[1], self.trec[1] = advance_flows(
            self.acked[0], self.sent[0], nf, w, adv, fill_ms, self.tseq[0], self.trec[0], self.acked[1], self.sent[1],
            self.tseq[1], self.trec[1])
        for x in (self.acked, self.sent, self.tseq, self.trec):
            x.reverse()
        return adv.tolist()
