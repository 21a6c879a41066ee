"""The inputs of the length, phase, threshold and scale tests of the ten multi-connection calls
(tests/test_gpu_txflows.py, test_gpu_flows.py, test_gpu_flows_flush.py, sections "edges of the
copies").  Nothing here needs a device: tests/test_flows_cases.py runs the model halves of
every case on the CPU, at the GPU tests' shapes where the models are quick and scaled down
(the builders' size arguments) where they are not, and asserts there what the GPU tests rely on: which lengths and
source phases occur, on which side of a threshold a count lies, that flow_fresh differs from
the raw hit count, how many slots are due."""
import numpy as np

import buildvar_model as B
import oracle as O
import retx_model as R
import txflows_model as T

MAXP, STRIDE, M32, EMPTY = T.MAXP, T.STRIDE, T.M32, T.EMPTY
NOW, TIMEOUT = 10_000, 500
OLD, FRESH = NOW - TIMEOUT - 1, NOW - TIMEOUT  # a timer that is due, and one that is just not
CLAIM = 0x80000005

# wtp_tx_flows.hip: the grid of k_txf_emit is one wave per ring entry, m = min(S, max_sel) of
# them in workgroups of kTfWaves = 4, capped at kTfMaxBlocks = 1280 workgroups = 5120 waves; a
# wave round is G = 2^g datagrams, the smallest power of two with G * waves >= the emitted
# count, g <= 6.  A grid below the cap has waves >= m >= count, so G = 1.  With the capped grid
# G changes at count = 5120 * 2^j: 5120 | 5121 (1 -> 2), 10 240 | 10 241 (2 -> 4), 20 480 |
# 20 481 (4 -> 8), 40 960 | 40 961 (8 -> 16), 81 920 | 81 921 (16 -> 32), 163 840 | 163 841
# (32 -> 64); above 64 * 5120 = 327 680 a wave takes a second round.
CAP_WAVES = 1280 * 4
THRESHOLDS = [CAP_WAVES << j for j in range(6)]
TWO_ROUNDS = 64 * CAP_WAVES
SELECT_BLOCK = 1024  # kTxfBlock: slots per block of k_txf_count / k_txf_select, one block count per lane
MAX_SLOTS = 1 << 20  # WTP_TX_MAX_FLOW_SLOTS


def round_log2(count, max_sel, slots):
    """g of k_txf_emit for `count` emitted datagrams: the kernel's own rule, from the launch's."""
    m = min(slots, max_sel)
    waves = min((m + 3) // 4, 1280) * 4
    g = 0
    while g < 6 and (waves << g) < count:
        g += 1
    return g


def state(n, due, rng=None, inflight=None):
    """(acked, sent_ms) of n slots of which the slots `due` (indices or a bool mask) are due: the
    others are ACKed (with an old timer) or un-ACKed with a timer that is just not due.  Slots
    where `inflight` (a mask) is False look due, so only the window rule keeps them out."""
    mask = np.zeros(n, bool)
    mask[due] = True
    rng = rng or np.random.default_rng(n)
    waiting = ~mask & (rng.random(n) < 0.3)
    acked = (~mask & ~waiting).astype(np.uint32) * rng.integers(1, 3, n).astype(np.uint32)
    sent = np.where(waiting, FRESH, OLD).astype(np.uint32)
    if inflight is not None:
        acked[~inflight], sent[~inflight] = 0, OLD
    return acked, sent


def inflight_mask(rec0, rec_end, nflows, window):
    return (np.arange(nflows * window) % window) < np.repeat(T.inflight_all(rec0, rec_end, nflows, window), window)


# ---- 1a. every length through the rebuild -----------------------------------------------------
PATTERNS = ("none", "one", "tenth", "half", "all")
EVERY_FLOWS, EVERY_WINDOW = 5, 300


def every_length_case(pattern, top=MAXP):
    """Records of every length 0 .. top once, permuted and packed, over 5 flows of
    ceil-sized windows (300 for top = 1456): record r is global slot r, so the last flow has
    fewer records than slots; flow 2's sequence numbers wrap.  Returns a dict with the record
    table, the bases, the state, the due mask over the records and the rings to run."""
    n = top + 1
    nflows, window = EVERY_FLOWS, -(-(n + 43) // EVERY_FLOWS)
    S = nflows * window
    rng = np.random.default_rng(len(pattern) * 131 + top)
    lens = rng.permutation(n).astype(np.uint32)
    due = {"none": np.zeros(n, bool), "one": np.arange(n) == (777 if n > 777 else n // 2), "tenth": rng.random(n) < 0.1,
           "half": rng.random(n) < 0.5, "all": np.ones(n, bool)}[pattern]
    rec0 = (np.arange(nflows) * window).astype(np.uint32)
    rec_end = np.minimum(rec0 + window, n).astype(np.uint32)
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    seq0[2] = 0xFFFFFF00 if window > 256 else M32 - 3
    mask = np.zeros(S, bool)
    mask[:n] = due
    acked, sent = state(S, mask, rng, inflight_mask(rec0, rec_end, nflows, window))
    d = int(due.sum())
    return dict(n=n, nflows=nflows, window=window, S=S, lens=lens, offs=B.packed_offsets(lens),
                base=O.synth_fill_np(max(int(lens.sum()), 1), start_byte=len(pattern)), seq0=seq0, rec0=rec0, rec_end=rec_end,
                acked=acked, sent=sent, due=due, d=d, rings=sorted({d, max(d - 1, 0), d + 70, S}))


# ---- 1b. each side of every round-size change ---------------------------------------------------
def count_case(count, rec_len, nflows=3):
    """`count` due slots spread evenly over `nflows` windows that together hold count + 9 slots
    or a few more, the window no multiple of 64; record r is global slot r, rec_len bytes each."""
    window = -(-(count + 9) // nflows)
    window += window % 64 == 0
    S = nflows * window
    due = np.round(np.linspace(0, S - 1, count)).astype(np.int64)
    assert np.unique(due).size == count and window % 64 and S >= count + 9
    acked, sent = state(S, due)
    lens = np.full(S, rec_len, np.uint32)
    rec0 = (np.arange(nflows) * window).astype(np.uint32)
    seq0 = np.array([M32 - count, 7, 0x80000000][:nflows], np.uint32)
    return dict(nflows=nflows, window=window, S=S, due=due, acked=acked, sent=sent, lens=lens, offs=B.packed_offsets(lens),
                base=O.synth_fill_np(max(int(lens.sum()), 1), start_byte=count & 0xFF), seq0=seq0, rec0=rec0,
                rec_end=rec0 + np.uint32(window))


def many_short_records(n=400_000, nflows=3):
    """n records of at most 8 bytes over nflows windows with two slots to spare, all due."""
    window = -(-(n + 2) // nflows)
    lens = ((np.arange(n) * 5 + (np.arange(n) >> 8)) % 9).astype(np.uint32)
    rec0 = (np.arange(nflows) * window).astype(np.uint32)
    rec_end = np.minimum(rec0 + window, n).astype(np.uint32)
    seq0 = np.array([0xFFFF0000, 5, M32 - 70_000][:nflows], np.uint32)
    return dict(n=n, nflows=nflows, window=window, S=nflows * window, lens=lens, offs=B.packed_offsets(lens),
                base=O.synth_fill_np(int(lens.sum()), start_byte=4), seq0=seq0, rec0=rec0, rec_end=rec_end)


# ---- 1c. selection at scale ---------------------------------------------------------------------
SCALE_SHAPES = ((4, 262_144), (4096, 256), (1, 65_537), (65_537, 1))
NAMED_SLOTS = (0, 63, 64, 1023, 1024, 65_535, 65_536, MAX_SLOTS - 1)


def scale_case(nflows, window, extra=1500):
    """A sparse due set over S = nflows * window slots: the named global slots below S, the
    first and the last slot of flows 0, 1, the middle one and the last, and `extra` random ones.
    Record r is global slot r, at most 8 bytes; every 97th flow (and flow 1 of a few) has fewer
    records than slots, and what lies behind its records looks due."""
    S = nflows * window
    rng = np.random.default_rng(S + nflows)
    rec0 = (np.arange(nflows, dtype=np.int64) * window).astype(np.uint32)
    count = np.full(nflows, window, np.int64)
    if window > 1:
        count[1::97] = window - window // 3
    rec_end = (rec0 + count).astype(np.uint32)
    inside = inflight_mask(rec0, rec_end, nflows, window)
    flows = sorted({0, min(1, nflows - 1), nflows // 2, nflows - 1})
    named = [g for g in NAMED_SLOTS if g < S] + [f * window for f in flows] + [(f + 1) * window - 1 for f in flows]
    due = np.zeros(S, bool)
    due[rng.integers(0, S, extra)] = True
    due[named] = True
    due &= inside
    acked, sent = state(S, due, rng, inside)
    g = np.arange(S)
    lens = ((g * 5 + (g >> 8)) % 9).astype(np.uint32)
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    seq0[0] = M32 - 1
    return dict(nflows=nflows, window=window, S=S, named=[g for g in named if inside[g]], due=due, d=int(due.sum()), acked=acked,
                sent=sent, lens=lens, offs=B.packed_offsets(lens), base=O.synth_fill_np(int(lens.sum()), start_byte=7),
                seq0=seq0, rec0=rec0, rec_end=rec_end)


def cut_inside_a_flow(sel, emitted, window):
    """A ring size in the middle of the selection that ends inside a flow (where a flow has
    more than three slots)."""
    return next(k for k in range(emitted // 2, emitted) if window < 4 or int(sel[k]) % window not in (0, window - 1))


# ---- 1d. timers ---------------------------------------------------------------------------------
TIMER_CASES = ((5, 500), (5, 0), (5, M32), (NOW, 500), (M32, 500), (0, 1), (3, M32 - 1))  # (now, timeout)
AGES = (-1, 0, 1, -3)  # relative to the timeout; and a timer three ticks in the future


def timer_case(now, timeout, nflows=3, window=40):
    """Every flow holds, un-ACKed and ACKed, timers of age timeout - 1, timeout, timeout + 1 (all
    mod 2^32) and one that lies 3 ms in the future (age 2^32 - 3).  Returns the state and the
    slots that are due without WTP_RETX_ALL and with it, from the rule itself."""
    S = nflows * window
    rng = np.random.default_rng(now % 1000 + timeout % 1000)
    kind = (np.arange(S) + np.arange(S) // window) % 4
    age = np.where(kind == 3, M32 - 2, (timeout + np.array(AGES)[kind]) & M32).astype(np.int64)
    sent = ((now - age) & M32).astype(np.uint32)
    acked = (rng.random(S) < 0.3).astype(np.uint32) * 5
    lens = rng.integers(0, 200, S).astype(np.uint32)
    rec0 = (np.arange(nflows) * window).astype(np.uint32)
    rec_end = rec0 + np.uint32(window)
    rec_end[nflows - 1] -= 7
    inside = inflight_mask(rec0, rec_end, nflows, window)
    due = inside & (acked == 0) & (age > timeout)  # ages are below 2^32 by construction
    return dict(nflows=nflows, window=window, S=S, acked=acked, sent=sent, lens=lens, offs=B.packed_offsets(lens),
                base=O.synth_fill_np(int(lens.sum()), start_byte=3), seq0=np.array([M32, 0, 9][:nflows], np.uint32), rec0=rec0,
                rec_end=rec_end, due=np.flatnonzero(due), all=np.flatnonzero(inside & (acked == 0)))


# ---- 2a. an ACK batch over many workgroups --------------------------------------------------------
def ack_batch(mode, nflows=300, window=100, general=30_000, hot=20_000, seed=0xACC):
    """(ring, recv_len, flow, seq0, rec0, rec_end, acked0) with stride 16.  `general` ACKs for
    uniformly drawn slots of uniformly drawn flows (cumulative: a value up to a per-flow top, so
    that windows stay partly open); `hot` ACKs for three slots of flow 3; `hot` ACKs of one value
    for flow 5; and, shuffled in with them, damaged checksums, the other packet types, flows at
    and above nflows, the sequence numbers one below and one past every window.  Flow 0's seq0
    is 0xFFFFFFFF; every seventh flow has fewer records than slots and every eleventh none.
    Half of acked0 is set, so a flow's fresh count is below its hit count."""
    rng = np.random.default_rng(seed + mode)
    S = nflows * window
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    seq0[0] = M32
    rec0 = (np.arange(nflows) * 2 * window).astype(np.uint32)
    k = np.arange(nflows)
    count = np.where(k % 11 == 10, 0, np.where(k % 7 == 6, max(window // 2, 1), 2 * window))
    rec_end = (rec0 + count).astype(np.uint32)
    infl = T.inflight_all(rec0, rec_end, nflows, window)
    first = 1 if mode == T.CUMULATIVE else 0  # the lowest value that counts
    f = rng.integers(0, nflows, general)
    top = rng.integers(1, window + 1, nflows)
    d = (rng.random(general) * (top[f] if mode == T.CUMULATIVE else np.maximum(infl[f], 1))).astype(np.int64) + first
    fl, sq, ty = [f], [seq0[f].astype(np.int64) + d], [np.full(general, 3)]
    three = np.array([0, window // 2, window - 1]) + first
    fl.append(np.full(hot, 3)), sq.append(int(seq0[3]) + three[rng.integers(0, 3, hot)]), ty.append(np.full(hot, 3))
    fl.append(np.full(hot, 5)), sq.append(np.full(hot, int(seq0[5]) + 57 * window // 100)), ty.append(np.full(hot, 3))
    edge = np.concatenate([seq0.astype(np.int64) + first - 1, seq0.astype(np.int64) + infl + first])  # one below, one past
    fl.append(np.tile(k, 2)), sq.append(edge), ty.append(np.full(2 * nflows, 3))
    m = 400
    fl.append(rng.integers(0, nflows, m)), sq.append(seq0[fl[-1]].astype(np.int64) + 1), ty.append(rng.integers(0, 3, m))  # non-ACK
    fl.append(rng.choice(np.array([nflows, nflows + 1, T.NO_FLOW], np.int64), m)), sq.append(seq0[rng.integers(0, nflows, m)].astype(np.int64) + 1)
    ty.append(np.full(m, 3))
    fl.append(rng.integers(0, nflows, m)), sq.append(seq0[fl[-1]].astype(np.int64) + 2), ty.append(np.full(m, 3))  # to be damaged
    fl, sq, ty = (np.concatenate(x).astype(np.int64) for x in (fl, sq, ty))
    n = fl.size
    words = np.stack([ty, sq & M32, np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1).astype(">u4")  # ack_datagram's layout
    ring = words.view(np.uint8).reshape(n, 16).copy()
    ring[np.arange(n - m, n), 12 + np.arange(m) % 4] ^= 0x10  # the checksum of the empty payload is 0
    order = rng.permutation(n)
    acked0 = (rng.random(S) < 0.5).astype(np.uint32) * rng.choice(np.array([1, 1, 7], np.uint32), S)
    return dict(ring=ring[order].reshape(-1), rl=np.full(n, 16, np.uint32), flow=fl[order].astype(np.uint32), seq0=seq0,
                rec0=rec0, rec_end=rec_end, acked0=acked0, nflows=nflows, window=window, damaged=int(m), n=n, hot=hot)


def check_ack_batch(case, got):
    """What the batch must be for its test to bite, from the model's (ok, hit, acked, adv, fresh)."""
    ok, hit, _, adv, fresh = got
    nf = case["nflows"]
    flow = case["flow"]
    placed = hit != T.NOT_PLACED
    hits = np.bincount(flow[placed], minlength=nf)
    assert (ok == 0).sum() == case["damaged"] and (flow >= nf).sum() >= 100 and not placed[flow >= nf].any()
    assert ((hits > 0) & (fresh != hits)).mean() > 0.5, "flow_fresh equals the raw hit count in most flows"
    assert (fresh > 0).mean() > 0.5 and hits[3] >= case["hot"] and hits[5] >= case["hot"]
    assert (adv == 0).any() and (adv > 0).any() and case["seq0"][0] == M32 and placed[flow == 0].any()


# ---- 2b. the sender's slide -----------------------------------------------------------------------
SLIDE_WINDOWS = (1, 63, 64, 65, 255, 256, 257, 1024, 1025)


def slide_case(window, nflows=7):
    """flow_adv cycles through 0, 1, window - 1, window, window + 1 and 0xFFFFFFFF; the bases of
    the flows that move lie just below 2^32, so seq0 and rec0 both wrap in the slide."""
    S = nflows * window
    rng = np.random.default_rng(window * 7 + nflows)
    kinds = np.array([0, 1, window - 1, window, window + 1, M32], np.int64)
    adv = kinds[np.arange(nflows) % 6].astype(np.uint32)
    moved = np.minimum(adv.astype(np.int64), window)
    seq0 = ((1 << 32) - (moved + 1) // 2 - (np.arange(nflows) % 2)).astype(np.int64) & M32
    rec0 = ((1 << 32) - moved // 2 - (np.arange(nflows) % 3 == 0)).astype(np.int64) & M32
    acked = (rng.random(S) < 0.5).astype(np.uint32) * rng.integers(1, 9, S).astype(np.uint32)
    sent = rng.integers(0, 1 << 32, S).astype(np.uint32)
    return dict(nflows=nflows, window=window, S=S, adv=adv, seq0=seq0.astype(np.uint32), rec0=rec0.astype(np.uint32), acked=acked,
                sent=sent, fill=0xF111F111)


def check_slide(case, got):
    _, _, sq, rc = got
    moved = np.minimum(case["adv"].astype(np.int64), case["window"])
    assert (sq.astype(np.int64) < case["seq0"]).any() and (rc.astype(np.int64) < case["rec0"]).any()  # both wrap somewhere
    assert np.array_equal(sq, ((case["seq0"].astype(np.int64) + moved) & M32).astype(np.uint32))
    assert set(case["adv"].tolist()) >= ({0, 1, M32} if case["nflows"] >= 6 else {0})


# ---- 3a. every length through the accept ------------------------------------------------------------
def accept_case(stride, top=1484, nflows=3, window=500):
    """(ring, recv_len, flow, seq0, lengths): one intact DATA datagram of every payload length
    0 .. top, dealt round-robin to the flows (length L is slot L // nflows of flow L % nflows), in
    a shuffled arrival order, in `stride`-byte ring slots with random bytes behind each datagram."""
    rng = np.random.default_rng(stride + top)
    seq0 = np.array([M32 - 100, 0, 0x7FFFFFF0][:nflows], np.uint32)
    order = rng.permutation(top + 1)
    ring = rng.integers(0, 256, (top + 1) * stride, dtype=np.uint8)
    rl = np.zeros(top + 1, np.uint32)
    for i, ln in enumerate(order.tolist()):
        d = O.build_datagram((int(seq0[ln % nflows]) + ln // nflows) & M32, O.synth_fill_np(ln, start_byte=ln * 3).tobytes())
        cut = min(len(d), stride)
        ring[i * stride:i * stride + cut] = np.frombuffer(d[:cut], dtype=np.uint8)
        rl[i] = len(d)
    return ring, rl, (order % nflows).astype(np.uint32), seq0, order


# ---- 3b, 3c. every length through the flush and the receiver's slide ----------------------------------
FLUSH_FLOWS, FLUSH_WINDOW = 5, 300
FLUSH_RUNS = (300, 290, 280, 300, 287)  # 1457 slots in the leading runs, 43 behind them


def flush_state(salt, top=MAXP, runs=FLUSH_RUNS, window=FLUSH_WINDOW, fill=None):
    """(image, slot_len, runs) of len(runs) flows: the leading runs together hold every length
    0 .. top once, permuted, with a full-size record in the middle of flow 2's run; the slots
    behind the runs hold 0xFFFFFFFE, 1457, a claim pattern and EMPTY.  sum(runs) == top + 1."""
    nflows = len(runs)
    assert sum(runs) == top + 1 and all(r <= window for r in runs)
    rng = np.random.default_rng(salt)
    lens = rng.permutation(top + 1).astype(np.uint32)
    at = sum(runs[:2]) + runs[2] // 2  # the middle of flow 2's run
    k = int(np.flatnonzero(lens == top)[0])
    lens[k], lens[at] = lens[at], lens[k]
    sl = np.full(nflows * window, EMPTY, np.uint32)
    it, behind = 0, iter([0xFFFFFFFE, MAXP + 1, CLAIM])
    for f, r in enumerate(runs):
        sl[f * window:f * window + r] = lens[it:it + r]
        it += r
        if r + 1 < window:
            sl[f * window + r + 1] = next(behind, EMPTY)  # the slot behind the run's end stays EMPTY
    img = rng.integers(0, 256, nflows * window * MAXP, dtype=np.uint8) if fill is None else np.full(nflows * window * MAXP, fill, np.uint8)
    return img, sl, np.array(runs)


def ack_ring(seqs):
    """16-byte ACK datagrams of these sequence numbers, back to back (retx_model.ack_datagram's)."""
    return np.frombuffer(b"".join(R.ack_datagram(int(s)) for s in seqs), dtype=np.uint8)
