"""The sequential model of the connection table (include/wtp_crc32.h: wtp_flows_classify,
wtp_flows_control), written from the header: a dict for the table, a list for the free-id
ring, all STARTs one by one in index order, then all ENDs.  The bucket function is an
argument (bucket_of(key, nbuckets)), so the CPU tests run it with the library's
wtp_conn_bucket and with functions of their own.

It also holds the fuzz corpus and the directed cases of the connection tests and the
connection-lifecycle driver; tests/test_conn_model.py runs them over the model and
tests/test_gpu_conn.py over the device calls, with the same seeds and so the same decisions."""
import numpy as np

import oracle as O

EMPTY, NO_FLOW, M32 = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
WAYS, KEY_BYTES = 16, 16
START, END, DATA, ACK = 0, 1, 2, 3
(NONE, OPENED, START_DUP, START_OTHER, REFUSED_FULL, REFUSED_BUCKET, CLOSED, END_STALE, END_OTHER, END_BUSY) = range(10)
ANSWERED = (OPENED, START_DUP, CLOSED, END_STALE)
VERDICTS = ("NONE", "OPENED", "START_DUP", "START_OTHER", "REFUSED_FULL", "REFUSED_BUCKET", "CLOSED", "END_STALE", "END_OTHER",
            "END_BUSY")


def key_of(port, addr=0x0A000001, tail=0):
    """A sockaddr_in as recvmmsg writes it (family 2, port and address in network order) with
    `tail` in its last eight bytes, which the kernel leaves zero: any 16 bytes are a key."""
    return (b"\x02\x00" + int(port).to_bytes(2, "big") + int(addr).to_bytes(4, "big") + int(tail).to_bytes(8, "little"))


def control_dgram(ptype, seq):
    """A START, END or ACK as the endpoints send it: the header alone, length 0, checksum 0."""
    return O.build_datagram(seq & M32, b"", ptype)


def header(ring, stride, i):
    h = bytes(ring[i * stride:i * stride + 8])
    return int.from_bytes(h[0:4], "big"), int.from_bytes(h[4:8], "big")


class State:
    """The caller-owned state of the two calls on the host: the table as a dict from key to
    flow, the per-flow arrays, the free ring and its position."""

    def __init__(self, nflows, window, nbuckets, head=0):
        self.nflows, self.window, self.nbuckets = nflows, window, nbuckets
        self.table = {}
        self.flow_start = np.full(nflows, 0x51A27, np.uint32)
        self.seq0 = np.full(nflows, 0x5E90, np.uint32)
        self.slot_len = np.full(nflows * window, 77, np.uint32)  # not EMPTY: opening resets it
        # a ring whose head is at `head`: the ids in FIFO order from there
        self.free = np.roll(np.arange(nflows, dtype=np.uint32), head)
        self.free_pos = np.array([head % max(nflows, 1), nflows], np.uint32)

    def copy(self):
        s = State.__new__(State)
        s.nflows, s.window, s.nbuckets = self.nflows, self.window, self.nbuckets
        s.table = dict(self.table)
        for k in ("flow_start", "seq0", "slot_len", "free", "free_pos"):
            setattr(s, k, getattr(self, k).copy())
        return s

    def free_ids(self):
        head, count = int(self.free_pos[0]), int(self.free_pos[1])
        return [int(self.free[(head + j) % self.nflows]) for j in range(count)]


def classify(table, keys):
    return np.array([table.get(k, NO_FLOW) for k in keys], dtype=np.uint32)


def control(st, ring, stride, keys, flow, ok, bucket_of, max_acks=None):
    """wtp_flows_control on `st` (not modified).  Returns a dict: state (the State after the
    call), verdict[n], ack_seq / ack_src (the emitted ACKs), opened / opened_src / closed,
    counts[6], overflow (did live entries plus distinct new keys exceed WAYS in a bucket) and
    exact (False where the header leaves open which keys of an overflowing bucket are refused:
    a bucket with free entries, and more new keys than those)."""
    n = len(keys)
    st = st.copy()
    nflows, window, nb = st.nflows, st.window, st.nbuckets
    max_acks = n if max_acks is None else max_acks
    verdict = np.zeros(n, np.uint32)
    hdr = [header(ring, stride, i) if ok[i] else (None, None) for i in range(n)]
    load = [0] * nb
    for k in st.table:
        load[bucket_of(k, nb)] += 1
    live = list(load)
    entry_slot_len = st.slot_len.copy()
    outcome = {}  # what the first START of a new key did: (OPENED, g) or (a refusal, None)
    opened, opened_src, closed = [], [], []
    new_keys = {}
    for i in range(n):
        ptype, seq = hdr[i]
        if ptype != START:
            continue
        f = int(flow[i])
        if f < nflows:
            verdict[i] = START_DUP if seq == st.flow_start[f] else START_OTHER
            continue
        key = keys[i]
        new_keys.setdefault(key, bucket_of(key, nb))
        if key not in outcome:
            b = bucket_of(key, nb)
            if nflows > 0 and load[b] >= WAYS:
                outcome[key] = (REFUSED_BUCKET, None)
            elif st.free_pos[1] == 0:
                outcome[key] = (REFUSED_FULL, None)
            else:
                head = int(st.free_pos[0])
                g = int(st.free[head])
                st.free_pos[0], st.free_pos[1] = (head + 1) % nflows, st.free_pos[1] - 1
                st.table[key] = g
                load[b] += 1
                st.flow_start[g], st.seq0[g] = seq, 0
                st.slot_len[g * window:(g + 1) * window] = EMPTY
                outcome[key] = (OPENED, g)
                opened.append(g)
                opened_src.append(i)
            verdict[i] = outcome[key][0]
        else:
            what, g = outcome[key]
            verdict[i] = what if g is None else START_DUP if seq == st.flow_start[g] else START_OTHER
    pushes = 0
    for i in range(n):
        ptype, seq = hdr[i]
        if ptype != END:
            continue
        f = int(flow[i])
        if f >= nflows:
            verdict[i] = END_STALE
        elif seq != st.flow_start[f]:
            verdict[i] = END_OTHER
        elif window > 0 and entry_slot_len[f * window] != EMPTY:
            verdict[i] = END_BUSY
        elif f in closed:
            verdict[i] = END_STALE
        else:
            verdict[i] = CLOSED
            del st.table[keys[i]]
            # head + count is where it was on entry (an open moves both): behind the ids the ring held then
            st.free[(int(st.free_pos[0]) + int(st.free_pos[1]) + pushes) % nflows] = f
            pushes += 1
            closed.append(f)
    st.free_pos[1] += pushes
    ans = [i for i in range(n) if verdict[i] in ANSWERED]
    ack_src = ans[:max_acks]
    counts = [len(ack_src), len(ans), len(opened), len(closed), int((verdict == REFUSED_FULL).sum()),
              int((verdict == REFUSED_BUCKET).sum())]
    fresh = [0] * nb
    for b in new_keys.values():
        fresh[b] += 1
    # the device's result is the model's unless new keys compete for fewer free entries than they are
    exact = not any(0 < WAYS - live[b] < fresh[b] for b in range(nb))
    return dict(state=st, verdict=verdict, ack_seq=np.array([hdr[i][1] for i in ack_src], np.uint32),
                ack_src=np.array(ack_src, np.uint32), opened=np.array(opened, np.uint32),
                opened_src=np.array(opened_src, np.uint32), closed=np.array(closed, np.uint32),
                counts=np.array(counts, np.uint32), exact=exact,
                overflow=any(live[b] + fresh[b] > WAYS for b in range(nb)))


def make_batch(items, stride=16):
    """(ring, keys, ok) of a batch of (key, type, seqNum) or (key, type, seqNum, ok) items; a DATA
    item carries three payload bytes where the stride has room."""
    n = len(items)
    ring = np.full(max(n, 1) * stride, 0xEE, np.uint8)
    keys, ok = [], np.ones(n, np.uint8)
    for i, it in enumerate(items):
        key, ptype, seq = it[:3]
        d = O.build_datagram(seq & M32, b"abc" if ptype == DATA and stride >= 19 else b"", ptype)
        ring[i * stride:i * stride + len(d)] = np.frombuffer(d, np.uint8)
        keys.append(key)
        if len(it) > 3:
            ok[i] = it[3]
    return ring, keys, ok


def header_ring(types, seqs, stride=16):
    """The ring of make_batch for header-only datagrams of these types and seqNums, without a
    loop: htonl{type, seqNum, 0, crc32("") = 0} at the start of every slot."""
    n = len(types)
    rows = np.zeros((n, 4), dtype=">u4")
    rows[:, 0], rows[:, 1] = types, seqs
    ring = np.full(max(n, 1) * stride, 0xEE, np.uint8)
    ring[:n * stride].reshape(n, stride)[:, :16] = rows.view(np.uint8).reshape(n, 16)
    return ring


# ---- the corpus of the randomised differential test -------------------------------------------
# FUZZ_KEYS keys over FUZZ_FLOWS flows in FUZZ_BUCKETS buckets: at most 8 live entries and at most
# FUZZ_NEW distinct new keys per batch, so no bucket holds more than 14 of its 16 and every
# round is exact.  REFUSED_BUCKET needs a bucket that is full, which the header counts as
# overflow; the directed cases below reach it.
FUZZ_SEED, FUZZ_KEYS, FUZZ_FLOWS, FUZZ_BUCKETS, FUZZ_WINDOW, FUZZ_ROUNDS, FUZZ_NMAX, FUZZ_NEW = 0xC0221, 40, 8, 2, 2, 30, 200, 6
FUZZ_STRIDES = (16, 20, 1472)


def fuzz_keys():
    """40 distinct keys: ports on two addresses, and eight that differ from the first only in
    the bytes behind the address."""
    keys = [key_of(9000 + k, 0x0A000001 + (k & 1)) for k in range(FUZZ_KEYS - 8)]
    return keys + [key_of(9000, 0x0A000001, tail=1 << (8 * k)) for k in range(8)]


def fuzz_rounds(bucket_of, seed=FUZZ_SEED, rounds=FUZZ_ROUNDS):
    """The rounds of the corpus: a list of dicts with the state on entry (entry), the batch
    (ring, stride, keys, ok, flow: the model's classify on entry), max_acks and the model's
    result (want).  Between rounds data "arrives" and is "delivered": slot 0 and 1 of every
    flow and the bases of the open flows change, as accept_flows and advance_flows would."""
    rng = np.random.default_rng(seed)
    keys = fuzz_keys()
    st = State(FUZZ_FLOWS, FUZZ_WINDOW, FUZZ_BUCKETS)
    next_seq = {k: int(rng.integers(0, 1 << 32)) for k in keys}
    next_seq[keys[0]] = M32
    out = []
    for r in range(rounds):
        n = 0 if r == 7 else int(rng.integers(1, FUZZ_NMAX + 1))
        stride = FUZZ_STRIDES[r % len(FUZZ_STRIDES)]
        is_open = {k: st.table[k] for k in st.table}
        fresh, items = [], []
        for _ in range(n):
            key = keys[int(rng.integers(len(keys)))]
            if key not in is_open and key not in fresh:
                if len(fresh) == FUZZ_NEW:
                    key = fresh[int(rng.integers(FUZZ_NEW))]
                else:
                    fresh.append(key)
            u = rng.random()
            mine = int(st.flow_start[is_open[key]]) if key in is_open else next_seq[key]
            seq = mine if rng.random() < 0.7 else (mine + int(rng.integers(1, 3))) & M32
            if u < 0.35:
                items.append((key, START, seq))
            elif u < 0.65:
                items.append((key, END, seq))
            elif u < 0.90:
                items.append((key, DATA, seq))
            elif u < 0.95:
                items.append((key, ACK, seq))
            else:
                items.append((key, (START, END)[int(rng.integers(2))], seq, 0))  # not intact: no control datagram
        ring, bkeys, ok = make_batch(items, stride)
        flow = classify(st.table, bkeys)
        max_acks = n if r % 5 else n // 3
        want = control(st, ring, stride, bkeys, flow, ok, bucket_of, max_acks)
        out.append(dict(entry=st, ring=ring, stride=stride, keys=bkeys, ok=ok, flow=flow, n=n, max_acks=max_acks, want=want))
        st = want["state"].copy()
        for k in keys:  # a closed connection's next START carries another seqNum
            if k in is_open and k not in st.table:
                next_seq[k] = (next_seq[k] + 7) & M32
            elif k in st.table:
                next_seq[k] = int(st.flow_start[st.table[k]])
        live = set(st.table.values())
        for f in range(FUZZ_FLOWS):
            st.slot_len[f * FUZZ_WINDOW] = (EMPTY, EMPTY, 5)[int(rng.integers(3))] if f in live else (EMPTY, 9)[int(rng.integers(2))]
            st.slot_len[f * FUZZ_WINDOW + 1] = (EMPTY, 1456, 0x80000003)[int(rng.integers(3))]
            if f in live:
                st.seq0[f] = int(rng.integers(0, 50))
    return out


def keys_in_bucket(bucket_of, nbuckets, b, count, first_port=20000):
    """`count` distinct keys that bucket_of puts into bucket b of nbuckets."""
    out, port = [], first_port
    while len(out) < count:
        k = key_of(port & 0xFFFF, 0xC0A80000 + (port >> 16))
        if bucket_of(k, nbuckets) == b:
            out.append(k)
        port += 1
    return out


CASE_NAMES = ("duplicates, equal seqNums", "duplicates, differing seqNums", "free ids run out", "refused followers",
              "bucket full, one bucket", "bucket full, four buckets", "busy", "ring wrap", "acks cut", "no flows")


def directed_cases(bucket_of):
    """Named sequences of batches on a fresh State(nflows, window, nbuckets, head): each case is
    (name, state arguments, [batch items ...], max_acks or None); a list entry that is a function
    is applied to the state between two batches (the data path's part)."""
    k = [key_of(7000 + j) for j in range(20)]
    one = keys_in_bucket(bucket_of, 4, 2, 17)

    def fill_slot0(st):
        st.slot_len[:] = EMPTY
        st.slot_len[0] = 3

    def drain(st):
        st.slot_len[:] = EMPTY

    return [
        ("duplicates, equal seqNums", (4, 2, 2, 0), [[(k[0], START, 5)] * 3], None),
        ("duplicates, differing seqNums", (4, 2, 2, 0), [[(k[0], START, 5), (k[0], START, 6), (k[0], START, 5)]], None),
        ("free ids run out", (3, 2, 2, 0),
         [[(k[j], START, 10 + j) for j in range(5)], [(k[0], END, 10)], [(k[3], START, 13), (k[4], START, 14)]], None),
        ("refused followers", (1, 2, 2, 0), [[(k[0], START, 1), (k[1], START, 2), (k[1], START, 2), (k[1], START, 3)]], None),
        ("bucket full, one bucket", (17, 1, 1, 0),
         [[(k[j], START, j) for j in range(16)], [(k[16], START, 16), (k[16], START, 16)], [(k[2], END, 2)],
          [(k[16], START, 16), (k[16], START, 16)]], None),
        ("bucket full, four buckets", (20, 1, 4, 0),
         [[(key, START, j) for j, key in enumerate(one[:16])], [(one[16], START, 16), (k[0], START, 0)], [(one[5], END, 5)],
          [(one[16], START, 16)]], None),
        ("busy", (2, 3, 2, 0),
         [[(k[0], START, 9)], fill_slot0, [(k[0], END, 9), (k[0], END, 8)], drain, [(k[0], END, 9), (k[0], END, 9), (k[1], END, 9)]],
         None),
        ("ring wrap", (4, 1, 2, 3), [[(k[j], START, j) for j in range(3)], [(k[0], END, 0), (k[1], END, 1)],
                                     [(k[j], START, j) for j in range(3, 6)]], None),
        ("acks cut", (4, 1, 2, 0), [[(k[j], START, j) for j in range(4)] + [(k[9], END, 0)],
                                    [(k[0], END, 0), (k[1], START, 1), (k[2], END, 2), (k[9], END, 1)]], 2),
        ("no flows", (0, 0, 1, 0), [[(k[0], START, 1), (k[0], END, 1), (k[1], DATA, 0)]], None),
    ]


def run_case(case, bucket_of, call=None, stride=16):
    """The batches of one directed case over the model; `call(entry_state, ring, stride, keys, ok,
    flow, max_acks, want)` is given every batch (the GPU test's comparison).  Returns the
    results."""
    name, (nflows, window, nbuckets, head), steps, max_acks = case
    st = State(nflows, window, nbuckets, head)
    results = []
    for step in steps:
        if callable(step):
            step(st)
            continue
        ring, keys, ok = make_batch(step, stride)
        flow = classify(st.table, keys)
        want = control(st, ring, stride, keys, flow, ok, bucket_of, max_acks)
        if call:
            call(st, ring, stride, keys, ok, flow, len(keys) if max_acks is None else max_acks, want)
        results.append(want)
        st = want["state"].copy()
    return results


# ---- connection lifecycles through one receiver -------------------------------------------------
# LIFE_TRANSFERS senders, each with a key and a START seqNum of its own and mixed-length records
# numbered from 0 (the endpoints' expected = 0), come and go over LIFE_FLOWS flows: more want to
# be open than there are ids, so STARTs are refused and come again, and every id is reused.  A
# sender sends START until it is ACKed, then its records through a window of LIFE_WINDOW with
# selective ACKs, then END until it is ACKed; one step later it sends a stale DATA datagram and
# a second END.  A step is two receive rounds (state A -> B, then B -> A: what one graph
# replays): both halves carry a lossy, permuted copy of what the senders have in flight, so
# the second half brings duplicates of the first; the batches are padded to LIFE_N datagrams
# with empty slots (recv_len 0).  A round is classify -> accept_flows -> build_acks_flows ->
# deliver_flows -> advance_flows -> control; the ACK rings are lossy too.
LIFE_FLOWS, LIFE_WINDOW, LIFE_BUCKETS, LIFE_TRANSFERS, LIFE_N, LIFE_LOSS, LIFE_MAX_STEPS = 4, 4, 2, 8, 48, 0.15, 80
LIFE_BEGIN = (0, 0, 1, 1, 2, 3, 4, 5)
MAXP, STRIDE, NOT_PLACED = 1456, 1472, 0xFFFFFFFF


class Life:
    """The senders and the host side of the receiver.  batches() gives a step's two halves as
    (items, ring, recv_len, keys): items[i] = (transfer, type, seqNum) of datagram i.  absorb()
    takes the two halves' results, each a dict of what the host reads back after a round:
    flow, ok, place (n each), ack_src (the data ACKs' datagram indices), info (nflows x 4,
    deliver_flows' d_flow_info), stream (the round's packed stream), verdict, counts, opened,
    opened_src, closed, ctl_src (the control ACKs' datagram indices) and seq0 after the round."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.t = []
        for j in range(LIFE_TRANSFERS):
            lens = O.zipf_lengths(7 + j % 3, seed=seed + j)
            lens[1:5] = [0, 1456, 1, 17]
            offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
            self.t.append(dict(key=key_of(5000 + j, 0x0A0A0000 + (seed & 0xFF)), start=(0xFFFFFFFE + 3 * j + seed) & M32, lens=lens,
                               offs=offs, data=O.synth_fill_np(int(lens.sum()), start_byte=13 * j + seed), state="idle",
                               acked=np.zeros(lens.size, bool), file=bytearray()))
        self.step, self.owner, self.log = 0, {}, []
        self.opens = np.zeros(LIFE_FLOWS, np.int64)
        self.refused = self.stale_checked = 0

    def done(self):
        return all(t["state"] == "gone" for t in self.t)

    def in_flight(self):
        out = []
        for j, t in enumerate(self.t):
            if t["state"] == "idle" and self.step >= LIFE_BEGIN[j]:
                t["state"] = "starting"
            if t["state"] == "starting":
                out.append((j, START, t["start"]))
            elif t["state"] == "data":
                base = int(np.argmin(t["acked"]))
                out += [(j, DATA, s) for s in range(base, min(base + LIFE_WINDOW, t["lens"].size)) if not t["acked"][s]]
            elif t["state"] == "ending":
                out.append((j, END, t["start"]))
            elif t["state"] == "done":  # what is still on the wire when the connection is gone
                out += [(j, DATA, 0), (j, END, t["start"])]
                t["state"] = "gone"
        return out

    def batches(self):
        sent = self.in_flight()
        halves = []
        for _ in range(2):
            pick = self.rng.permutation(len(sent))
            pick = pick[self.rng.random(len(sent))[pick] >= LIFE_LOSS]
            items = [sent[k] for k in pick]
            assert len(items) <= LIFE_N
            ring = np.full(LIFE_N * STRIDE, 0xEE, np.uint8)
            rl = np.zeros(LIFE_N, np.uint32)
            keys = np.zeros(LIFE_N * KEY_BYTES, np.uint8)
            for i, (j, ptype, seq) in enumerate(items):
                t = self.t[j]
                pay = t["data"][t["offs"][seq]:t["offs"][seq] + t["lens"][seq]].tobytes() if ptype == DATA else b""
                d = O.build_datagram(seq & M32, pay, ptype)
                ring[i * STRIDE:i * STRIDE + len(d)] = np.frombuffer(d, np.uint8)
                rl[i] = len(d)
                keys[i * KEY_BYTES:(i + 1) * KEY_BYTES] = np.frombuffer(t["key"], np.uint8)
            halves.append((items, ring, rl, keys))
        self.step += 1
        assert self.step <= LIFE_MAX_STEPS, [t["state"] for t in self.t]
        return halves

    def absorb(self, halves, results):
        for (items, _, _, _), r in zip(halves, results):
            n = len(items)
            open_keys = {self.t[j]["key"] for j in self.owner.values()}
            assert all(r["ok"][:n]) and not any(r["ok"][n:]) and (np.asarray(r["verdict"][n:]) == NONE).all()
            for i, (j, ptype, seq) in enumerate(items):  # no connection: no flow, and DATA is never placed
                if self.t[j]["key"] not in open_keys:
                    assert r["flow"][i] == NO_FLOW and r["place"][i] == NOT_PLACED
                    self.stale_checked += ptype == DATA
                else:
                    assert self.owner[int(r["flow"][i])] == j
            for f in range(LIFE_FLOWS):  # the flows' byte ranges of the round's stream go to their files
                _, _, at, nbytes = (int(v) for v in r["info"][f])
                if nbytes:
                    self.t[self.owner[f]]["file"] += bytes(r["stream"][at:at + nbytes])
            for i in r["ack_src"]:
                if self.rng.random() >= LIFE_LOSS:
                    j, ptype, seq = items[int(i)]
                    assert ptype == DATA
                    self.t[j]["acked"][seq] = True
            for g, i in zip(r["opened"], r["opened_src"]):
                self.owner[int(g)] = items[int(i)][0]
                self.opens[int(g)] += 1
                assert r["seq0"][int(g)] == 0
            for f in r["closed"]:
                del self.owner[int(f)]
            self.refused += int(r["counts"][4])
            for i in r["ctl_src"]:
                if self.rng.random() >= LIFE_LOSS:
                    j, ptype, seq = items[int(i)]
                    t = self.t[j]
                    if ptype == START and t["state"] == "starting":
                        t["state"] = "data"
                    elif ptype == END and t["state"] == "ending":
                        t["state"] = "done"
            for t in self.t:
                if t["state"] == "data" and t["acked"].all():
                    t["state"] = "ending"
            self.log.append(tuple(np.asarray(r[k]).astype(np.int64).reshape(-1).tolist() for k in (
                "flow", "place", "ack_src", "info", "verdict", "counts", "opened", "opened_src", "closed", "ctl_src", "seq0")))

    def check_finished(self):
        for t in self.t:
            assert bytes(t["file"]) == t["data"].tobytes()  # every delivered byte range is its source's
        assert (self.opens >= 2).all() and self.opens.sum() == LIFE_TRANSFERS and not self.owner
        assert self.refused >= 1 and self.stale_checked >= LIFE_TRANSFERS // 2


class ModelReceiver:
    """The receiver's six calls on the models, two window states as the device keeps them."""

    def __init__(self, bucket_of):
        import flows_flush_model
        import flows_model
        self.F, self.FM, self.bucket_of = flows_model, flows_flush_model, bucket_of
        nf, w = LIFE_FLOWS, LIFE_WINDOW
        self.st = State(nf, w, LIFE_BUCKETS)
        self.img = [np.full(nf * w * MAXP, 0x3C, np.uint8) for _ in range(2)]
        self.sl = [np.full(nf * w, EMPTY, np.uint32) for _ in range(2)]  # accept_flows' initial state: nothing to deliver
        self.seq0 = [np.full(nf, 0x5E90, np.uint32) for _ in range(2)]

    def round(self, half, a, b):
        F, FM, nf, w, n = self.F, self.FM, LIFE_FLOWS, LIFE_WINDOW, LIFE_N
        items, ring, rl, keys = half
        bkeys = [keys[i * KEY_BYTES:(i + 1) * KEY_BYTES].tobytes() for i in range(n)]
        flow = classify(self.st.table, bkeys)
        ok, place, self.img[a], self.sl[a], ack = F.accept_flows(ring, STRIDE, rl, flow, self.seq0[a], nf, w, self.img[a], self.sl[a])
        _, src, _ = F.build_acks_flows(ring, STRIDE, rl, flow, F.SELECTIVE, self.seq0[a], nf, w, ok, ack)
        cap = nf * w * MAXP
        stream, _, _, adv, info, _ = FM.deliver_flows(self.img[a], self.sl[a], nf, w, w, np.full(cap, 0xA5, np.uint8), cap, 0,
                                                      np.zeros(nf * w, np.uint64), np.zeros(nf * w, np.uint32))
        self.img[b], self.sl[b], self.seq0[b] = FM.advance_flows(self.img[a], self.sl[a], nf, w, adv, self.seq0[a], self.img[b],
                                                                 self.sl[b], self.seq0[b])
        self.st.seq0, self.st.slot_len = self.seq0[b], self.sl[b]
        want = control(self.st, ring, STRIDE, bkeys, flow, ok, self.bucket_of)
        assert want["exact"]
        self.st = want["state"]
        self.seq0[b], self.sl[b] = self.st.seq0, self.st.slot_len
        return dict(flow=flow, ok=ok, place=place, ack_src=src, info=info, stream=stream, verdict=want["verdict"],
                    counts=want["counts"], opened=want["opened"], opened_src=want["opened_src"], closed=want["closed"],
                    ctl_src=want["ack_src"], seq0=self.seq0[b].copy())

    def step(self, halves):
        return [self.round(halves[0], 0, 1), self.round(halves[1], 1, 0)]


def run_life(seed, receiver):
    """One lifecycle run to its end over `receiver` (an object with step(halves)); returns the Life."""
    life = Life(seed)
    while not life.done():
        halves = life.batches()
        life.absorb(halves, receiver.step(halves))
    life.check_finished()
    return life
