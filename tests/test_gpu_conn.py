"""GPU tests of the connection table, wtp_flows_classify and wtp_flows_control: every output
of both calls is compared with tests/conn_model.py, the sequential model written from the
header, over the fuzz corpus and the directed cases that tests/test_conn_model.py runs on the
CPU, at the batch sizes around the wave and ranking-block edges, with keys at every alignment,
at one large shape, and through whole connection lifecycles, eagerly and from one graph.

The sentinel rule of every case: every output array has guard words behind it and holds a
sentinel past its count; the table, the ACK ring, the ok bytes and the keys sit between guard
bytes (the keys end with their allocation); all inputs are read back unchanged.  The table
is opaque: it is observed only through wtp_flows_classify."""
import numpy as np
import pytest

import conn_model as M
import flows_model as F
from gpu_support import W, W_noinit  # noqa: F401 (fixtures: W for verify's tables in the lifecycle tests)
from gpu_support import Bytes, Words, assert_no_data_error, capture, dev_s32, u32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SENT = 0x0BADC0DE
MAXP, STRIDE = F.MAXP, F.STRIDE
ACK_LAYOUTS = ((16, 0), (24, 0), (17, 1))  # (ack_stride, the ring's byte offset): vector, vector, bytes
KEY_LAYOUTS = ((16, 0), (20, 0), (17, 0), (16, 1), (32, 4))  # (key_stride, the keys' byte offset)


def key_bytes(keys, key_stride):
    """The keys `key_stride` apart; the last one ends the array."""
    n = len(keys)
    out = np.full((n - 1) * key_stride + 16 if n else 0, 0x99, np.uint8)
    for i, k in enumerate(keys):
        out[i * key_stride:i * key_stride + 16] = np.frombuffer(k, np.uint8)
    return out


class DevKeys:
    """A batch's keys on the device, at byte `off` of an allocation that ends with the last key."""

    def __init__(self, keys, key_stride=16, off=0):
        self.n, self.stride = len(keys), key_stride
        self.mem = Bytes(key_bytes(keys, key_stride), off=off, flush=True) if keys else Bytes(fill=0, size=16)
        self.t = self.mem.t


class DevConn:
    """The table of one receiver on the device (between guard bytes, filled with 0xFF once) and
    the calls on it.  The per-flow arrays and the ring are uploaded from the model's entry state
    with every batch, which is what the previous batch left plus what the data path did since."""

    def __init__(self, W, nflows, window, nbuckets):
        self.W, self.nflows, self.window, self.nbuckets = W, nflows, window, nbuckets
        self.table = Bytes(fill=0xFF, size=W.conn_table_bytes(nbuckets), front=64, back=64, guard=0xC3)
        self.calls = 0

    def classify(self, keys, key_stride=16, off=0):
        dk, flow = DevKeys(keys, key_stride, off), Words(SENT, len(keys))
        self.W.flows_classify(dk.t, key_stride, len(keys), self.table.t, self.nbuckets, flow.t)
        torch.cuda.synchronize()
        if keys:
            assert self.W.LIB.wtp_last_kernel().decode() == "k_conn_classify"
        dk.mem.get()  # the guard in front
        return flow.get()

    def control(self, entry, ring, stride, keys, ok, flow, max_acks, want, known=(), exact=True):
        """One batch on the device: classify (compared with `flow`, the model's), control from the
        state `entry`, every output against `want`, and a classify of the keys `known` afterwards
        against the model's table.  exact False: only what holds for every result (see callers).
        Returns the device's outputs."""
        W, nf, w, n = self.W, self.nflows, self.window, len(keys)
        layout = self.calls
        self.calls += 1
        key_stride, key_off = KEY_LAYOUTS[layout % len(KEY_LAYOUTS)]
        ack_stride, ack_off = ACK_LAYOUTS[layout % len(ACK_LAYOUTS)]
        table_before = self.table.get().copy()
        dk = DevKeys(keys, key_stride, key_off)
        d_flow = Words(SENT, n)
        W.flows_classify(dk.t, key_stride, n, self.table.t, self.nbuckets, d_flow.t)
        d_ring = Bytes(ring, off=layout % 2, front=64, back=64)
        d_rl = Words(np.full(n, 16, np.uint32))
        d_ok = Bytes(ok if n else np.zeros(1, np.uint8), front=16, back=16)
        fs, sq, sl = Words(entry.flow_start), Words(entry.seq0), Words(entry.slot_len)
        fr, fp = Words(entry.free), Words(entry.free_pos)
        wire = Bytes(fill=0xA5, size=max(n, 1) * ack_stride, off=ack_off, front=64, back=64, guard=0xA5)
        src, opened, osrc, closed = Words(SENT, n), Words(SENT, nf), Words(SENT, nf), Words(SENT, nf)
        verdict, counts = Words(SENT, n), Words(SENT, 6)
        need = W.conn_scratch_bytes(n, nf)
        work_off = (16, 1, 3)[layout % 3]
        wk = torch.randint(0, 256, (need + work_off + 16,), dtype=torch.uint8, device="cuda")
        before = wk.clone()
        W.flows_control(d_ring.t, stride, d_rl.t, dk.t, key_stride, d_flow.t, d_ok.t, n, self.table.t, self.nbuckets, nf, w,
                        fs.t, sq.t, sl.t, fr.t, fp.t, wire.t, ack_stride, max_acks, src.t, opened.t, osrc.t, closed.t,
                        verdict.t, counts.t, work=wk[work_off:work_off + need])
        torch.cuda.synchronize()
        assert W.LIB.wtp_last_kernel().decode() == ("k_conn_reset" if n and nf * w else "k_conn_emit")
        got = dict(flow=d_flow.get(), verdict=verdict.get(), counts=counts.get(), opened=opened.get(), opened_src=osrc.get(),
                   closed=closed.get(), ack_src=src.get(), flow_start=fs.get(), seq0=sq.get(), slot_len=sl.get(), free=fr.get(),
                   free_pos=fp.get())
        rows = wire.get().reshape(max(n, 1), ack_stride)
        got["ack_seq"] = rows[:, 4:8].copy().view(">u4").reshape(-1).astype(np.uint32)
        # the inputs are only read, the scratch stays inside its bytes, the ring's tails are not written
        assert np.array_equal(d_ring.get(), d_ring.host) and np.array_equal(d_ok.get(), d_ok.host) and (d_rl.get() == 16).all()
        assert np.array_equal(dk.mem.get(), dk.mem.host) if n else True
        assert torch.equal(wk[:work_off], before[:work_off]) and torch.equal(wk[work_off + need:], before[work_off + need:])
        assert (rows[:, 16:] == 0xA5).all()
        e, elig, no, nc = (int(c) for c in got["counts"][:4])
        assert e == min(elig, max_acks) and (rows[e:] == 0xA5).all() and (got["ack_src"][e:] == SENT).all()
        assert (rows[:e, :4] == (0, 0, 0, 3)).all() and (rows[:e, 8:16] == 0).all()
        assert (got["opened"][no:] == SENT).all() and (got["opened_src"][no:] == SENT).all() and (got["closed"][nc:] == SENT).all()
        assert np.array_equal(got["flow"], flow)
        if not (got["verdict"] == M.OPENED).any() and nc == 0:
            assert np.array_equal(self.table.get(), table_before)  # no open and no close: no byte of the table changed
        if exact:
            after = want["state"]
            assert np.array_equal(got["verdict"], want["verdict"]), (got["verdict"].tolist(), want["verdict"].tolist())
            assert got["counts"].tolist() == want["counts"].tolist()
            assert np.array_equal(got["ack_src"][:e], want["ack_src"]) and np.array_equal(got["ack_seq"][:e], want["ack_seq"])
            assert np.array_equal(got["opened"][:no], want["opened"]) and np.array_equal(got["opened_src"][:no], want["opened_src"])
            assert np.array_equal(got["closed"][:nc], want["closed"])
            assert np.array_equal(got["flow_start"], after.flow_start) and np.array_equal(got["seq0"], after.seq0)
            assert np.array_equal(got["slot_len"], after.slot_len)
            assert np.array_equal(got["free"], after.free) and np.array_equal(got["free_pos"], after.free_pos)
            known = list(known)
            if known:
                assert np.array_equal(self.classify(known, *KEY_LAYOUTS[(layout + 1) % len(KEY_LAYOUTS)]), M.classify(after.table, known))
        return got


def bucket(W):
    return W.conn_bucket


# ---- 1. exact against the model, every round ----------------------------------------------------------
def test_fuzz_rounds_against_the_model(W_noinit):
    W = W_noinit
    dev = DevConn(W, M.FUZZ_FLOWS, M.FUZZ_WINDOW, M.FUZZ_BUCKETS)
    keys = M.fuzz_keys()
    seen = np.zeros(10, np.int64)
    for r in M.fuzz_rounds(bucket(W)):
        assert r["want"]["exact"] and not r["want"]["overflow"]
        dev.control(r["entry"], r["ring"], r["stride"], r["keys"], r["ok"], r["flow"], r["max_acks"], r["want"], known=keys)
        seen += np.bincount(r["want"]["verdict"], minlength=10)
    assert (np.delete(seen, M.REFUSED_BUCKET) > 0).all()
    assert_no_data_error(W)


# ---- 2. the directed cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_directed_case(W_noinit, name):
    """Duplicates in a batch, the free ids running out (no trace of the refused keys; the next
    START opens after a close), a full bucket with one bucket and with keys that wtp_conn_bucket
    puts into one of four (the host's hash is the kernels'), END_BUSY, the ring's wrap, the ACK
    ring's cut, no flows at all: every batch exact, at a rotating key and ACK layout."""
    W = W_noinit
    case = next(c for c in M.directed_cases(bucket(W)) if c[0] == name)
    nflows, window, nbuckets, _ = case[1]
    dev = DevConn(W, nflows, window, nbuckets)
    known = sorted({it[0] for step in case[2] if not callable(step) for it in step})
    got = M.run_case(case, bucket(W), call=lambda *a: dev.control(*a, known=known))
    assert all(w["exact"] for w in got)
    if name.startswith("bucket full"):
        assert sum(int(w["counts"][5]) for w in got) >= 1 and int(got[-1]["counts"][2]) == 1
    assert_no_data_error(W)


# ---- 3. batch sizes around the wave and the ranking block ----------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_batch_sizes(W_noinit, n):
    """STARTs of new keys at both ends of the batch; between them duplicates of the first, ENDs
    with no connection (answered, so the ACK ranking crosses every block) and DATA."""
    W = W_noinit
    rng = np.random.default_rng(n)
    a, b, c = M.key_of(1), M.key_of(2), M.key_of(3)
    kinds = [(a, M.START, 7), (c, M.END, 1), (c, M.DATA, 2), (a, M.START, 8), (b, M.END, 9)]
    items = [kinds[int(k)] for k in rng.integers(0, len(kinds), n)]
    if n:
        items[0], items[-1] = (a, M.START, 7), ((b, M.START, 9) if n > 1 else (a, M.START, 7))
    dev = DevConn(W, 4, 3, 2)
    st = M.State(4, 3, 2, head=2)
    for rep in range(2):  # the second time every key is known
        ring, keys, ok = M.make_batch(items, 16)
        flow = M.classify(st.table, keys)
        want = M.control(st, ring, 16, keys, flow, ok, bucket(W), max_acks=n - n // 5)
        got = dev.control(st, ring, 16, keys, ok, flow, n - n // 5, want, known=[a, b, c])
        assert int(got["counts"][2]) == (min(n, 2) if rep == 0 else 0)
        st = want["state"].copy()
    assert_no_data_error(W)


# ---- 4. a bucket that overflows: the specified properties ---------------------------------------------
def test_seventeen_keys_race_for_sixteen_entries(W_noinit):
    """nbuckets 1, 17 new keys in one batch, each twice: 16 are opened and one is refused, which one
    is not specified.  The opened ones get the ring's ids in arrival order, the refused key's two
    datagrams get the same refusal and leave nothing in the table; after one close its next START
    opens into the freed entry."""
    W = W_noinit
    keys = [M.key_of(100 + j) for j in range(17)]
    dev = DevConn(W, 20, 1, 1)
    st = M.State(20, 1, 1)
    items = [(k, M.START, j) for j, k in enumerate(keys)] + [(k, M.START, j) for j, k in enumerate(keys)]
    ring, bkeys, ok = M.make_batch(items)
    flow = M.classify(st.table, bkeys)
    want = M.control(st, ring, 16, bkeys, flow, ok, bucket(W))
    assert want["overflow"] and not want["exact"]
    got = dev.control(st, ring, 16, bkeys, ok, flow, len(items), want, exact=False)
    v = got["verdict"]
    assert got["counts"].tolist() == [32, 32, 16, 0, 0, 2]
    refused = np.flatnonzero(v == M.REFUSED_BUCKET)
    assert refused.size == 2 and refused[1] == refused[0] + 17 and (v[:17] != M.REFUSED_BUCKET).sum() == 16
    opened_idx = np.flatnonzero(v[:17] == M.OPENED)
    assert opened_idx.size == 16 and (np.delete(v[17:], refused[0]) == M.START_DUP).all()
    assert got["opened"][:16].tolist() == list(range(16)) and got["opened_src"][:16].tolist() == opened_idx.tolist()
    assert got["ack_src"][:32].tolist() == sorted(np.flatnonzero(v != M.REFUSED_BUCKET).tolist())
    after = dev.classify(keys)
    assert after[refused[0]] == M.NO_FLOW and np.delete(after, refused[0]).tolist() == list(range(16))
    assert got["free_pos"].tolist() == [16, 4] and (got["slot_len"][:16] == M.EMPTY).all() and (got["slot_len"][16:] == 77).all()
    # the model from the state the device is in
    st.table = {keys[j]: int(after[j]) for j in range(17) if after[j] != M.NO_FLOW}
    for name in ("flow_start", "seq0", "slot_len", "free", "free_pos"):
        setattr(st, name, got[name].copy())
    loser, victim = keys[refused[0]], keys[int(opened_idx[3])]
    for items in ([(loser, M.START, 50)], [(victim, M.END, int(opened_idx[3]))], [(loser, M.START, 50), (loser, M.START, 50)]):
        ring, bkeys, ok = M.make_batch(items)
        flow = M.classify(st.table, bkeys)
        want = M.control(st, ring, 16, bkeys, flow, ok, bucket(W))
        assert want["exact"]
        dev.control(st, ring, 16, bkeys, ok, flow, len(items), want, known=keys)
        st = want["state"].copy()
    assert want["verdict"].tolist() == [M.OPENED, M.START_DUP] and st.table[loser] == 16
    assert_no_data_error(W)


# ---- 5. keys at every alignment -------------------------------------------------------------------------
@pytest.mark.parametrize("key_stride,off", [(16, 0), (20, 0), (17, 0), (16, 1), (20, 2), (4096, 4), (33, 15)])
def test_key_layouts(W_noinit, key_stride, off):
    """classify and control with the keys at this stride and byte offset, the last key ending its
    allocation: the same flows as at stride 16, offset 0, for keys that are there, that are not,
    and that differ from one that is there in one byte."""
    W = W_noinit
    rng = np.random.default_rng(key_stride + off)
    keys = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(70)]
    near = [k[:j] + bytes([k[j] ^ 0x80]) + k[j + 1:] for j, k in zip(range(16), keys)]
    dev = DevConn(W, 64, 1, 16)
    st = M.State(64, 1, 16)
    ring = M.header_ring([M.START] * 64, np.arange(64))
    want = M.control(st, ring, 16, keys[:64], M.classify(st.table, keys[:64]), np.ones(64, np.uint8), bucket(W))
    assert want["exact"] and int(want["counts"][2]) == 64
    dev.control(st, ring, 16, keys[:64], np.ones(64, np.uint8), M.classify(st.table, keys[:64]), 64, want)
    probe = keys + near
    table = want["state"].table
    assert np.array_equal(dev.classify(probe, key_stride, off), M.classify(table, probe))
    assert (M.classify(table, probe) == M.NO_FLOW).sum() == 6 + 16
    # control with the same layout: ENDs by key close exactly those flows
    dk = DevKeys(keys[10:20], key_stride, off)
    st2 = want["state"].copy()
    ring = M.header_ring([M.END] * 10, np.arange(10, 20))
    flow = M.classify(st2.table, keys[10:20])
    want2 = M.control(st2, ring, 16, keys[10:20], flow, np.ones(10, np.uint8), bucket(W))
    assert want2["closed"].tolist() == list(range(10, 20))
    fs, sq, sl, fr, fp = (Words(getattr(st2, k)) for k in ("flow_start", "seq0", "slot_len", "free", "free_pos"))
    out = [Words(SENT, k) for k in (10, 64, 64, 64, 10, 6)]
    wire = Bytes(fill=0xA5, size=160)
    W.flows_control(torch.from_numpy(ring).cuda(), 16, dev_s32(np.full(10, 16)), dk.t, key_stride, dev_s32(flow),
                    torch.ones(10, dtype=torch.uint8, device="cuda"), 10, dev.table.t, 16, 64, 1, fs.t, sq.t, sl.t, fr.t, fp.t,
                    wire.t, 16, 10, *(o.t for o in out))
    torch.cuda.synchronize()
    assert out[5].get().tolist() == want2["counts"].tolist() and out[3].get()[:10].tolist() == list(range(10, 20))
    assert np.array_equal(dev.classify(probe, key_stride, off), M.classify(want2["state"].table, probe))
    assert np.array_equal(dk.mem.get(), dk.mem.host)
    assert_no_data_error(W)


# ---- 6. one large shape ---------------------------------------------------------------------------------
def test_scale(W_noinit):
    """65 536 datagrams of 16 384 distinct keys, nbuckets 8192, nflows 16 384: a batch of STARTs
    (every key four times, the repeats with the first's seqNum or another), then the classify of a
    DATA batch; both against the model."""
    W = W_noinit
    n, nkeys, nb = 65536, 16384, 8192
    rng = np.random.default_rng(0x5CA1E)
    keys = [M.key_of(j & 0xFFFF, 0x0A000000 + j * 7919) for j in range(nkeys)]
    pick = np.concatenate([rng.permutation(nkeys) for _ in range(4)])
    first = np.zeros(nkeys, bool)
    seqs = pick.astype(np.uint32) * 3
    for i, k in enumerate(pick):  # repeats: half of them carry another seqNum
        if first[k] and i % 2:
            seqs[i] += 1
        first[k] = True
    bkeys = [keys[k] for k in pick]
    ring = M.header_ring(np.full(n, M.START), seqs)
    ok = np.ones(n, np.uint8)
    st = M.State(nkeys, 1, nb)
    flow = M.classify(st.table, bkeys)
    want = M.control(st, ring, 16, bkeys, flow, ok, bucket(W), max_acks=38000)
    assert want["exact"] and not want["overflow"] and want["counts"].tolist()[1:4] == [int((want["verdict"] <= 2).sum()), nkeys, 0]
    assert 16384 + 20000 < want["counts"][1] < 65536 and want["counts"][0] == 38000
    dev = DevConn(W, nkeys, 1, nb)
    dev.control(st, ring, 16, bkeys, ok, flow, 38000, want)
    probe = [keys[k] for k in rng.integers(0, nkeys, n - 1000)] + [M.key_of(j, 0x7F000001) for j in range(1000)]
    got = dev.classify(probe, 20, 4)
    assert np.array_equal(got, M.classify(want["state"].table, probe)) and (got[-1000:] == M.NO_FLOW).all()
    assert_no_data_error(W)


# ---- 7. connection lifecycles, eagerly and from one graph ---------------------------------------------
def u64(t):
    return t.cpu().numpy().view(np.uint64)


def _z(k, dt=torch.int32, v=0):
    return torch.full((k,), v, dtype=dt, device="cuda")


class DevReceiver:
    """The receiver of conn_model.Life on the device: two window states, the table, the ring and
    one set of batch and output buffers per half of a step.  A step is the twelve calls of
    call(), made eagerly or replayed from the graph that captured them once; the host rewrites
    the batch buffers before it and reads the outputs after it."""

    class Half:
        def __init__(self, W):
            nf, w, n = M.LIFE_FLOWS, M.LIFE_WINDOW, M.LIFE_N
            self.ring, self.rl, self.keys = _z(n * STRIDE, torch.uint8), _z(n), _z(n * 16, torch.uint8)
            self.flow, self.ok, self.place, self.ack = _z(n), _z(n, torch.uint8), _z(n), _z(nf)
            self.wire, self.src, self.acnt = _z(n * 16, torch.uint8), _z(n), _z(2)
            self.awork = _z(W.rx_ack_flows_work_bytes(n), torch.uint8)
            self.stream = Bytes(fill=0xA5, size=nf * w * MAXP, front=64, back=64, guard=0xA5)
            self.offs, self.lens = _z(nf * w, torch.int64), _z(nf * w)
            self.adv, self.info, self.dcnt = _z(nf, torch.int64), _z(4 * nf, torch.int64), _z(4, torch.int64)
            self.dwork = _z(W.rx_deliver_flows_work_bytes(nf, w), torch.uint8)
            self.cwire, self.csrc = Bytes(fill=0xA5, size=n * 16, front=64, back=64, guard=0xA5), Words(SENT, n)
            self.opened, self.osrc, self.closed = Words(SENT, nf), Words(SENT, nf), Words(SENT, nf)
            self.verdict, self.ccnt = Words(SENT, n), Words(SENT, 6)
            self.cwork = _z(W.conn_scratch_bytes(n, nf), torch.uint8)

    def __init__(self, W, graph=False):
        nf, w = M.LIFE_FLOWS, M.LIFE_WINDOW
        self.W = W
        self.table = Bytes(fill=0xFF, size=W.conn_table_bytes(M.LIFE_BUCKETS), front=64, back=64, guard=0xC3)
        self.img = [_z(nf * w * MAXP, torch.uint8) for _ in range(2)]
        self.sl, self.seq0 = [_z(nf * w) for _ in range(2)], [_z(nf) for _ in range(2)]
        self.flow_start, self.free, self.free_pos = Words(0, nf), Words(0, nf), Words(0, 2)
        self.h = [self.Half(W), self.Half(W)]
        self.reset()
        self.graph = None
        if graph:
            # captured over batches of empty slots, which change nothing; the state is reset all the same
            self.graph, self.stream = capture(self.call)
            self.reset()

    def reset(self):
        nf = M.LIFE_FLOWS
        self.table.payload.fill_(0xFF)
        for x in range(2):
            self.img[x].fill_(0x3C)
            self.sl[x].fill_(-1)
            self.seq0[x].fill_(0x5E90)
        self.flow_start.t.fill_(0x51A27)
        self.free.t.copy_(dev_s32(np.arange(nf)))
        self.free_pos.t.copy_(dev_s32([0, nf]))
        for h in self.h:
            h.rl.fill_(0)
        torch.cuda.synchronize()

    def call(self):
        W, nf, w, n, nb = self.W, M.LIFE_FLOWS, M.LIFE_WINDOW, M.LIFE_N, M.LIFE_BUCKETS
        for h, (a, b) in zip(self.h, ((0, 1), (1, 0))):
            W.flows_classify(h.keys, 16, n, self.table.t, nb, h.flow)
            W.accept_data_packets_flows(h.ring, STRIDE, h.rl, h.flow, n, self.seq0[a], nf, w, self.img[a], self.sl[a], h.ok, h.place,
                                        h.ack)
            W.rx_build_acks_flows(h.ring, STRIDE, h.rl, h.flow, n, F.SELECTIVE, self.seq0[a], nf, w, h.ok, h.ack, h.wire, 16, 0, n,
                                  h.src, h.acnt, work=h.awork)
            W.rx_deliver_flows(self.img[a], self.sl[a], nf, w, w, h.stream.t, nf * w * MAXP, 0, h.offs, h.lens, h.adv, h.info, h.dcnt,
                               work=h.dwork)
            W.rx_advance_flows(self.img[a], self.sl[a], nf, w, h.adv, self.seq0[a], self.img[b], self.sl[b], self.seq0[b])
            W.flows_control(h.ring, STRIDE, h.rl, h.keys, 16, h.flow, h.ok, n, self.table.t, nb, nf, w, self.flow_start.t,
                            self.seq0[b], self.sl[b], self.free.t, self.free_pos.t, h.cwire.t, 16, n, h.csrc.t, h.opened.t,
                            h.osrc.t, h.closed.t, h.verdict.t, h.ccnt.t, work=h.cwork)

    def load(self, halves):
        for h, (_, ring, rl, keys) in zip(self.h, halves):
            h.ring.copy_(torch.from_numpy(ring))
            h.rl.copy_(dev_s32(rl))
            h.keys.copy_(torch.from_numpy(keys))
            for t in (h.csrc, h.opened, h.osrc, h.closed, h.verdict, h.ccnt):
                t.t.fill_(SENT)
            h.cwire.payload.fill_(0xA5)
            h.stream.payload.fill_(0xA5)
            h.cwork.random_(0, 256)
        torch.cuda.synchronize()

    def read(self):
        out = []
        for h, b in zip(self.h, (1, 0)):
            counts = h.ccnt.get()
            e, _, no, nc = (int(c) for c in counts[:4])
            opened, osrc, closed, csrc = h.opened.get(), h.osrc.get(), h.closed.get(), h.csrc.get()
            assert (opened[no:] == SENT).all() and (osrc[no:] == SENT).all() and (closed[nc:] == SENT).all() and (csrc[e:] == SENT).all()
            rows = h.cwire.get().reshape(-1, 16)
            assert (rows[e:] == 0xA5).all() and (rows[:e, :4] == (0, 0, 0, 3)).all()
            out.append(dict(flow=u32(h.flow), ok=h.ok.cpu().numpy(), place=u32(h.place), ack_src=u32(h.src)[:int(u32(h.acnt)[0])],
                            info=u64(h.info).reshape(-1, 4), stream=h.stream.get().copy(), verdict=h.verdict.get(), counts=counts,
                            opened=opened[:no], opened_src=osrc[:no], closed=closed[:nc], ctl_src=csrc[:e],
                            seq0=u32(self.seq0[b])))
        return out

    def replay(self):
        with torch.cuda.stream(self.stream):
            self.graph.replay()

    def step(self, halves):
        self.load(halves)
        if self.graph is None:
            self.call()
        else:
            self.replay()
        torch.cuda.synchronize()
        return self.read()

    def check_finished(self, life):
        """Every id is free again and the table maps none of the run's keys."""
        assert sorted(self.free.get().tolist()) == list(range(M.LIFE_FLOWS)) and int(self.free_pos.get()[1]) == M.LIFE_FLOWS
        flow = Words(SENT, len(life.t))
        keys = torch.from_numpy(np.frombuffer(b"".join(t["key"] for t in life.t), np.uint8).copy()).cuda()
        self.W.flows_classify(keys, 16, len(life.t), self.table.t, M.LIFE_BUCKETS, flow.t)
        assert (flow.get() == M.NO_FLOW).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_lifecycles_against_the_models(W, seed):
    """Eight transfers of mixed-length records over four flows, classify -> accept_flows ->
    build_acks_flows -> deliver_flows -> advance_flows -> control every round: every round's
    outputs are the models', every file is its source, every id is reused with d_seq0 back at 0,
    and DATA that arrives for a closed connection is never placed (conn_model.Life asserts the last
    three as it goes)."""
    want = M.run_life(seed, M.ModelReceiver(bucket(W)))
    dev = DevReceiver(W)
    got = M.run_life(seed, dev)
    assert got.log == want.log and got.step == want.step
    dev.check_finished(got)
    assert_no_data_error(W)


def test_lifecycle_from_one_graph(W):
    """The twelve calls of a step captured once and replayed for every step of a run, the batches
    rewritten on the device in between: the run's log is the eager run's (the models')."""
    want = M.run_life(1, M.ModelReceiver(bucket(W)))
    dev = DevReceiver(W, graph=True)
    got = M.run_life(1, dev)
    assert got.log == want.log
    dev.check_finished(got)
    assert_no_data_error(W)


def test_two_graphs_on_two_streams(W):
    """Two receivers, each with its own table, state, scratch, graph and stream, replayed at the same
    time through two different runs: each run is its model's."""
    seeds = (3, 4)
    want = [M.run_life(s, M.ModelReceiver(bucket(W))) for s in seeds]
    devs = [DevReceiver(W, graph=True) for _ in seeds]
    lives = [M.Life(s) for s in seeds]
    while not all(x.done() for x in lives):
        busy = [(x, d, x.batches()) for x, d in zip(lives, devs) if not x.done()]
        for _, d, halves in busy:
            d.load(halves)
        for _, d, _ in busy:
            d.replay()
        torch.cuda.synchronize()
        for x, d, halves in busy:
            x.absorb(halves, d.read())
    for x, d, w in zip(lives, devs, want):
        x.check_finished()
        d.check_finished(x)
        assert x.log == w.log
    assert len(want[0].log) != len(want[1].log) or want[0].log != want[1].log
    assert_no_data_error(W)
