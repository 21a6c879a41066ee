"""wtp_rx_digest_flows on the GPU against tests/digest_model.py: every output of every call is
compared whole with the model's, guard words sit behind every output array and around the
scratch (whose contents are random on entry), and every input is read back unchanged."""
import numpy as np
import pytest

import conn_model as CM
import digest_model as M
import flows_model as F
import oracle as O
from gpu_support import W, W_noinit  # noqa: F401 (fixtures)
from gpu_support import (BOUNDS, MAXP, STRIDE, Bytes, Words, assert_no_data_error, capture, datagram_ring, dev_s32, periodic,
                         periodic_crc, replay_each_then_together, u32)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
GIB = 1 << 30
SENT32, SENT64 = 0x0BADD1CE, 0x0BADD1CE0BADD1CE


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Call:
    """One call's device buffers.  stream: a Bytes (its payload is d_stream).  ranges: (B, bytes)
    per flow.  crc0 / bytes0: the state on entry (zero by default).  reset / report: (ids,
    count, max) or None; the id arrays hold 2 entries more than max, which must keep their
    values, as the output entries past the count must."""

    def __init__(self, W, stream, ranges, crc0=None, bytes0=None, reset=None, report=None, stream_bytes=None, work_off=3):
        self.W, self.stream, self.nf = W, stream, len(ranges)
        self.stream_bytes = stream.size if stream_bytes is None else stream_bytes
        self.h_info = M.info_of(ranges)
        self.info = Words(self.h_info.reshape(-1), dtype=np.uint64)
        self.h_crc = np.zeros(self.nf, np.uint32) if crc0 is None else np.array(crc0, np.uint32)
        self.h_bytes = np.zeros(self.nf, np.uint64) if bytes0 is None else np.array(bytes0, np.uint64)
        self.crc, self.bytes = Words(self.h_crc), Words(self.h_bytes, dtype=np.uint64)
        self.counts = Words(SENT64, 4, dtype=np.uint64)
        self.lists = []
        for spec in (reset, report):
            if spec is None:
                self.lists.append(None)
            else:
                ids, count, cap = spec
                self.lists.append((np.array(ids, np.uint32), Words(ids), int(count), Words([count]), cap))
        cap = self.lists[1][4] if self.lists[1] else 0
        self.rcrc, self.rbytes = Words(SENT32, cap + 2), Words(SENT64, cap + 2, dtype=np.uint64)
        need = W.rx_digest_scratch_bytes(self.nf)
        self.work = Bytes(fill=0, size=need, off=work_off, front=16, back=16, guard=0x6B)
        self.work.payload.random_(0, 256)

    def args(self):
        rs, rp = self.lists
        return (self.stream.t, self.stream_bytes, self.info.t, self.nf, self.crc.t, self.bytes.t,
                rs[1].t if rs else None, rs[3].t if rs else None, rs[4] if rs else 0,
                rp[1].t if rp else None, rp[3].t if rp else None, rp[4] if rp else 0, self.rcrc.t, self.rbytes.t, self.counts.t)

    def run(self, stream=None):
        self.W.rx_digest_flows(*self.args(), work=self.work.payload, stream=stream)

    def want(self, host_stream=None, seg_crc=None):
        rs, rp = self.lists
        return M.digest(host_stream, self.stream_bytes, self.h_info, self.h_crc, self.h_bytes,
                        reset=rs[0] if rs else None, reset_count=rs[2] if rs else 0, max_reset=rs[4] if rs else 0,
                        report=rp[0] if rp else None, report_count=rp[2] if rp else 0, max_report=rp[4] if rp else 0,
                        report_crc=np.full(self.rcrc.n, SENT32, np.uint32), report_bytes=np.full(self.rbytes.n, SENT64, np.uint64),
                        seg_crc=seg_crc)

    def got(self):
        """The outputs, after the guard checks and the checks that the inputs were only read."""
        self.work.check_guards()
        assert np.array_equal(self.info.get(), self.h_info.reshape(-1))
        for spec in self.lists:
            if spec:
                assert np.array_equal(spec[1].get(), spec[0]) and int(spec[3].get()[0]) == spec[2]
        return self.crc.get(), self.bytes.get(), self.rcrc.get(), self.rbytes.get(), self.counts.get()

    def check(self, want, last="k_dig_report"):
        torch.cuda.synchronize()
        got = self.got()
        for name, g, w in zip(("flow_crc", "flow_bytes", "report_crc", "report_bytes", "counts"), got, want):
            if not np.array_equal(g, w):
                bad = np.flatnonzero(g != w)
                f = int(bad[0])
                where = [int(v) for v in self.h_info[f, 2:]] if name.startswith("flow") else ""
                raise AssertionError(f"{name}: {bad.size} differ, first at {f} {where}: got {int(g[f]):#x}, want {int(w[f]):#x}")
        if last:
            assert self.W.LIB.wtp_last_kernel().decode() == last
        return got


def both(W, stream, host, ranges, **kw):
    c = Call(W, stream, ranges, **kw)
    c.run()
    got = c.check(c.want(host), last="k_dig_reset" if kw.get("reset") and kw["reset"][2] and ranges else "k_dig_report")
    assert np.array_equal(stream.get(), host)  # between its guards, unchanged
    return c, got


# ---- 1. unit edges without knowing the unit -----------------------------------------------------------
POW = range(6, 18)
STARTS = [0, 1, 3, 15, 16, 17] + [(1 << k) + d for k in POW for d in (-1, 0, 1)]
LENGTHS = list(range(6)) + [15, 16, 17, 63, 64, 65] + [v for k in POW for v in ((1 << k) - 1, 1 << k, (1 << k) + 1, (2 << k) + 7)]


@pytest.fixture(scope="module")
def edge_stream():
    host = np.random.default_rng(0xD16E57).integers(0, 256, max(STARTS) + max(LENGTHS), dtype=np.uint8)
    ranges = [(b, n) for b in STARTS for n in LENGTHS]
    want = M.digest(host, host.size, M.info_of(ranges), np.zeros(len(ranges), np.uint32), np.zeros(len(ranges), np.uint64))
    return host, ranges, want


@pytest.mark.parametrize("phase", [0, 5])
def test_unit_edges(W_noinit, edge_stream, phase):
    """Every start against every length in one call of 2520 overlapping flows, the stream's
    base at byte `phase` past a 16-B boundary."""
    host, ranges, want = edge_stream
    stream = Bytes(host, off=phase, front=64, back=64)
    c = Call(W_noinit, stream, ranges)
    c.run()
    got = c.check(want[:2] + c.want(host, seg_crc=lambda b, n: 0)[2:4] + (want[4],))
    assert int(got[4][1]) == sum(n > 0 for _, n in ranges) and int(got[4][2]) == 0
    assert np.array_equal(stream.get(), host)
    assert_no_data_error(W_noinit)


# ---- 2. buffer edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("off,size", [(5, 10007), (0, 8192), (15, 4097), (1, 33), (9, 7)])
def test_buffer_edges(W_noinit, off, size):
    """Ranges that begin with the buffer and ranges that end with it: the guard bytes on both
    sides, whatever they hold, are not part of any result."""
    host = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
    ranges = [(0, n) for n in (1, 2, 16, 17, 4096, 4100, size) if n <= size]
    ranges += [(size - n, n) for n in (1, 2, 16, 17, 4096, 4100, size - 3) if 0 < n <= size] + [(size, 0), (0, 0)]
    outs = []
    for guard in (0xC3, 0x3C):
        stream = Bytes(host, off=off, front=64, back=64, guard=guard)
        outs.append(both(W_noinit, stream, host, ranges)[1])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


# ---- 3. refused ranges ----------------------------------------------------------------------------------
def test_refused_ranges(W_noinit):
    size = 20000
    host = np.random.default_rng(3).integers(0, 256, size, dtype=np.uint8)
    bad = [(size + 1, 0), (size + 1, 5), (1 << 63, 1), (size - 4, 5), (0, size + 1), (7, (1 << 64) - 1), ((1 << 64) - 8, 16),
           (8, (1 << 64) - 4), ((1 << 64) - 1, (1 << 64) - 1)]
    good = [(0, size), (size, 0), (size - 4, 4), (100, 9000), (4095, 2)]
    ranges = [r for pair in zip(bad, good * 2) for r in pair]
    rng = np.random.default_rng(33)
    crc0 = rng.integers(1, 1 << 32, len(ranges), dtype=np.uint64).astype(np.uint32)
    bytes0 = rng.integers(1, 1 << 40, len(ranges), dtype=np.uint64)
    stream = Bytes(host, off=7, front=64, back=64)
    _, got = both(W_noinit, stream, host, ranges, crc0=crc0, bytes0=bytes0)
    assert int(got[4][2]) == len(bad)
    assert np.array_equal(got[0][0::2], crc0[0::2]) and np.array_equal(got[1][0::2], bytes0[0::2])  # untouched
    assert_no_data_error(W_noinit)  # no status flag


# ---- 4. the running combine ----------------------------------------------------------------------------
def test_running_combine(W_noinit):
    size = 70000
    host = np.random.default_rng(4).integers(0, 256, size, dtype=np.uint8)
    rng = np.random.default_rng(44)
    starts = rng.integers(0, size - 9000, 300)
    ranges = [(int(b), int(n)) for b, n in zip(starts, rng.integers(0, 9000, 300))]
    crc0 = rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    bytes0 = (1 << 40) - rng.integers(0, 5000, 300).astype(np.uint64)
    bytes0[0], ranges[0] = (1 << 64) - 5, (11, 100)  # the byte count wraps mod 2^64
    stream = Bytes(host, off=11, front=64, back=64)
    _, got = both(W_noinit, stream, host, ranges, crc0=crc0, bytes0=bytes0)
    for f in (0, 1, 299):
        b, n = ranges[f]
        assert int(got[0][f]) == (O.combine(int(crc0[f]), O.crc32(host[b:b + n]), n) if n else int(crc0[f]))
        assert int(got[1][f]) == (int(bytes0[f]) + n) % (1 << 64)


# ---- 5. scale shapes -------------------------------------------------------------------------------------
def test_many_flows_mostly_empty(W_noinit):
    """65,536 flows: a run of 3000 empty ones, nine of ten of the rest empty, the others one to
    three short records back to back in the stream."""
    nf = 1 << 16
    rng = np.random.default_rng(5)
    n = np.where(rng.random(nf) < 0.1, rng.integers(1, 4, nf) * rng.integers(1, MAXP + 1, nf), 0)
    n[20000:23000] = 0
    n[[0, 19999, 23000, nf - 1]] = [1, MAXP, 3 * MAXP, 17]
    b = np.concatenate([[0], np.cumsum(n[:-1])])
    host = rng.integers(0, 256, int(n.sum()), dtype=np.uint8)
    stream = Bytes(host, off=3, front=64, back=64)
    _, got = both(W_noinit, stream, host, list(zip(b.tolist(), n.tolist())))
    assert int(got[4][0]) == host.size and int(got[4][1]) == int((n > 0).sum())


def test_one_large_flow_against_the_buffer_call(W):
    """One flow of 64 MiB: every wave of the grid flushes into one flow.  With nflows == 1 and a
    zeroed state the result is wtp_crc32_buffer's, round after round."""
    size = 64 << 20
    host = np.random.default_rng(6).integers(0, 256, size, dtype=np.uint8)
    stream = Bytes(host, off=9, front=64, back=64)
    c = Call(W, stream, [(0, size)])
    c.run()
    whole = O.crc32(host)
    got = c.check(c.want(host, lambda b, n: whole))
    assert int(got[0][0]) == whole and got[4].tolist() == [size, 1, 0, 0]
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(stream.t, size, out)
    assert int(u32(out)[0]) == whole
    # the same file in three rounds of odd sizes, the state carried on the device
    cuts = [0, 12345677, 12345678, 50000001, size]
    crc, nb = Words(0, 1), Words(0, 1, dtype=np.uint64)
    for a, e in zip(cuts, cuts[1:]):
        r = Call(W, stream, [(a, e - a)])
        r.crc, r.bytes = crc, nb
        r.run()
    torch.cuda.synchronize()
    assert int(crc.get()[0]) == whole and int(nb.get()[0]) == size
    stream.check_guards()


# ---- 6. the lists ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,cap", [(0, 4), (3, 8), (8, 8), (11, 8), (5, 0)])
def test_lists(W_noinit, count, cap):
    size, nf = 9000, 12
    host = np.random.default_rng(60 + count).integers(0, 256, size, dtype=np.uint8)
    ranges = [(700 * f, 650 + f) for f in range(nf)]
    ids = [3, 3, nf, 0, 0xFFFFFFFF, 7, nf - 1, 3, 5, 11, 2, 1, 9][:cap + 2]  # duplicates, ids >= nflows, 3 and 7 in both lists
    other = [7, 1 << 31, 3, 7, 4, nf + 5, 6, 8, 10, 0][:cap + 2]
    crc0 = np.arange(1, nf + 1, dtype=np.uint32) * 0x01010101
    stream = Bytes(host, off=2, front=64, back=64)
    for reset, report in (((ids, count, cap), (other, min(count + 1, 9), cap)), ((other, count, cap), None), (None, (ids, count, cap)),
                          (None, None)):
        _, got = both(W_noinit, stream, host, ranges, crc0=crc0, bytes0=np.full(nf, 5, np.uint64), reset=reset, report=report)
        k = min(report[1], cap) if report else 0
        assert int(got[4][3]) == k and (got[2][k:] == SENT32).all() and (got[3][k:] == SENT64).all()
        if reset and report and min(count, cap) > 0 and k > 2:
            assert got[0][3] == 0 and got[1][3] == 0 and got[2][2] != 0 and got[3][2] == 5 + 653  # reported folded, then zeroed


def test_no_flows(W_noinit):
    """nflows == 0 is valid: the counts and the report entries (no id is below nflows) are written."""
    stream = Bytes(np.arange(64, dtype=np.uint8), front=16, back=16)
    c = Call(W_noinit, stream, [], report=([0, 5], 2, 2), reset=([0], 1, 1))
    c.run()
    got = c.check(c.want(stream.host))
    assert got[2][:2].tolist() == [0, 0] and got[3][:2].tolist() == [M.NO_BYTES] * 2 and got[4].tolist() == [0, 0, 0, 2]


# ---- 7. end to end ---------------------------------------------------------------------------------------
def _z(k, dt=torch.int32, v=0):
    return torch.full((k,), v, dtype=dt, device="cuda")


def test_five_flows_through_a_stream_that_cuts(W_noinit):
    """Five files of mixed-length records, zero-length ones included, through rounds of
    accept_flows -> build_acks_flows -> deliver_flows -> advance_flows -> digest with a stream of
    3000 bytes: the cut falls inside a flow and the later flows deliver nothing that round.  At
    the end every flow's (crc, bytes) is its file's."""
    W, nf, w, cap = W_noinit, 5, 4, 3000
    rng = np.random.default_rng(7)
    lens = [[1456, 0, 1, 17, 1456, 1455, 0], [0], [5, 1456, 1456, 1456, 2, 0, 0, 900, 16], [], [1456] * 3 + [0, 0, 33]]
    files = [rng.integers(0, 256, sum(ls), dtype=np.uint8) for ls in lens]
    start = [0xFFFFFFFE, 7, 0, 99, 1 << 31]
    img, sl = [_z(nf * w * MAXP, torch.uint8, 0x3C) for _ in range(2)], [_z(nf * w, v=-1) for _ in range(2)]
    seq0 = [dev_s32(start), _z(nf)]
    stream = Bytes(fill=0xA5, size=cap, off=5, front=64, back=64, guard=0xA5)
    adv, info, dcnt = _z(nf, torch.int64), _z(4 * nf, torch.int64), _z(4, torch.int64)
    crc, nb, counts = Words(0, nf), Words(0, nf, dtype=np.uint64), Words(SENT64, 4, dtype=np.uint64)
    work = _z(W.rx_digest_scratch_bytes(nf), torch.uint8)
    done, rounds, starved = [0] * nf, 0, 0
    while any(done[f] < len(lens[f]) for f in range(nf)):
        dgrams, flow = [], []
        for f in range(nf):
            offs = np.concatenate([[0], np.cumsum(lens[f])]).astype(int)
            for r in range(done[f], min(done[f] + w, len(lens[f]))):
                dgrams.append(O.build_datagram((start[f] + r) & 0xFFFFFFFF, files[f][offs[r]:offs[r + 1]].tobytes()))
                flow.append(f)
        n = len(dgrams)
        h_ring, h_rl = datagram_ring(dgrams, STRIDE)
        ring, rl, d_flow = torch.from_numpy(h_ring).cuda(), dev_s32(h_rl), dev_s32(flow)
        ok, ack, wire, src, acnt = _z(n, torch.uint8), _z(nf), _z(n * 16, torch.uint8), _z(n), _z(2)
        W.accept_data_packets_flows(ring, STRIDE, rl, d_flow, n, seq0[0], nf, w, img[0], sl[0], ok, None, ack)
        W.rx_build_acks_flows(ring, STRIDE, rl, d_flow, n, F.SELECTIVE, seq0[0], nf, w, ok, ack, wire, 16, 0, n, src, acnt)
        W.rx_deliver_flows(img[0], sl[0], nf, w, w, stream.t, cap, 0, None, None, adv, info, dcnt)
        W.rx_advance_flows(img[0], sl[0], nf, w, adv, seq0[0], img[1], sl[1], seq0[1])
        W.rx_digest_flows(stream.t, cap, info, nf, crc.t, nb.t, None, None, 0, None, None, 0, None, None, counts.t, work=work)
        torch.cuda.synchronize()
        k = u64(adv).tolist()
        h_info = u64(info).reshape(nf, 4)
        assert bool(ok.all()) and int(counts.get()[0]) == int(h_info[:, 3].sum()) == int(u64(dcnt)[2])
        starved += any(k[f] == 0 and done[f] < len(lens[f]) for f in range(nf))
        done = [d + a for d, a in zip(done, k)]
        for x in (img, sl, seq0):
            x.reverse()
        rounds += 1
        assert rounds < 40
    assert starved >= 2  # the cut did fall before a flow that had records
    assert crc.get().tolist() == [O.crc32(x) for x in files] and nb.get().tolist() == [x.size for x in files]
    stream.check_guards()
    assert_no_data_error(W)


def _receiver():
    import test_gpu_conn  # the lifecycle receiver of the connection table's tests, reused as it is
    return test_gpu_conn.DevReceiver


def make_receiver(W, graph=False):
    nf = CM.LIFE_FLOWS

    class DigestReceiver(_receiver()):
        """DevReceiver with wtp_rx_digest_flows as the seventh call of each round, wired to
        control's lists: d_report = d_closed, d_reset = d_opened, the counts control's d_counts + 3
        and + 2."""

        def __init__(self, W, graph=False):
            self.crc, self.nb = Words(0, nf), Words(0, nf, dtype=np.uint64)
            self.dig = [dict(rcrc=Words(SENT32, nf), rbytes=Words(SENT64, nf, dtype=np.uint64), counts=Words(SENT64, 4, dtype=np.uint64),
                             work=_z(W.rx_digest_scratch_bytes(nf) + 1, torch.uint8)) for _ in range(2)]
            self.reports = []
            super().__init__(W, graph)

        def reset(self):
            super().reset()
            self.crc.t.fill_(0)
            self.nb.t.fill_(0)
            torch.cuda.synchronize()

        def call(self):
            W, w, n, nb = self.W, CM.LIFE_WINDOW, CM.LIFE_N, CM.LIFE_BUCKETS
            for h, d, (a, b) in zip(self.h, self.dig, ((0, 1), (1, 0))):
                W.flows_classify(h.keys, 16, n, self.table.t, nb, h.flow)
                W.accept_data_packets_flows(h.ring, STRIDE, h.rl, h.flow, n, self.seq0[a], nf, w, self.img[a], self.sl[a], h.ok,
                                            h.place, h.ack)
                W.rx_build_acks_flows(h.ring, STRIDE, h.rl, h.flow, n, F.SELECTIVE, self.seq0[a], nf, w, h.ok, h.ack, h.wire, 16, 0,
                                      n, h.src, h.acnt, work=h.awork)
                W.rx_deliver_flows(self.img[a], self.sl[a], nf, w, w, h.stream.t, nf * w * MAXP, 0, h.offs, h.lens, h.adv, h.info,
                                   h.dcnt, work=h.dwork)
                W.rx_advance_flows(self.img[a], self.sl[a], nf, w, h.adv, self.seq0[a], self.img[b], self.sl[b], self.seq0[b])
                W.flows_control(h.ring, STRIDE, h.rl, h.keys, 16, h.flow, h.ok, n, self.table.t, nb, nf, w, self.flow_start.t,
                                self.seq0[b], self.sl[b], self.free.t, self.free_pos.t, h.cwire.t, 16, n, h.csrc.t, h.opened.t,
                                h.osrc.t, h.closed.t, h.verdict.t, h.ccnt.t, work=h.cwork)
                W.rx_digest_flows(h.stream.t, nf * w * MAXP, h.info, nf, self.crc.t, self.nb.t, h.opened.t, h.ccnt.t[2:], nf,
                                  h.closed.t, h.ccnt.t[3:], nf, d["rcrc"].t, d["rbytes"].t, d["counts"].t, work=d["work"][1:])

        def load(self, halves):
            for d in self.dig:
                d["rcrc"].t.fill_(SENT32)
                d["work"].random_(0, 256)
            super().load(halves)

        def read(self):
            out = super().read()
            self.reports.append([(d["rcrc"].get(), d["rbytes"].get(), d["counts"].get()) for d in self.dig])
            return out

    return DigestReceiver(W, graph)


def run_life_with_digests(seed, dev):
    """conn_model.run_life, half by half: the report entries of the flows a round closed are
    taken as the digests of the transfers that owned them.  Returns (life, {transfer: (crc,
    bytes)})."""
    life, digest = CM.Life(seed), {}
    while not life.done():
        halves = life.batches()
        results = dev.step(halves)
        for half, r, (rcrc, rbytes, counts) in zip(halves, results, dev.reports[-1]):
            owner = dict(life.owner)
            life.absorb([half], [r])
            nc = len(r["closed"])
            assert int(counts[3]) == nc and (rcrc[nc:] == SENT32).all()
            for q, f in enumerate(r["closed"]):
                assert owner[int(f)] not in digest
                digest[owner[int(f)]] = (int(rcrc[q]), int(rbytes[q]))
    life.check_finished()
    return life, digest


def check_digests(life, digest):
    assert sorted(digest) == list(range(CM.LIFE_TRANSFERS))  # every id was reused, and every connection reported once
    for j, t in enumerate(life.t):
        assert digest[j] == (O.crc32(t["data"]), t["data"].size), j


def test_connections_that_come_and_go(W):
    """Eight transfers over four flow ids with loss, wtp_flows_control in the loop: the report
    entry of each connection that closes carries its whole file's CRC and size, and a
    connection that reuses the id ends with its own."""
    dev = make_receiver(W)
    life, digest = run_life_with_digests(1, dev)
    check_digests(life, digest)
    dev.check_finished(life)
    assert_no_data_error(W)


# ---- 8. one graph for every round -----------------------------------------------------------------------
def test_the_seven_call_round_from_one_graph(W_noinit):
    """Both halves of a step, seven calls each, captured once with no wtp_init and replayed for
    every step of a run: the log and the digests are the eager run's."""
    eager_life, eager = run_life_with_digests(2, make_receiver(W_noinit))
    dev = make_receiver(W_noinit, graph=True)
    life, digest = run_life_with_digests(2, dev)
    assert life.log == eager_life.log and digest == eager
    check_digests(life, digest)
    assert_no_data_error(W_noinit)


class GraphCall:
    """A captured call on its own stream, state and scratch, for replay_each_then_together."""

    def __init__(self, W, host, stream, seed):
        self.W, self.host, self.mem = W, host, stream
        self.rng = np.random.default_rng(seed)
        self.c = Call(W, stream, [(0, 0)] * 40, reset=([0] * 6, 0, 4), report=([0] * 6, 0, 4), work_off=seed % 16)
        self.graph, self.stream = capture(self.c.run)

    def reset(self, salt):
        c, size = self.c, self.host.size
        b = self.rng.integers(0, size - 70000, c.nf)
        c.h_info = M.info_of(list(zip(b.tolist(), (self.rng.integers(0, 70000, c.nf) + salt).tolist())))
        c.h_crc = self.rng.integers(0, 1 << 32, c.nf, dtype=np.uint64).astype(np.uint32)
        c.h_bytes = self.rng.integers(0, 1 << 50, c.nf, dtype=np.uint64)
        c.info.t.copy_(torch.from_numpy(c.h_info.reshape(-1).view(np.int64)))
        c.crc.t.copy_(dev_s32(c.h_crc))
        c.bytes.t.copy_(torch.from_numpy(c.h_bytes.view(np.int64)))
        lists = []
        for spec in c.lists:
            ids, count = self.rng.integers(0, c.nf + 3, 6).astype(np.uint32), int(self.rng.integers(0, 6))
            spec[1].t.copy_(dev_s32(ids))
            spec[3].t.copy_(dev_s32([count]))
            lists.append((ids, spec[1], count, spec[3], spec[4]))
        c.lists = lists
        c.rcrc.t.fill_(SENT32)
        c.rbytes.t.fill_(SENT64)
        c.counts.t.fill_(SENT64)
        c.work.payload.random_(0, 256)

    def check(self):
        self.c.check(self.c.want(self.host), last=None)


def test_two_graphs_alone_and_together(W_noinit):
    host = np.random.default_rng(8).integers(0, 256, 300000, dtype=np.uint8)
    stream = Bytes(host, off=4, front=64, back=64)
    g = GraphCall(W_noinit, host, stream, 81)
    replay_each_then_together(g, [(0,), (1,)], lambda: (GraphCall(W_noinit, host, stream, 82), GraphCall(W_noinit, host, stream, 83)),
                              [(2,), (3,), (4,)])
    assert np.array_equal(stream.get(), host)


# ---- 9. a stream past 4 GiB --------------------------------------------------------------------------------
def test_wide_stream(W_noinit):
    """One stream of 4 GiB + 1 MiB: ranges that end just below, contain, and begin at or above
    2^31 and 2^32, and one of 2 GiB across both."""
    size = 4 * GIB + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < size + GIB // 2:
        pytest.skip(f"{free / GIB:.1f} GiB free, the test needs {size / GIB:.1f}")
    period = np.random.default_rng(9).integers(0, 256, 65521, dtype=np.uint8)
    stream = periodic(period, size, off=6)
    ranges = []
    for bound in BOUNDS:
        ranges += [(bound - 5000, 4000), (bound - 4097, 4097), (bound - 100, 5000), (bound - 1, 2), (bound, 3000), (bound + 1, 1),
                   (bound + 4096, 70000)]
    ranges += [((1 << 31) - 7, 2 * GIB + (1 << 20)), (1, size - 1), (size - 1, 1), (size, 0), (size + 1, 0)]  # one above 2^32 bytes

    def seg_crc(b, n):
        return periodic_crc(np.roll(period, -(b % period.size)), n)

    c = Call(W_noinit, stream, ranges)
    c.run()
    got = c.check(c.want(None, seg_crc))
    assert int(got[4][2]) == 1 and int(got[4][1]) == len(ranges) - 2
    stream.check_guards()
    assert_no_data_error(W_noinit)
