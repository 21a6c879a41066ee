"""GPU tests of the multi-connection receive, wtp_accept_data_packets_flows and
wtp_rx_build_acks_flows: every output of both calls is compared with tests/flows_model.py,
whose accept is accept_model.accept per flow, and for one flow with the single-connection
calls on the device.  Buffers are gpu_support's guarded ones and every output starts from a
sentinel, so a byte or word that must stay untouched is checkable.

Section 8 puts every payload length 0 .. 1484 once through k_flows_place, over three flows, on
the vector path and on the bytewise one (the inputs are tests/flows_cases.py's)."""
import numpy as np
import pytest

import accept_model
import flows_cases as C
import flows_model as F
import oracle as O
from gpu_support import W, W_noinit  # noqa: F401 (fixtures: W for verify's tables; the graph test takes W_noinit)
from gpu_support import (Bytes, Words, assert_bytes_equal, assert_no_data_error, capture, datagram_ring, dev_s32, s32, u32)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MAXP, STRIDE, EMPTY, M32, SENT = F.MAXP, F.STRIDE, F.EMPTY, F.M32, 12345
MODES = [F.SELECTIVE, F.CUMULATIVE]


class DevFlows:
    """The caller-owned state of wtp_accept_data_packets_flows on the device and its host copy:
    a 0xA5 image of nflows * window slots at byte `out_off` past a 16-B aligned address between
    64 guard bytes, and slot_len with guard words.  accept() uploads one batch (the ring at byte
    `ring_off` between guards, recv_len, flow, seq0) and sentinel-filled outputs, makes the call
    and the model's from the same entry state, compares all five outputs, every guard and the
    inputs, and carries the state over."""
    OK_SENT, PLACE_SENT, ACK_SENT = 7, 12345, 0x0BADACC0

    def __init__(self, nflows, window, out_off=0, slot_len=None):
        self.nflows, self.window = nflows, window
        slots = nflows * window
        self.h_out = np.full(slots * MAXP, 0xA5, dtype=np.uint8)
        self.h_sl = np.full(slots, EMPTY, np.uint32) if slot_len is None else np.array(slot_len, dtype=np.uint32)
        assert self.h_sl.size == slots
        self.img = Bytes(self.h_out, off=out_off, front=64, back=64)
        self.sl = Words(self.h_sl)

    def stage(self, ring, stride, rl, flow, seq0, ring_off=0):
        self.stride = stride
        self.ring = Bytes(ring, off=ring_off, front=64, back=64)
        self.h_rl, self.h_flow = np.array(rl, dtype=np.uint32), np.array(flow, dtype=np.uint32)
        self.h_seq0 = np.array(seq0, dtype=np.uint32)
        self.rl, self.fl, self.sq = Words(self.h_rl), Words(self.h_flow), Words(self.h_seq0)
        n = self.n = self.h_rl.size
        self.ok = Bytes(fill=self.OK_SENT, size=n, front=16, back=16)
        self.place, self.ack = Words(self.PLACE_SENT, n), Words(self.ACK_SENT, self.nflows)

    def call(self, W, with_place=True, with_ack=True, stream=None):
        W.accept_data_packets_flows(self.ring.t, self.stride, self.rl.t, self.fl.t, self.n, self.sq.t, self.nflows, self.window,
                                    self.img.t, self.sl.t, self.ok.t, self.place.t if with_place else None,
                                    self.ack.t if with_ack else None, stream=stream)

    def check(self, want, with_place=True, with_ack=True):
        want_ok, want_place, want_out, want_sl, want_ack = want
        n, w = self.n, self.window
        assert np.array_equal(self.ok.get(), want_ok)
        assert np.array_equal(self.place.get(), want_place if with_place else np.full(n, self.PLACE_SENT, np.uint32))
        assert np.array_equal(self.sl.get(), want_sl)
        assert_bytes_equal(self.img.get(), want_out, MAXP,
                           lambda s: f"flow {s // max(w, 1)} slot {s % max(w, 1)}, slot_len {want_sl[s]:#x}")
        assert np.array_equal(self.ack.get(), want_ack if with_ack else np.full(self.nflows, self.ACK_SENT, np.uint32))
        assert np.array_equal(self.ring.get(), self.ring.host)  # the inputs are only read
        assert np.array_equal(self.rl.get(), self.h_rl) and np.array_equal(self.fl.get(), self.h_flow)
        assert np.array_equal(self.sq.get(), self.h_seq0)

    def accept(self, W, ring, stride, rl, flow, seq0, ring_off=0, with_place=True, with_ack=True):
        """One call on the device and in the model; returns the model's result."""
        self.stage(ring, stride, rl, flow, seq0, ring_off)
        self.call(W, with_place, with_ack)
        torch.cuda.synchronize()
        want = F.accept_flows(ring, stride, rl, flow, seq0, self.nflows, self.window, self.h_out, self.h_sl)
        self.check(want, with_place, with_ack)
        if self.n or (with_ack and self.nflows):  # otherwise nothing is launched
            assert W.LIB.wtp_last_kernel().decode() == "k_flows_place"
        assert_no_data_error(W)
        self.want = want
        self.h_out, self.h_sl = want[2], want[3]
        return want


def acks(W, st, mode, skip=0, max_acks=None, ack_stride=16, ack_off=0, with_src=True, work_off=16, flow_ack=True):
    """One wtp_rx_build_acks_flows behind st.accept() on the device and in the model; asserts
    every output equal and every input and guard untouched; returns the model's result."""
    n = st.n
    max_acks = n if max_acks is None else max_acks
    cap = max_acks + 2  # two ring entries more than the call may use
    wbuf = torch.full((cap * ack_stride + ack_off + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    wire = wbuf[ack_off:ack_off + cap * ack_stride]
    src = Words(SENT, cap)
    cbuf = torch.full((6,), 0x77777777, dtype=torch.int32, device="cuda")
    need = W.rx_ack_flows_work_bytes(n)
    wkbuf = torch.randint(0, 256, (need + work_off + 16,), dtype=torch.uint8, device="cuda")
    before = wkbuf.clone()
    fa = Words(st.want[4])  # accept's d_ack, whether or not the call was given one
    W.rx_build_acks_flows(st.ring.t, st.stride, st.rl.t, st.fl.t, n, mode, st.sq.t, st.nflows, st.window, st.ok.t,
                          fa.t if flow_ack else None, wire, ack_stride, skip, max_acks, src.t if with_src else None, cbuf[2:4],
                          work=wkbuf[work_off:work_off + need])
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == "k_flows_ack_emit"
    seq, idx, (emitted, total) = F.build_acks_flows(st.ring.host, st.stride, st.h_rl, st.h_flow, mode, st.h_seq0, st.nflows,
                                                    st.window, st.want[0], st.want[4], skip=skip, max_acks=max_acks)
    assert u32(cbuf).tolist() == [0x77777777] * 2 + [emitted, total] + [0x77777777] * 2
    rows = wire.view(cap, ack_stride).cpu().numpy()
    assert np.array_equal(rows[:emitted, :16], F.A.ack_bytes(seq))
    assert (rows[emitted:] == 0xA5).all() and (rows[:, 16:] == 0xA5).all()  # past the count / the datagram
    assert (wbuf[:ack_off] == 0xA5).all() and (wbuf[wbuf.numel() - 16:] == 0xA5).all()
    want_src = np.concatenate([idx, np.full(cap - emitted, SENT, np.uint32)]) if with_src else np.full(cap, SENT, np.uint32)
    assert np.array_equal(src.get(), want_src)
    assert torch.equal(wkbuf[:work_off], before[:work_off]) and torch.equal(wkbuf[work_off + need:], before[work_off + need:])
    # every input is only read
    assert np.array_equal(st.ring.get(), st.ring.host) and np.array_equal(st.ok.get(), st.want[0])
    assert np.array_equal(st.rl.get(), st.h_rl) and np.array_equal(st.fl.get(), st.h_flow)
    assert np.array_equal(st.sq.get(), st.h_seq0) and np.array_equal(fa.get(), st.want[4])
    assert_no_data_error(W)
    return seq, idx, (emitted, total)


# ---- 1. edges ------------------------------------------------------------------------------------
EDGE_LENS = (0, 1, 15, 16, 17, 1455, 1456)
EDGE_SEQ0 = (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF)  # three windows of 5 that wrap 2^32 and share 0xFFFFFFFF, 0, 1


def edge_batch():
    """(datagrams, recv_len overrides, flow, prefilled slot_len) of the edge test: 3 flows x
    window 5, every length of EDGE_LENS placed, and one datagram or more of every way not to
    be placed."""
    rng = np.random.default_rng(0xED6E)
    nflows, window = 3, 5
    sl = np.full(nflows * window, EMPTY, np.uint32)
    sl[0 * window + 1], sl[2 * window + 0] = 7, 0  # filled before: a length and an empty payload
    d, flow, cut = [], [], {}

    def add(f, seq, ln, ptype=2, damage=None):
        g = bytearray(O.build_datagram(seq & M32, rng.integers(0, 256, ln, dtype=np.uint8).tobytes(), ptype=ptype))
        if damage == "payload":
            g[16 + ln // 2] ^= 0x10
        elif damage == "crc":
            g[13] ^= 0x01
        elif damage == "runt":
            cut[len(d)] = 12
        d.append(bytes(g))
        flow.append(f)

    lens = iter(EDGE_LENS * 6)
    for f in range(nflows):  # the same seqNum, 0, in all three flows: three different slots
        add(f, 0, next(lens))
    for _ in range(3):  # three intact duplicates with different payloads and lengths: the first wins
        add(1, 1, next(lens))
    add(0, EDGE_SEQ0[0] + 1, 16)        # its slot was filled before the batch
    add(2, EDGE_SEQ0[2], 1456)          # the same, over an empty payload
    add(0, EDGE_SEQ0[0] + 4, next(lens))  # the last slot of a window, past the wrap
    add(1, EDGE_SEQ0[1], next(lens))      # the first slot, before the wrap
    add(2, EDGE_SEQ0[2] + 2, 1456, damage="payload")
    add(2, EDGE_SEQ0[2] + 2, 17, damage="crc")
    add(2, EDGE_SEQ0[2] + 2, 15, damage="runt")
    for t in (0, 1, 3):
        add(1, EDGE_SEQ0[1] + 4, next(lens), ptype=t)
    add(1, EDGE_SEQ0[1] + 4, 1457)        # a payload above 1456
    add(0, EDGE_SEQ0[0] + 2, 16, damage=None)
    add(nflows, EDGE_SEQ0[0] + 3, 17)     # no connection: flow ids nflows and 0xFFFFFFFF
    add(F.NO_FLOW, EDGE_SEQ0[0] + 3, 1456)
    add(0, EDGE_SEQ0[0] - 1, 1)           # below the window
    add(0, EDGE_SEQ0[0] + 5, 1)           # at its end
    add(2, EDGE_SEQ0[2] + 2, next(lens))  # placed after the corrupt ones for the same slot
    add(2, EDGE_SEQ0[2] + 3, next(lens))
    add(2, EDGE_SEQ0[2] + 4, next(lens))
    add(1, EDGE_SEQ0[1] + 1, next(lens))
    add(0, EDGE_SEQ0[0], next(lens))
    add(1, EDGE_SEQ0[1] + 4, next(lens))  # after the other types and the long one for the same slot
    add(0, 0, 1455)                       # duplicates of the first three, each in its own flow
    add(1, 0, 16)
    add(2, 0, 0)
    add(1, EDGE_SEQ0[1] + 5, 1456)        # past the end of flow 1 (inside flow 2's numbers)
    add(2, EDGE_SEQ0[2] - 2, 15)          # below flow 2 (inside flow 0's numbers)
    add(1, 1, 1455)                       # a fourth arrival for the slot of the three duplicates
    add(nflows + 5, 0, 16)                # no connection
    add(0, EDGE_SEQ0[0] + 2, 0, ptype=1)  # an END for a filled slot
    add(2, 0, 17, damage="crc")           # corrupt duplicates
    add(1, 0, 1456, damage="payload")
    add(0, EDGE_SEQ0[0], 1456)            # a full-size duplicate
    return d, cut, np.array(flow, np.uint32), sl, nflows, window


@pytest.mark.parametrize("stride,ring_off,out_off", [(1488, 0, 0), (1500, 1, 3)], ids=["vector", "bytewise"])
def test_edges(W, stride, ring_off, out_off):
    d, cut, flow, sl, nflows, window = edge_batch()
    assert 36 <= len(d) <= 44
    ring, rl = datagram_ring(d, stride)
    for i, v in cut.items():
        rl[i] = v
    st = DevFlows(nflows, window, out_off=out_off, slot_len=sl)
    ok, place, _, sl_after, ack = st.accept(W, ring, stride, rl, flow, EDGE_SEQ0, ring_off=ring_off)
    assert (st.ring.t.data_ptr() + 16) % 16 == ring_off and st.img.t.data_ptr() % 16 == out_off
    # the batch is what it was made to be
    placed = place != F.NOT_PLACED
    assert set(EDGE_LENS) == set((rl[placed] - 16).tolist()) and (sl_after != EMPTY).all()  # every window fills up
    assert ack.tolist() == [(s + window) & M32 for s in EDGE_SEQ0]
    assert placed.sum() == 13 and placed[:4].all() and not placed[4:6].any() and (ok == 0).sum() == 5
    assert ok[flow >= nflows].all() and (flow >= nflows).sum() == 3
    for mode in MODES:
        seq, idx, (e, total) = acks(W, st, mode)
        assert e == total and 20 < e < len(d)
        acks(W, st, mode, skip=3, max_acks=e - 7, ack_stride=20, ack_off=1, work_off=1, with_src=False)
    # the calls again without the optional outputs
    st2 = DevFlows(nflows, window, out_off=out_off, slot_len=sl)
    st2.accept(W, ring, stride, rl, flow, EDGE_SEQ0, ring_off=ring_off, with_place=False, with_ack=False)
    acks(W, st2, F.SELECTIVE, flow_ack=False)


# ---- 2. more than one workgroup --------------------------------------------------------------------
def test_more_than_one_workgroup(W):
    """600 datagrams over 4 flows x window 160: claims and copy groups span blocks, first-wins
    duplicates sit at indices 0, 300 and 599, and flow 3, which no datagram names, still gets
    its ACK from its prefilled state."""
    rng = np.random.default_rng(600)
    n, nflows, window = 600, 4, 160
    seq0 = np.array([5, 0xFFFFFF80, 5, 9000], np.uint32)
    sl = np.full(nflows * window, EMPTY, np.uint32)
    sl[3 * window:3 * window + 7] = 100
    sl[3 * window + 20] = 3
    sl[0:3], sl[window + 1] = 1456, 0
    flow = rng.integers(0, 3, n).astype(np.uint32)
    slot = (window * rng.random(n) ** 2).astype(np.int64)  # low slots mostly: leading runs and duplicates
    lens = rng.choice([0, 1, 16, 40, 333, 1456], n)
    for i in (0, 300, 599):
        flow[i], slot[i], lens[i] = 2, 150, (1456, 40, 333)[i % 3]
    d = [O.build_datagram((int(seq0[flow[i]]) + int(slot[i])) & M32, rng.integers(0, 256, lens[i], dtype=np.uint8).tobytes())
         for i in range(n)]
    ring, rl = datagram_ring(d, STRIDE)
    st = DevFlows(nflows, window, slot_len=sl)
    ok, place, _, sl_after, ack = st.accept(W, ring, STRIDE, rl, flow, seq0)
    assert ok.all() and place[0] == 150 and place[300] == place[599] == F.NOT_PLACED and sl_after[2 * window + 150] == 1456
    assert int(ack[3]) == 9007 and all(0 < ((int(ack[f]) - int(seq0[f])) & M32) < window for f in range(3))
    assert 100 < (place != F.NOT_PLACED).sum() < n - 100
    for mode in MODES:
        _, _, (e, total) = acks(W, st, mode)
        assert e == total == n


@pytest.mark.parametrize("nflows,window", [(100_000, 3), (1, 300_000), (7, 42_857)])
def test_ack_scan_takes_more_than_one_turn(W, nflows, window):
    """About 300 000 slots are more than the 1024 x 256 lanes the per-flow ACK scan is capped
    at, so a lane looks at a second slot: many windows of 3 slots, one window, and windows that
    no wave boundary lines up with.  Every flow has a leading run of its own, other slots filled
    behind a gap, and 64 datagrams extend some of the runs.  The image is not compared as a
    whole (it is 437 MB): the placed payloads are, with slot_len, d_place, d_ok and every ACK."""
    rng = np.random.default_rng(nflows)
    slots, n = nflows * window, 64
    assert slots > 1024 * 256
    lead = rng.integers(0, window + 1, nflows)
    s = np.arange(window)[None, :]
    filled = (s < lead[:, None]) | ((s > lead[:, None]) & (rng.random((nflows, window)) < 0.3))
    sl = np.where(filled, 5, EMPTY).astype(np.uint32).reshape(-1)
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    flow = rng.integers(0, nflows, n).astype(np.uint32)
    flow[:8] = (0, nflows - 1, nflows // 2, 0, nflows - 1, nflows // 2, 0, 0)
    behind = lead[flow] + rng.integers(0, window, n) % np.maximum(window - lead[flow], 1)  # at or behind the run's end
    slot = np.minimum(np.where(rng.random(n) < 0.6, lead[flow], behind), window - 1)
    pay = [rng.integers(0, 256, int(rng.choice([0, 1, 16, 100, 1456])), dtype=np.uint8) for _ in range(n)]
    ring, rl = datagram_ring([O.build_datagram((int(seq0[flow[i]]) + int(slot[i])) & M32, pay[i].tobytes()) for i in range(n)],
                             STRIDE)
    want_sl, want_place = sl.copy(), np.full(n, F.NOT_PLACED, np.uint32)
    for i in range(n):  # the sequential loop, on the slots the batch touches
        g = int(flow[i]) * window + int(slot[i])
        if want_sl[g] == EMPTY:
            want_sl[g], want_place[i] = pay[i].size, slot[i]
    run = np.cumprod(want_sl.reshape(nflows, window) != EMPTY, axis=1).sum(axis=1)
    want_ack = ((seq0.astype(np.int64) + run) & M32).astype(np.uint32)
    assert (want_place != F.NOT_PLACED).sum() > 10 and (run > lead).sum() >= min(3, nflows)

    img = torch.empty(slots * MAXP, dtype=torch.uint8, device="cuda")
    d_ring, d_rl, d_flow, d_seq0, d_sl = Bytes(ring), Words(rl), Words(flow), Words(seq0), Words(sl)
    ok, place, ack = Bytes(fill=7, size=n, front=16, back=16), Words(SENT, n), Words(SENT, nflows)
    W.accept_data_packets_flows(d_ring.t, STRIDE, d_rl.t, d_flow.t, n, d_seq0.t, nflows, window, img, d_sl.t, ok.t, place.t,
                                ack.t)
    torch.cuda.synchronize()
    assert ok.get().all() and np.array_equal(place.get(), want_place) and np.array_equal(d_sl.get(), want_sl)
    got_ack = ack.get()
    bad = np.flatnonzero(got_ack != want_ack)
    assert bad.size == 0, (bad[:5], got_ack[bad[:5]], want_ack[bad[:5]])
    for i in np.flatnonzero(want_place != F.NOT_PLACED):
        g = int(flow[i]) * window + int(slot[i])
        assert np.array_equal(img[g * MAXP:g * MAXP + pay[i].size].cpu().numpy(), pay[i]), i
    assert np.array_equal(d_ring.get(), ring) and np.array_equal(d_seq0.get(), seq0) and np.array_equal(d_flow.get(), flow)
    assert_no_data_error(W)


# ---- 3. one flow is the single-connection calls ----------------------------------------------------
@pytest.mark.parametrize("seed", [1, 4])
def test_single_flow_identity(W, seed):
    """nflows == 1, device against device: d_out, d_slot_len, d_ok, d_place and d_ack are those of
    wtp_accept_data_packets, selective ACK rings those of wtp_rx_build_acks, also with skip > 0
    and max_acks below the eligible count."""
    rng, window, seq0, stride, ring_off, out_off, ns = accept_model.fuzz_case(seed)
    one = DevFlows(1, window, out_off=out_off)
    ref_img, ref_sl = Bytes(one.h_out, off=out_off, front=64, back=64), Words(one.h_sl)
    for n in ns:
        ring, rl, _ = accept_model.fuzz_batch(rng, seq0, window, stride, one.h_sl, n)
        want = one.accept(W, ring, stride, rl, np.zeros(n, np.uint32), [seq0], ring_off=ring_off)
        ok, place, ack = Bytes(fill=7, size=n, front=16, back=16), Words(SENT, n), Words(0, 1)
        W.accept_data_packets(one.ring.t, stride, one.rl.t, n, seq0, window, ref_img.t, ref_sl.t, ok.t, place.t, ack.t)
        torch.cuda.synchronize()
        assert np.array_equal(ref_img.get(), one.img.get()) and np.array_equal(ref_sl.get(), one.sl.get())
        assert np.array_equal(ok.get(), one.ok.get()) and np.array_equal(place.get(), one.place.get())
        assert np.array_equal(ack.get(), one.ack.get())
        _, _, (e, _) = acks(W, one, F.SELECTIVE)
        for skip, max_acks in ((0, n), (3, max(e - 5, 0))):
            cap = max_acks + 2
            rings, srcs, counts = [], [], []
            for flows_call in (False, True):
                wire = torch.full((cap, 16), 0xA5, dtype=torch.uint8, device="cuda")
                src, cnt = Words(SENT, cap), Words(0x77777777, 2)
                if flows_call:
                    W.rx_build_acks_flows(one.ring.t, stride, one.rl.t, one.fl.t, n, F.SELECTIVE, one.sq.t, 1, window,
                                          one.ok.t, None, wire, 16, skip, max_acks, src.t, cnt.t)
                else:
                    W.rx_build_acks(one.ring.t, stride, one.rl.t, n, F.SELECTIVE, seq0, window, ok.t, None, None, wire, 16,
                                    skip, max_acks, src.t, cnt.t)
                torch.cuda.synchronize()
                rings.append(wire.cpu().numpy()), srcs.append(src.get()), counts.append(cnt.get())
            assert np.array_equal(rings[0], rings[1]) and np.array_equal(srcs[0], srcs[1])
            assert np.array_equal(counts[0], counts[1]) and (n == 0 or counts[0][1] == e)
        assert want[4].tolist() == ack.get().tolist()
    assert_no_data_error(W)


# ---- 4. degenerate shapes ----------------------------------------------------------------------------
def _small_batch(rng, n, flow, seq0, window, stride=STRIDE):
    """n intact DATA datagrams of 0 .. 40 bytes for slots -2 .. window + 1 of their flows."""
    d = []
    for i in range(n):
        base = int(seq0[flow[i]]) if flow[i] < len(seq0) else 0
        ln = int(rng.integers(0, 41))
        d.append(O.build_datagram((base + int(rng.integers(-2, window + 2))) & M32,
                                  rng.integers(0, 256, ln, dtype=np.uint8).tobytes()))
    return datagram_ring(d, stride)


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_shapes(W, mode):
    rng = np.random.default_rng(44 + mode)
    seq0 = np.array([0xFFFFFFFF, 50], np.uint32)
    # n == 0: every flow's ACK from the existing state, counts {0, 0}
    sl = np.full(2 * 6, EMPTY, np.uint32)
    sl[0:2], sl[6 + 1] = 9, 9
    st = DevFlows(2, 6, slot_len=sl)
    want = st.accept(W, np.zeros(0, np.uint8), STRIDE, np.zeros(0, np.uint32), np.zeros(0, np.uint32), seq0)
    assert want[4].tolist() == [1, 50]
    assert acks(W, st, mode)[2] == (0, 0)
    st.accept(W, np.zeros(0, np.uint8), STRIDE, np.zeros(0, np.uint32), np.zeros(0, np.uint32), seq0, with_ack=False)
    # nflows == 0: every datagram is verified, none has a connection
    flow = rng.integers(0, 2, 30).astype(np.uint32)
    ring, rl = _small_batch(rng, 30, flow, seq0, 6)
    st = DevFlows(0, 6)
    want = st.accept(W, ring, STRIDE, rl, flow, seq0)
    assert want[0].all() and (want[1] == F.NOT_PLACED).all()
    assert acks(W, st, mode)[2] == (0, 0)
    # window == 0: nothing is placed, every ACK is the flow's base, only datagrams below it are answered
    st = DevFlows(2, 0)
    want = st.accept(W, ring, STRIDE, rl, flow, seq0)
    assert (want[1] == F.NOT_PLACED).all() and want[4].tolist() == seq0.tolist()
    _, _, (e, total) = acks(W, st, mode)
    assert 0 < e == total < 30
    # max_acks == 0: the counts are still written; NULL d_place / d_ack / d_src
    st = DevFlows(2, 6, slot_len=sl)
    st.accept(W, ring, STRIDE, rl, flow, seq0, with_place=False, with_ack=False)
    _, _, (e, total) = acks(W, st, mode, max_acks=0, with_src=False)
    assert e == 0 and total > 15
    acks(W, st, mode, with_src=False)


# ---- 5. the corpus -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(F.FUZZ_SEEDS))
def test_fuzz(W, seed):
    """The model's corpus (tests/test_flows_model.py asserts what it contains): successive calls
    on one state, both ACK modes behind each."""
    calls, (nflows, window, seq0, stride, ring_off, out_off) = F.fuzz_calls(seed)
    st = DevFlows(nflows, window, out_off=out_off)
    for k, c in enumerate(calls):
        want = st.accept(W, c["ring"], stride, c["rl"], c["flow"], seq0, ring_off=ring_off)
        assert all(np.array_equal(a, b) for a, b in zip(want, c["want"]))
        for mode in MODES:
            _, _, (e, total) = acks(W, st, mode, ack_stride=(16, 24)[k % 2], ack_off=(0, 1)[seed % 2])
            assert e == total > nflows


# ---- 6. one graph for every round ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_graph_replay(W_noinit, mode):
    """accept_flows + acks_flows captured once with no wtp_init before it, and replayed for two
    rounds with d_seq0 and the batch buffers rewritten on the device in between: each replay is
    the model's result for that round's inputs on the state the round before left."""
    W = W_noinit
    nflows, window, n = 3, 40, 200
    rng = np.random.default_rng(0x6EA + mode)
    z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt, device="cuda")  # noqa: E731
    d_ring, d_rl, d_flow, d_seq0 = z(n * STRIDE, torch.uint8), z(n), z(n), z(nflows)
    img = torch.full((nflows * window * MAXP,), 0xA5, dtype=torch.uint8, device="cuda")
    sl = torch.full((nflows * window,), -1, dtype=torch.int32, device="cuda")
    ok, place, ack = z(n, torch.uint8), z(n), z(nflows)
    wire, src, counts = z(n * 16, torch.uint8), z(n), z(2)
    work = z(W.rx_ack_flows_work_bytes(n), torch.uint8)

    def call():
        W.accept_data_packets_flows(d_ring, STRIDE, d_rl, d_flow, n, d_seq0, nflows, window, img, sl, ok, place, ack)
        W.rx_build_acks_flows(d_ring, STRIDE, d_rl, d_flow, n, mode, d_seq0, nflows, window, ok, ack, wire, 16, 0, n, src,
                              counts, work=work)

    def load(seq0):
        flow = rng.integers(0, nflows + 1, n).astype(np.uint32)  # nflows: no connection
        d = []
        for i in range(n):
            ln = int(rng.choice([0, 5, 16, 100, 1456]))
            g = bytearray(O.build_datagram((int(seq0[min(flow[i], nflows - 1)]) + int(rng.integers(-3, window // 2))) & M32,
                                           rng.integers(0, 256, ln, dtype=np.uint8).tobytes()))
            if rng.random() < 0.1:
                g[12] ^= 0x80
            d.append(bytes(g))
        ring, rl = datagram_ring(d, STRIDE)
        d_ring.copy_(torch.from_numpy(ring))
        d_rl.copy_(dev_s32(rl))
        d_flow.copy_(dev_s32(flow))
        d_seq0.copy_(dev_s32(seq0))
        for t, v in ((ok, 7), (place, SENT), (ack, SENT), (wire, 0xA5), (src, SENT), (counts, 0x77777777)):
            t.fill_(v)
        work.random_(0, 256)
        return ring, rl, flow

    h_out, h_sl = np.full(nflows * window * MAXP, 0xA5, np.uint8), np.full(nflows * window, EMPTY, np.uint32)
    seq0 = np.array([0xFFFFFFF0, 7, 7], np.uint32)
    load(seq0)
    graph, stream = capture(call)
    img.fill_(0xA5)  # the state the rounds start from: what the capture's own run left is dropped
    sl.fill_(-1)
    for rnd in range(2):
        ring, rl, flow = load(seq0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        w_ok, w_place, h_out, h_sl, w_ack = F.accept_flows(ring, STRIDE, rl, flow, seq0, nflows, window, h_out, h_sl)
        assert np.array_equal(ok.cpu().numpy(), w_ok) and np.array_equal(u32(place), w_place)
        assert np.array_equal(u32(sl), h_sl) and np.array_equal(u32(ack), w_ack)
        assert_bytes_equal(img.cpu().numpy(), h_out, MAXP, f"round {rnd}")
        seq, idx, (e, total) = F.build_acks_flows(ring, STRIDE, rl, flow, mode, seq0, nflows, window, w_ok, w_ack)
        assert tuple(u32(counts)) == (e, total) and e > n // 3
        rows = wire.view(n, 16).cpu().numpy()
        assert np.array_equal(rows[:e], F.A.ack_bytes(seq)) and (rows[e:] == 0xA5).all()
        assert np.array_equal(u32(src), np.concatenate([idx, np.full(n - e, SENT, np.uint32)]))
        # the next round: every flow's base moves by its leading run, as deliver -> advance would move it
        lead = (w_ack.astype(np.int64) - seq0) & M32
        assert lead.sum() > 0
        for f in range(nflows):
            a = int(lead[f])
            lo = f * window
            h_out[lo * MAXP:(lo + window - a) * MAXP] = h_out[(lo + a) * MAXP:(lo + window) * MAXP].copy()
            h_sl[lo:lo + window - a] = h_sl[lo + a:lo + window].copy()
            h_sl[lo + window - a:lo + window] = EMPTY
        img.copy_(torch.from_numpy(h_out))
        sl.copy_(dev_s32(h_sl))
        seq0 = ((seq0.astype(np.int64) + lead) & M32).astype(np.uint32)
    assert_no_data_error(W)


# ---- 7. four connections through one receiver --------------------------------------------------------------
class DevFlowsEnd:
    """Both ends of flows_model.transfer on the device: per sender the existing
    wtp_tx_build_retransmit_var, wtp_tx_ingest_acks and wtp_tx_advance over two (acked, sent_ms)
    pairs; one accept_flows + acks_flows for all arrivals; per flow the existing wtp_rx_deliver and
    wtp_rx_advance on its sub-window of two (img, slot_len) states.  The channels are index
    selections over the wire and the ACK ring; the host reads back selections, counts, d_src and
    the per-flow ACKs."""

    def __init__(self, W, nflows=F.XFER_FLOWS, window=F.XFER_WINDOW):
        self.W, self.nflows, self.window = W, nflows, window
        w = window
        z = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        self.rec = [F.xfer_records(f) for f in range(nflows)]
        self.base = [torch.from_numpy(r[3]).cuda() for r in self.rec]
        self.o = [torch.from_numpy(r[1].view(np.int64)).cuda() for r in self.rec]
        self.l = [dev_s32(r[0]) for r in self.rec]
        fill0 = int(s32([(F.XFER_NOW0 - F.XFER_TIMEOUT - 1) & M32])[0])
        self.acked = [[z(w), z(w)] for _ in range(nflows)]
        self.sent = [[z(w, fill0), z(w, fill0)] for _ in range(nflows)]
        self.wire = torch.full((nflows * w, STRIDE), 0xA5, dtype=torch.uint8, device="cuda")
        self.wl, self.sel, self.txc, self.adv = z(nflows * w), z(w), z(2), z(2)
        self.txwork = torch.empty(W.tx_work_bytes(w, w), dtype=torch.uint8, device="cuda")
        self.img = [torch.full((nflows * w * MAXP,), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.sl = [z(nflows * w, -1) for _ in range(2)]
        self.seq0, self.ack, self.counts = z(nflows), z(nflows), z(2)
        self.file = [Bytes(fill=0xA5, size=r[2], front=64, back=64, guard=0xA5) for r in self.rec]
        self.dcounts = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.offs_out, self.lens_out = torch.zeros(w, dtype=torch.int64, device="cuda"), z(w)
        self.dwork = torch.empty(W.rx_deliver_work_bytes(w), dtype=torch.uint8, device="cuda")
        self.offs, self.lens = [[] for _ in range(nflows)], [[] for _ in range(nflows)]

    def seq(self, f, chunk):
        return (F.XFER_SEQ[f] + chunk) & M32

    def emit(self, f, sbase, inflight, now, timeout):
        w = self.window
        self.W.tx_build_retransmit_var(self.base[f], self.rec[f][2], self.o[f][sbase:], self.l[f][sbase:], self.seq(f, sbase),
                                       inflight, self.acked[f][0], self.sent[f][0], now, timeout, 0, self.wire[f * w:(f + 1) * w],
                                       STRIDE, w, self.sel, self.wl[f * w:(f + 1) * w], None, self.txc, work=self.txwork)
        torch.cuda.synchronize()
        return u32(self.sel[:int(u32(self.txc)[0])])

    def receive(self, gidx, flow, rbase, mode):
        W, w, nf, n = self.W, self.window, self.nflows, gidx.size
        pick = torch.from_numpy(gidx).cuda()
        self.ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        ring = self.wire[pick].contiguous() if n else self.ok  # n == 0: any pointer
        rl = self.wl[pick].contiguous() if n else self.counts
        d_flow = dev_s32(flow) if n else self.counts
        self.seq0.copy_(dev_s32([self.seq(f, rbase[f]) for f in range(nf)]))  # rewritten between rounds
        self.ack_ring = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device="cuda")
        src = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        W.accept_data_packets_flows(ring, STRIDE, rl, d_flow, n, self.seq0, nf, w, self.img[0], self.sl[0], self.ok, None,
                                    self.ack)
        W.rx_build_acks_flows(ring, STRIDE, rl, d_flow, n, mode, self.seq0, nf, w, self.ok, self.ack, self.ack_ring, 16, 0, n,
                              src, self.counts)
        torch.cuda.synchronize()
        e, total = (int(c) for c in u32(self.counts))
        assert bool(self.ok[:n].all()) and e == total == n  # every arrival is intact and answered
        return u32(self.ack), u32(src[:e])

    def flush(self, f, off):
        W, w = self.W, self.window
        img, sl = self.img[0][f * w * MAXP:(f + 1) * w * MAXP], self.sl[0][f * w:(f + 1) * w]
        W.rx_deliver(img, sl, w, w, self.file[f].t, self.rec[f][2], off, self.offs_out, self.lens_out, self.dcounts,
                     work=self.dwork)
        W.rx_advance(img, sl, w, self.dcounts, self.img[1][f * w * MAXP:(f + 1) * w * MAXP], self.sl[1][f * w:(f + 1) * w])
        torch.cuda.synchronize()
        k, run, pk, prun = (int(c) for c in self.dcounts.cpu().numpy().view(np.uint64))
        assert k == run and pk == prun
        self.offs[f] += self.offs_out[:k].cpu().numpy().view(np.uint64).tolist()
        self.lens[f] += u32(self.lens_out[:k]).tolist()
        return k, pk

    def flushed(self):
        self.img.reverse()
        self.sl.reverse()

    def ingest(self, f, aidx, mode, sbase, inflight, fill_ms):
        W, w, na = self.W, self.window, aidx.size
        aok = torch.zeros(max(na, 1), dtype=torch.uint8, device="cuda")
        acks_ = self.ack_ring[torch.from_numpy(aidx).cuda()].contiguous() if na else aok  # na == 0: any pointer
        arl = torch.full((max(na, 1),), 16, dtype=torch.int32, device="cuda")
        W.tx_ingest_acks(acks_, 16, arl, na, mode, self.seq(f, sbase), inflight, self.acked[f][0], aok, None, self.adv)
        W.tx_advance(self.acked[f][0], self.sent[f][0], w, self.adv, fill_ms, self.acked[f][1], self.sent[f][1])
        self.acked[f].reverse()
        self.sent[f].reverse()
        torch.cuda.synchronize()
        assert bool(aok[:na].all())
        return int(u32(self.adv)[0])


@pytest.mark.parametrize("mode", MODES)
def test_transfer_of_four_connections(W, mode):
    """4 senders of 40 mixed-length records, window 8, through a lossy, duplicating, reordering
    channel into one receiver that serves all four with one accept_flows + acks_flows per round:
    every round's selections, ACKs, flushes and advances are the model loop's, and the four
    delivered streams, offsets and lengths are the sources'."""
    want, stats = F.transfer(F.ModelEnd(), mode)
    assert (stats >= 1).all()
    end = DevFlowsEnd(W)
    got, _ = F.transfer(end, mode)
    assert got == want and len(got) <= F.XFER_MAX_ROUNDS
    for f in range(F.XFER_FLOWS):
        lens, offs, total, host = end.rec[f]
        assert np.array_equal(end.file[f].get(), host)  # between 64 guard bytes on both sides
        assert np.array_equal(np.array(end.offs[f], np.uint64), offs) and np.array_equal(np.array(end.lens[f], np.uint32), lens)
        crc = torch.zeros(1, dtype=torch.int32, device="cuda")
        W.crc32_buffer(end.file[f].t, total, crc)
        assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)


# ---- 8. every length through the copy -----------------------------------------------------------------------
@pytest.mark.parametrize("stride,ring_off,out_off", [(1488, 0, 0), (1504, 0, 0), (1500, 1, 3)],
                         ids=["vector-1488", "vector-1504", "bytewise"])
def test_every_length(W, stride, ring_off, out_off):
    """The counterpart of test_gpu_accept.py::test_every_length for k_flows_place, this unit's own
    copy (16 lanes per datagram: a strided vector loop, the 1456-byte case, a tail of one byte per
    lane): one datagram of every payload length 0 .. 1484, dealt round-robin to 3 flows of window
    500 and shuffled.  Up to 1456 bytes are placed, with bytes [len, 1456) of the slot untouched;
    1457 .. 1484 are intact where the ring slot holds them (a 1488-byte slot holds 1472 payload
    bytes: the longer ones are cut by the ring and not ok) and not placed.  Aligned ring and
    image take the vector path; ring at +1 and image at +3 the bytewise one."""
    ring, rl, flow, seq0, order = C.accept_case(stride)
    st = DevFlows(3, 500, out_off=out_off)
    ok, place, out, sl, ack = st.accept(W, ring, stride, rl, flow, seq0, ring_off=ring_off)
    assert (st.ring.t.data_ptr() + 16) % 16 == ring_off and st.img.t.data_ptr() % 16 == out_off
    fits = order + 16 <= stride
    assert np.array_equal(ok != 0, fits) and fits[order <= 1472].all() and (stride == 1488 or fits.all())
    assert np.array_equal(place, np.where(order <= MAXP, order // 3, F.NOT_PLACED))
    assert ack.tolist() == [(int(s) + a) & M32 for s, a in zip(seq0, (486, 486, 485))]
    img = out.reshape(1500, MAXP)
    for ln in range(MAXP + 1):
        g = (ln % 3) * 500 + ln // 3
        assert sl[g] == ln and (img[g, ln:] == 0xA5).all(), ln
