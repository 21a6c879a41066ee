"""GPU tests of the multi-connection sender (include/wtp_crc32.h: wtp_tx_ingest_acks_flows,
wtp_tx_advance_flows, wtp_tx_build_retransmit_var_flows) against tests/txflows_model.py: the
fuzz corpus in both ACK modes, the single-flow identity with the three single-window calls,
windows whose boundaries fall inside a wave and inside a 1024-slot block, an emitted set large
enough for a round size above one, the bytewise paths, offsets above 2^32, a sender graph
captured once and replayed over states whose bases only the device writes, and the whole
transfer with seven calls per round.  Every output lies between guards and is compared whole,
and so is the state a call must not touch.

Section 9 gives the unit's own copies of the single-window bodies the edge suite those bodies
have: k_txf_emit at every length 0 .. 1456 and source phase with five due patterns and four
ring sizes on the vector and the bytewise path, on each side of every change of its round size
(g = 0 .. 6) and with 400 000 records (a second round per wave); k_txf_count / k_txf_select at
S = 2^20 (1024 block counts) and S = 65 537 (65) with sparse due sets and a cut inside a flow;
txf_due across the clock's wrap, at timeout 0 and 0xFFFFFFFF, with timers in the future, with
and without WTP_RETX_ALL; k_txf_ingest with 70 000 ACKs over some 280 workgroups and 20 000 on
one flow; k_txf_advance by 0, 1, window - 1, window, window + 1 and 0xFFFFFFFF at windows around
64, 256 and 1024 with wrapping bases, and at 2^20 slots.  Its inputs are tests/flows_cases.py's."""
import functools

import numpy as np
import pytest

import buildvar_model
import flows_cases as C
import flows_model as F
import oracle as O
import retx_model as R
import txflows_model as T
from gpu_support import (Batch, Bytes, W, W_noinit, Words, assert_bytes_equal, assert_no_data_error, capture, dev_s32,  # noqa: F401
                         periodic, s32, torch, u32)

pytestmark = pytest.mark.gpu
MAXP, STRIDE, M32 = T.MAXP, T.STRIDE, T.M32
MODES = (T.SELECTIVE, T.CUMULATIVE)
JUNK = 0x77777777


# ---- one call on the device and in the model -------------------------------------------------
def ingest(W, ring, stride, rl, flow, mode, seq0, rec0, rec_end, nflows, window, acked, with_hit=True, ring_off=0,
           model=T.ingest_flows):
    """wtp_tx_ingest_acks_flows against the model; returns the model's (ok, hit, acked, adv, fresh)."""
    want = model(ring, stride, rl, flow, mode, seq0, rec0, rec_end, nflows, window, acked)
    n = len(rl)
    d_ring = Bytes(ring if n else np.zeros(16, np.uint8), off=ring_off, front=64, back=64)
    ins = [Words(a) for a in (rl, flow, seq0, rec0, rec_end)]
    d_acked, d_ok = Words(acked), Bytes(fill=7, size=n, front=16, back=16)
    d_hit, d_adv, d_fresh = Words(12345, n), Words(0xADADAD, nflows), Words(0xF4F4F4, nflows)
    W.tx_ingest_acks_flows(d_ring.t, stride, ins[0].t, ins[1].t, n, mode, ins[2].t, ins[3].t, ins[4].t, nflows, window, d_acked.t,
                           d_ok.t, d_hit.t if with_hit else None, d_adv.t, d_fresh.t)
    torch.cuda.synchronize()
    assert np.array_equal(d_ok.get(), want[0])
    assert np.array_equal(d_hit.get(), want[1] if with_hit else np.full(n, 12345, np.uint32))
    assert np.array_equal(d_acked.get(), want[2])
    assert np.array_equal(d_adv.get(), want[3]) and np.array_equal(d_fresh.get(), want[4])
    for d, h in zip(ins, (rl, flow, seq0, rec0, rec_end)):  # the inputs are only read
        assert np.array_equal(d.get(), np.asarray(h, dtype=np.uint32))
    assert np.array_equal(d_ring.get(), d_ring.host)
    return want


def advance(W, acked, sent, nflows, window, adv, fill, seq0, rec0, bases=True, model=T.advance_flows):
    """wtp_tx_advance_flows into buffers that hold JUNK, against the model; returns the model's
    (acked_next, sent_next, seq0_next, rec0_next)."""
    S = nflows * window
    junk, junk_f = np.full(S, JUNK, np.uint32), np.full(nflows, JUNK, np.uint32)
    want = model(acked, sent, nflows, window, adv, fill, seq0 if bases else None, rec0 if bases else None, junk, junk,
                 junk_f if bases else None, junk_f if bases else None)
    ins = [Words(a) for a in (acked, sent, adv, seq0, rec0)]
    outs = [Words(JUNK, S), Words(JUNK, S), Words(JUNK, nflows), Words(JUNK, nflows)]
    b = (lambda x: x.t) if bases else (lambda x: None)  # noqa: E731
    W.tx_advance_flows(ins[0].t, ins[1].t, nflows, window, ins[2].t, fill, b(ins[3]), b(ins[4]), outs[0].t, outs[1].t, b(outs[2]),
                       b(outs[3]))
    torch.cuda.synchronize()
    for d, h in zip(outs, want[:2] + ((want[2], want[3]) if bases else (junk_f, junk_f))):
        assert np.array_equal(d.get(), h)
    for d, h in zip(ins, (acked, sent, adv, seq0, rec0)):
        assert np.array_equal(d.get(), np.asarray(h, dtype=np.uint32))
    if S:
        assert W.LIB.wtp_last_kernel().decode() == "k_txf_advance"
    return want


def build(W, b, nrec, seq0, rec0, rec_end, nflows, window, acked, sent, now, timeout, flags, max_sel, wire_stride=STRIDE,
          wire_off=0, work_off=16, optional=True, model=T.retransmit_var_flows):
    """wtp_tx_build_retransmit_var_flows over the Batch `b` against the model on the same prior
    contents; the scratch is exactly wtp_tx_work_bytes(S, max_sel) at byte `work_off` of its
    allocation, filled with 0xFF, with 40 bytes behind it that must stay.  Returns the model's
    result."""
    S = nflows * window
    prior = (np.full(max(max_sel, 1) * wire_stride, 0xA5, np.uint8), np.full(max_sel, 0x5E1, np.uint32),
             np.full(max_sel, 0x1E4, np.uint32), np.full(max_sel, 0xC4C, np.uint32))
    want = model(b.host, b.base_bytes, b.offs, b.lens, nrec, seq0, rec0, rec_end, nflows, window, acked, sent, now, timeout, flags,
                 prior[0], wire_stride, max_sel, *(prior[1:] if optional else (None, None, None)))
    wire = Bytes(prior[0], off=wire_off, front=64, back=64)
    ins = [Words(a) for a in (seq0, rec0, rec_end, acked)]
    d_sent, counts = Words(sent), Words(0x99, 2)
    outs = [Words(a) for a in prior[1:]]
    need = W.tx_work_bytes(S, max_sel)
    work = torch.full((work_off + need + 40,), 0xFF, dtype=torch.uint8, device="cuda")
    o = (lambda x: x.t) if optional else (lambda x: None)  # noqa: E731
    W.tx_build_retransmit_var_flows(b.base, b.base_bytes, b.o, b.l.t, nrec, ins[0].t, ins[1].t, ins[2].t, nflows, window, ins[3].t,
                                    d_sent.t, now, timeout, flags, wire.t, wire_stride, max_sel, o(outs[0]), o(outs[1]),
                                    o(outs[2]), counts.t, work=work[work_off:work_off + need])
    torch.cuda.synchronize()
    emitted, due = want[5]
    assert tuple(counts.get().tolist()) == (emitted, due)
    for d, h, p in zip(outs, want[1:4], prior[1:]):
        assert np.array_equal(d.get(), h if optional else p)
    sel = want[1] if optional else model(b.host, b.base_bytes, b.offs, b.lens, nrec, seq0, rec0, rec_end, nflows, window, acked,
                                         sent, now, timeout, flags, prior[0], wire_stride, max_sel, prior[1])[1]
    assert_bytes_equal(wire.get(), want[0], wire_stride, lambda k: f"ring entry {k}, global slot {sel[k] if k < emitted else None}")
    assert np.array_equal(d_sent.get(), want[4])
    for d, h in zip(ins, (seq0, rec0, rec_end, acked)):
        assert np.array_equal(d.get(), np.asarray(h, dtype=np.uint32))
    b.check_untouched()
    assert bool((work[:work_off] == 0xFF).all()) and bool((work[work_off + need:] == 0xFF).all())
    assert W.LIB.wtp_last_kernel().decode() == ("k_txf_emit" if min(S, max_sel) else "k_txf_select")
    return want


# ---- 1. the fuzz corpus ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", T.FUZZ_SEEDS)
def test_fuzz(W, seed, mode):
    """Every call of the corpus against the model (tests/test_txflows_model.py holds the corpus
    to its kinds): ingest, slide and build of two successive rounds on one state."""
    calls, case = T.fuzz_calls(seed, mode)
    nf, w = case["nflows"], case["window"]
    b = Batch(case["base"], case["offs"], case["lens"], base_off=(0, 1, 4)[seed % 3], base_bytes=case["base_bytes"])
    for i, c in enumerate(calls):
        got = ingest(W, c["ring"], case["stride"], c["rl"], c["flow"], mode, c["seq0"], c["rec0"], case["rec_end"], nf, w,
                     c["acked0"], with_hit=(seed + i) % 4 != 3, ring_off=(0, 1, 8)[(seed + i) % 3])
        assert all(np.array_equal(g, x) for g, x in zip(got, c["ingest"]))
        ak, sm, sq, rc = advance(W, got[2], c["sent0"], nf, w, got[3], c["fill"], c["seq0"], c["rec0"])
        assert all(np.array_equal(g, x) for g, x in zip((ak, sm, sq, rc), c["advance"]))
        got = build(W, b, case["nrec"], sq, rc, case["rec_end"], nf, w, ak, sm, c["now"], T.FUZZ_TIMEOUT, c["flags"], c["max_sel"],
                    wire_stride=case["wire_stride"], work_off=(16, 1, 6)[(seed + i) % 3])
        assert all(np.array_equal(g, x) for g, x in zip(got[:5], c["build"][:5])) and got[5] == c["build"][5]
    assert_no_data_error(W)


# ---- 2. one flow is the three single-window calls ------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_single_flow_identity(W, mode):
    """nflows == 1: every output equals, word for word, what wtp_tx_ingest_acks, wtp_tx_advance
    and wtp_tx_build_retransmit_var write on the same inputs (offsets and lengths advanced by
    rec0, inflight = the flow's)."""
    for seed in (1, 2, 6):
        calls, case = T.fuzz_calls(seed, mode)
        c, w, stride = calls[0], case["window"], case["stride"]
        mine = np.flatnonzero(c["flow"] == 0)
        ring, rl, n = F.rows(c["ring"], stride, mine), c["rl"][mine], mine.size
        seq0, rec0, rec_end = c["seq0"][:1], c["rec0"][:1], np.array([int(c["rec0"][0]) + w - 1], np.uint32)
        inf = w - 1
        acked, sent = c["acked0"][:w].copy(), c["sent0"][:w]
        want = ingest(W, ring, stride, rl, np.zeros(n, np.uint32), mode, seq0, rec0, rec_end, 1, w, acked)
        d_ring, d_rl, d_acked = Bytes(ring, front=64, back=64), Words(rl), Words(acked)
        d_ok, d_hit, d_counts = Bytes(fill=7, size=n), Words(12345, n), Words(9, 2)
        W.tx_ingest_acks(d_ring.t, stride, d_rl.t, n, mode, int(seq0[0]), inf, d_acked.t, d_ok.t, d_hit.t, d_counts.t)
        torch.cuda.synchronize()
        assert np.array_equal(d_ok.get(), want[0]) and np.array_equal(d_hit.get(), want[1])
        assert np.array_equal(d_acked.get(), want[2]) and d_counts.get().tolist() == [int(want[3][0]), int(want[4][0])]
        ak, sm, sq, rc = advance(W, want[2], sent, 1, w, want[3], c["fill"], seq0, rec0)
        outs = [Words(JUNK, w), Words(JUNK, w)]
        W.tx_advance(Words(want[2]).t, Words(sent).t, w, d_counts.t, c["fill"], outs[0].t, outs[1].t)
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].get(), ak) and np.array_equal(outs[1].get(), sm)
        b = Batch(case["base"], case["offs"], case["lens"], base_bytes=case["base_bytes"])
        inf, r0 = T.inflight_of(rc, rec_end, 0, w), int(rc[0])
        for max_sel in (w, 2, 0):
            got = build(W, b, case["nrec"], sq, rc, rec_end, 1, w, ak, sm, c["now"], T.FUZZ_TIMEOUT, c["flags"], max_sel)
            wire = Bytes(fill=0xA5, size=max(max_sel, 1) * STRIDE, front=64, back=64)
            o = [Words(0x5E1, max_sel), Words(0x1E4, max_sel), Words(0xC4C, max_sel)]
            d_sent, cnt = Words(sm), Words(0x99, 2)
            W.tx_build_retransmit_var(b.base, b.base_bytes, b.o[r0:], b.l.t[r0:], int(sq[0]), inf, Words(ak).t, d_sent.t, c["now"],
                                      T.FUZZ_TIMEOUT, c["flags"], wire.t, STRIDE, max_sel, o[0].t, o[1].t, o[2].t, cnt.t)
            torch.cuda.synchronize()
            assert np.array_equal(wire.get(), got[0]) and all(np.array_equal(d.get(), h) for d, h in zip(o, got[1:4]))
            assert np.array_equal(d_sent.get(), got[4]) and tuple(cnt.get().tolist()) == got[5]
    assert_no_data_error(W)


# ---- 3. flow boundaries inside a wave and inside a 1024-slot block -------------------------------
def shape_state(rng, nflows, window, records=None):
    """A state of `nflows` windows: seq0 random (flow 0 at the wrap), records of 0 .. 40 bytes,
    flow f's at [f * per, (f + 1) * per) with per = 2 * window + 2, except that every seventh flow
    has fewer records than slots and every eleventh none; acked mostly set, with whole leading
    runs, so that the leading-run pass has something to find in every part of a wave."""
    S, per = nflows * window, 2 * window + 2
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    seq0[0] = M32 - 1
    rec0 = (np.arange(nflows) * per).astype(np.uint32)
    count = np.where(np.arange(nflows) % 11 == 10, 0, np.where(np.arange(nflows) % 7 == 6, max(window // 2, 1), per))
    rec_end = (rec0 + count).astype(np.uint32)
    lens = rng.integers(0, 41, nflows * per).astype(np.uint32) if records is None else records
    acked = (rng.random(S) < 0.8).astype(np.uint32)
    lead = rng.integers(0, window + 1, nflows)
    acked[(np.arange(S) % window) < np.repeat(lead, window)] = 1
    acked[np.repeat(rng.random(nflows) < 0.3, window)] = 0  # some flows with nothing ACKed
    return seq0, rec0, rec_end, lens, acked


def shape_acks(rng, mode, seq0, rec0, rec_end, nflows, window, per_flow=2):
    dg, flow = [], []
    for f in rng.permutation(nflows):
        inf = T.inflight_of(rec0, rec_end, int(f), window)
        for _ in range(per_flow):
            dg.append(R.ack_datagram(int(seq0[f]) + int(rng.integers(0, inf + 2))))
            flow.append(int(f))
    ring, rl = R.make_ring(dg, 16)
    return ring, rl, np.array(flow, np.uint32)


SHAPES = ((700, 3), (3, 1025), (1, 2049), (65, 63), (2, 64))


@pytest.mark.parametrize("nflows,window", SHAPES)
def test_flow_boundaries_inside_a_wave_and_a_block(W, nflows, window):
    rng = np.random.default_rng(nflows * 4099 + window)
    S = nflows * window
    seq0, rec0, rec_end, lens, acked = shape_state(rng, nflows, window)
    b = Batch(O.synth_fill_np(max(int(lens.sum()), 1), start_byte=5), buildvar_model.packed_offsets(lens), lens,
              base_bytes=int(lens.sum()))
    now, timeout = 5000, 100
    sent_sparse = np.where(rng.random(S) < 0.2, now - timeout - 1, now).astype(np.uint32)  # a sparse due set
    for mode in MODES:
        ring, rl, flow = shape_acks(rng, mode, seq0, rec0, rec_end, nflows, window)
        got = ingest(W, ring, 16, rl, flow, mode, seq0, rec0, rec_end, nflows, window, acked)
        assert nflows < 10 or ((got[3] > 0).any() and (got[3] == 0).any())
        ak, sm, sq, rc = advance(W, got[2], sent_sparse, nflows, window, got[3], now, seq0, rec0)  # shifted in: not due
        sparse = build(W, b, lens.size, sq, rc, rec_end, nflows, window, ak, sm, now, timeout, 0, S)
        assert 0 < sparse[5][0] == sparse[5][1] < S // 2
        every = build(W, b, lens.size, sq, rc, rec_end, nflows, window, np.zeros(S, np.uint32), sm, now, timeout, T.RETX_ALL, S)
        infl = sum(T.inflight_of(rc, rec_end, f, window) for f in range(nflows))
        assert every[5] == (infl, infl) and infl > S // 2
        cut = next(k for k in range(infl // 2, infl) if every[1][k] % window not in (0, window - 1) or window < 4)
        part = build(W, b, lens.size, sq, rc, rec_end, nflows, window, np.zeros(S, np.uint32), sm, now, timeout, T.RETX_ALL, cut)
        assert part[5] == (cut, infl) and np.array_equal(part[1], every[1][:cut])
        none = build(W, b, lens.size, sq, rc, rec_end, nflows, window, np.zeros(S, np.uint32), sm, now, timeout, T.RETX_ALL, 0)
        assert none[5] == (0, infl)
    advance(W, acked, sent_sparse, nflows, window, np.full(nflows, window + 5, np.uint32), 1, seq0, rec0, bases=False)
    assert_no_data_error(W)


def test_degenerate_shapes(W):
    z, one = np.zeros(0, np.uint32), np.zeros(1, np.uint32)
    ring, rl = R.make_ring([R.ack_datagram(0), R.ack_datagram(1, checksum=5)], 16)
    b = Batch(np.zeros(16, np.uint8), [0], [4])
    for mode in MODES:
        assert ingest(W, ring, 16, rl, [7, T.NO_FLOW], mode, z, z, z, 0, 9, z)[0].tolist() == [1, 0]  # no flows
        assert ingest(W, ring, 16, rl, [0, 0], mode, one, one, one + 3, 1, 0, z)[3].tolist() == [0]  # no slots
        got = ingest(W, ring[:0], 16, z, z, mode, one, one, one + 3, 1, 4, [1, 1, 0, 1])  # no datagrams: the state's run
        assert got[3].tolist() == [2] and got[4].tolist() == [0]
    for nf, w in ((0, 5), (3, 0)):
        f = np.zeros(nf, np.uint32)
        assert build(W, b, 1, f, f, f + 1, nf, w, z, z, 1, 1, T.RETX_ALL, 4)[5] == (0, 0)
        advance(W, z, z, nf, w, f, 1, f, f)  # launches nothing, writes nothing
    assert_no_data_error(W)


# ---- 4. a round size above one ---------------------------------------------------------------
def test_more_emitted_datagrams_than_waves_in_the_grid(W):
    """S = 5200, every slot due: above 5120 emitted datagrams a wave of the emit kernel takes two
    datagrams per round.  Short mixed lengths, 13 flows of 400 slots."""
    nflows, window = 13, 400
    S = nflows * window
    rng = np.random.default_rng(5200)
    lens = rng.choice(np.array([0, 1, 15, 16, 17, 63, 64, 65, 130], np.uint32), S)
    b = Batch(O.synth_fill_np(int(lens.sum()), start_byte=9), buildvar_model.packed_offsets(lens), lens, base_off=1)
    seq0 = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    rec0 = (np.arange(nflows) * window).astype(np.uint32)
    got = build(W, b, S, seq0, rec0, rec0 + np.uint32(window), nflows, window, np.zeros(S, np.uint32), np.zeros(S, np.uint32), 77,
                0, T.RETX_ALL, S)
    assert got[5] == (S, S) and S > 5120
    assert_no_data_error(W)


# ---- 5. alignment ----------------------------------------------------------------------------
@pytest.mark.parametrize("wire_off,wire_stride,base_off,work_off", [(1, 1473, 0, 16), (0, 1473, 1, 3), (1, STRIDE, 1, 1),
                                                                   (0, STRIDE, 1, 7)])
def test_alignment(W, wire_off, wire_stride, base_off, work_off):
    """A wire at 1 byte past a 16-B boundary and a stride of 1473 take the bytewise path; a
    source at byte 1 takes the fast path's realigned loads; the scratch at any alignment."""
    calls, case = T.fuzz_calls(4, T.CUMULATIVE)
    c, nf, w = calls[0], case["nflows"], case["window"]
    b = Batch(case["base"], case["offs"], case["lens"], base_off=base_off, base_bytes=case["base_bytes"])
    ak, sm, sq, rc = c["advance"]
    got = build(W, b, case["nrec"], sq, rc, case["rec_end"], nf, w, ak, sm, c["now"], T.FUZZ_TIMEOUT, T.RETX_ALL, nf * w,
                wire_stride=wire_stride, wire_off=wire_off, work_off=work_off, optional=wire_off == 0)
    assert got[5][0] > w and len(b.phases()) > 4
    assert_no_data_error(W)


# ---- 6. offsets above 2^32 -------------------------------------------------------------------
def test_offsets_above_4_gib(W):
    """Records whose 64-bit offsets lie below, across and above 2^32 in a source of 4 GiB + 1 MiB
    that repeats a 1 MiB period: tests/test_gpu_wide.py's scheme and its skip condition."""
    period = O.synth_fill_np(1 << 20, start_byte=3)
    total = (1 << 32) + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < total + (1 << 29):
        pytest.skip(f"{free / 2**30:.1f} GiB free, the test needs {total / 2**30:.1f}")
    nflows, window = 3, 5
    S = nflows * window
    rng = np.random.default_rng(32)
    lens = rng.choice(np.array([1, 17, 700, MAXP], np.uint32), S)
    offs = ((1 << 32) - 3000 + np.arange(S, dtype=np.uint64) * np.uint64(997)).astype(np.uint64)
    offs[0], offs[1], offs[S - 1] = 5, (1 << 32) - 700, total - int(lens[S - 1])  # low, across 2^32, the last byte
    assert (offs < (1 << 32)).any() and (offs > (1 << 32)).sum() > 5 and ((offs < (1 << 32)) & (offs + lens > (1 << 32))).any()
    mem = None
    try:
        mem = periodic(period, total)

        class Wide:  # what build() reads of a Batch, with the host image given by the period
            base, base_bytes, host = mem.t, total, None
            o, l = torch.from_numpy(offs.view(np.int64)).cuda(), Words(lens)

            def check_untouched(self):
                mem.check_guards()

        b = Wide()
        b.offs, b.lens = offs, lens

        def model(base, base_bytes, offsets, lengths, *rest):
            # the same records in a compact image: the model never sees 4 GiB
            small = np.concatenate([period[(int(o) + np.arange(int(n))) % period.size] for o, n in zip(offsets, lengths)])
            return T.retransmit_var_flows(small, small.size, buildvar_model.packed_offsets(lengths), lengths, *rest)

        seq0 = np.array([M32 - 2, 7, 7], np.uint32)
        rec0 = (np.arange(nflows) * window).astype(np.uint32)
        got = build(W, b, S, seq0, rec0, rec0 + np.uint32(window), nflows, window, np.zeros(S, np.uint32), np.zeros(S, np.uint32),
                    9, 0, T.RETX_ALL, S, model=model)
        assert got[5] == (S, S) and (got[2] == 16 + lens).all()
    finally:
        del mem
        torch.cuda.empty_cache()
    assert_no_data_error(W)


# ---- 7. the sender's graph ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_graph_replay(W_noinit, mode):
    """Two sender rounds captured once, A -> B then B -> A over two sets of state (acked, sent_ms,
    seq0, rec0), and replayed: between replays the host rewrites the two ACK rings with their
    flow labels (and refills the output rings with the model's prior image) and nothing else,
    every base is what the advance left on the device, and every replay equals the model.
    WTP_RETX_ALL, so no input depends on the time."""
    W = W_noinit
    nflows, window, n, now = 5, 37, 24, 4242
    S = nflows * window
    rng = np.random.default_rng(0x6AF + mode)
    lens = rng.integers(0, 300, 4000).astype(np.uint32)
    b = Batch(O.synth_fill_np(int(lens.sum()), start_byte=2), buildvar_model.packed_offsets(lens), lens)
    h_seq = rng.integers(0, 1 << 32, nflows).astype(np.uint32)
    h_seq[0] = M32 - 5
    h_rec = (np.arange(nflows) * 800).astype(np.uint32)
    rec_end = h_rec + np.array([800, 800, 20, 0, 800], np.uint32)
    h_ack, h_sent = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
    z = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
    acked, sent = [dev_s32(h_ack), z(S, 5)], [dev_s32(h_sent), z(S, 5)]
    seq, rec, d_end = [dev_s32(h_seq), z(nflows)], [dev_s32(h_rec), z(nflows)], dev_s32(rec_end)
    rings = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for _ in range(2)]
    flows_ = [z(n) for _ in range(2)]
    rl, ok, hit = z(n, 16), torch.zeros(n, dtype=torch.uint8, device="cuda"), z(n)
    adv, fresh = [z(nflows), z(nflows)], [z(nflows), z(nflows)]
    wire = [torch.full((S * STRIDE,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sel, wl, cnt = [z(S), z(S)], [z(S), z(S)], [z(2), z(2)]
    work = torch.empty(W.tx_work_bytes(S, S), dtype=torch.uint8, device="cuda")

    def call():
        for r in range(2):  # round r reads state r and leaves state 1 - r
            W.tx_ingest_acks_flows(rings[r], 16, rl, flows_[r], n, mode, seq[r], rec[r], d_end, nflows, window, acked[r], ok, hit,
                                   adv[r], fresh[r])
            W.tx_advance_flows(acked[r], sent[r], nflows, window, adv[r], now, seq[r], rec[r], acked[1 - r], sent[1 - r],
                               seq[1 - r], rec[1 - r])
            W.tx_build_retransmit_var_flows(b.base, b.base_bytes, b.o, b.l.t, lens.size, seq[1 - r], rec[1 - r], d_end, nflows,
                                            window, acked[1 - r], sent[1 - r], now, 0, T.RETX_ALL, wire[r], STRIDE, S, sel[r],
                                            wl[r], None, cnt[r], work=work)

    def stage():
        """The two rounds' ACK rings for the bases as they stand, and the model's results."""
        nonlocal h_ack, h_sent, h_seq, h_rec
        want = []
        for r in range(2):
            ring, r_l, fl = shape_acks(rng, mode, h_seq, h_rec, rec_end, nflows, window, per_flow=5)
            fl[:4] = (nflows, T.NO_FLOW, 0, 0)
            ring, fl = ring[:n * 16], fl[:n]
            rings[r].copy_(torch.from_numpy(ring))
            wire[r].fill_(0xA5)  # the model's prior image; the call leaves a slot's tail as it was
            flows_[r].copy_(dev_s32(fl))
            ing = T.ingest_flows(ring, 16, r_l[:n], fl, mode, h_seq, h_rec, rec_end, nflows, window, h_ack)
            junk = np.zeros(S, np.uint32)
            h_ack, sm, h_seq, h_rec = T.advance_flows(ing[2], h_sent, nflows, window, ing[3], now, h_seq, h_rec, junk, junk,
                                                      junk[:nflows], junk[:nflows])
            bld = T.retransmit_var_flows(b.host, b.base_bytes, b.offs, b.lens, lens.size, h_seq, h_rec, rec_end, nflows, window,
                                         h_ack, sm, now, 0, T.RETX_ALL, np.full(S * STRIDE, 0xA5, np.uint8), STRIDE, S,
                                         np.zeros(S, np.uint32), np.zeros(S, np.uint32))
            h_sent = bld[4]
            want.append((ing, bld))
        return want

    def check(want):
        for r, (ing, bld) in enumerate(want):
            e = bld[5][0]
            assert u32(cnt[r]).tolist() == list(bld[5]) and np.array_equal(u32(adv[r]), ing[3]) and np.array_equal(u32(fresh[r]), ing[4])
            assert np.array_equal(u32(sel[r])[:e], bld[1][:e]) and np.array_equal(u32(wl[r])[:e], bld[2][:e])
            assert_bytes_equal(wire[r].cpu().numpy()[:e * STRIDE], bld[0][:e * STRIDE], STRIDE, f"round {r}")
        assert np.array_equal(u32(acked[0]), h_ack) and np.array_equal(u32(sent[0]), h_sent)
        assert np.array_equal(u32(seq[0]), h_seq) and np.array_equal(u32(rec[0]), h_rec)  # written by the device alone

    # capture() runs the call once before it captures it: that run makes the first two rounds
    want = stage()
    torch.cuda.synchronize()
    graph, _ = capture(call)
    check(want)
    for _ in range(4):
        want = stage()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(want)
    assert (h_rec > np.arange(nflows) * 800)[[0, 1, 4]].any()  # windows did move, over several replays
    assert_no_data_error(W)


# ---- 8. four connections, seven calls per round --------------------------------------------------
class DevEnd:
    """Both ends of txflows_model.transfer on the device.  The sender is the three calls under
    test over two sets of state; the receiver is accept_flows, acks_flows, deliver_flows and
    rx_advance_flows.  The channels are index selections over the wire and the ACK ring; the
    host reads back selections, counts and per-flow results, and writes no base after the start."""

    def __init__(self, W, nflows=F.XFER_FLOWS, window=F.XFER_WINDOW):
        self.W, self.nflows, self.window = W, nflows, window
        nf, S = nflows, nflows * window
        z = lambda k, v=0: torch.full((k,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        z64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")  # noqa: E731
        base, base_bytes, offs, lens, rec0, rec_end, self.rec = T.xfer_table(nflows)
        self.b = Batch(base, offs, lens)
        seq0 = np.array(F.XFER_SEQ[:nf], dtype=np.uint32)
        self.tseq, self.trec, self.rec_end = [dev_s32(seq0), z(nf)], [dev_s32(rec0), z(nf)], dev_s32(rec_end)
        fill0 = int(s32([(F.XFER_NOW0 - F.XFER_TIMEOUT - 1) & M32])[0])
        self.acked, self.sent = [z(S), z(S)], [z(S, fill0), z(S, fill0)]
        self.wire = torch.full((S, STRIDE), 0xA5, dtype=torch.uint8, device="cuda")
        self.wl, self.sel, self.txc, self.tadv, self.tfresh = z(S), z(S), z(2), z(nf), z(nf)
        self.txwork = torch.empty(W.tx_work_bytes(S, S), dtype=torch.uint8, device="cuda")
        self.rseq = [dev_s32(seq0), z(nf)]
        self.img = [torch.full((S * MAXP,), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.sl = [z(S, -1) for _ in range(2)]
        self.ack, self.counts = z(nf), z(2)
        self.cap = S * MAXP
        self.rstream = Bytes(fill=0xA5, size=self.cap, front=64, back=64, guard=0xA5)
        self.fadv, self.finfo, self.dcounts = z64(nf), z64(4 * nf), z64(4)
        self.fwork = torch.empty(W.rx_deliver_flows_work_bytes(nf, window), dtype=torch.uint8, device="cuda")
        self.file = [Bytes(fill=0xA5, size=r[2], front=64, back=64, guard=0xA5) for r in self.rec]
        self.off = [0] * nf

    def build(self, now, timeout):
        S = self.nflows * self.window
        self.W.tx_build_retransmit_var_flows(self.b.base, self.b.base_bytes, self.b.o, self.b.l.t, self.b.n, self.tseq[0],
                                             self.trec[0], self.rec_end, self.nflows, self.window, self.acked[0], self.sent[0],
                                             now, timeout, 0, self.wire, STRIDE, S, self.sel, self.wl, None, self.txc,
                                             work=self.txwork)
        torch.cuda.synchronize()
        e, due = (int(c) for c in u32(self.txc))
        assert e == due
        return u32(self.sel[:e])

    def receive(self, gidx, flow, mode):
        W, w, nf, n = self.W, self.window, self.nflows, gidx.size
        pick = torch.from_numpy(gidx).cuda()
        ok = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        ring = self.wire[pick].contiguous() if n else ok  # n == 0: any pointer
        rl = self.wl[pick].contiguous() if n else self.counts
        d_flow = dev_s32(flow) if n else self.counts
        self.ack_ring = torch.zeros((max(n, 1), 16), dtype=torch.uint8, device="cuda")
        src = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
        W.accept_data_packets_flows(ring, STRIDE, rl, d_flow, n, self.rseq[0], nf, w, self.img[0], self.sl[0], ok, None, self.ack)
        W.rx_build_acks_flows(ring, STRIDE, rl, d_flow, n, mode, self.rseq[0], nf, w, ok, self.ack, self.ack_ring, 16, 0, n, src,
                              self.counts)
        W.rx_deliver_flows(self.img[0], self.sl[0], nf, w, w, self.rstream.t, self.cap, 0, None, None, self.fadv, self.finfo,
                           self.dcounts, work=self.fwork)
        W.rx_advance_flows(self.img[0], self.sl[0], nf, w, self.fadv, self.rseq[0], self.img[1], self.sl[1], self.rseq[1])
        torch.cuda.synchronize()
        for x in (self.img, self.sl, self.rseq):
            x.reverse()
        e, total = (int(c) for c in u32(self.counts))
        assert bool(ok[:n].all()) and e == total == n
        k, run, pk, prun = self.dcounts.cpu().tolist()
        assert k == run and pk == prun
        adv, info = self.fadv.cpu().tolist(), self.finfo.cpu().numpy().reshape(nf, 4).tolist()
        self.last = []
        for f in range(nf):
            _, _, B, nbytes = info[f]
            self.file[f].payload[self.off[f]:self.off[f] + nbytes] = self.rstream.payload[B:B + nbytes]
            self.off[f] += nbytes
            self.last.append((adv[f], nbytes))
        return u32(self.ack), u32(src[:e])

    def flushed(self):
        return self.last

    def ingest(self, aidx, aflow, mode, fill_ms):
        W, w, nf, na = self.W, self.window, self.nflows, aidx.size
        aok = torch.zeros(max(na, 1), dtype=torch.uint8, device="cuda")
        acks = self.ack_ring[torch.from_numpy(aidx).cuda()].contiguous() if na else aok  # na == 0: any pointer
        arl = torch.full((max(na, 1),), 16, dtype=torch.int32, device="cuda")
        W.tx_ingest_acks_flows(acks, 16, arl, dev_s32(aflow) if na else arl, na, mode, self.tseq[0], self.trec[0], self.rec_end, nf,
                               w, self.acked[0], aok, None, self.tadv, self.tfresh)
        W.tx_advance_flows(self.acked[0], self.sent[0], nf, w, self.tadv, fill_ms, self.tseq[0], self.trec[0], self.acked[1],
                           self.sent[1], self.tseq[1], self.trec[1])
        torch.cuda.synchronize()
        for x in (self.acked, self.sent, self.tseq, self.trec):
            x.reverse()
        assert bool(aok[:na].all())
        return u32(self.tadv).tolist()


@pytest.mark.parametrize("mode", MODES)
def test_transfer_of_four_connections(W, mode):
    """4 senders of 40 mixed-length records, window 8, loss and duplication 0.15, seven library
    calls per round whatever the number of connections: the log is the model loop's, round for
    round (so the model's round count bounds the device's), the four delivered files are the
    sources between guard bytes, and wtp_crc32_buffer of each is the oracle's CRC."""
    want, stats = T.transfer(T.ModelEnd(), mode)
    assert (stats >= 1).all() and len(want) <= F.XFER_MAX_ROUNDS
    end = DevEnd(W)
    got, _ = T.transfer(end, mode, max_rounds=len(want))
    assert got == want
    assert u32(end.trec[0]).tolist() == u32(end.rec_end).tolist()  # moved by the advance calls alone
    for f in range(F.XFER_FLOWS):
        _, _, total, host = end.rec[f]
        assert np.array_equal(end.file[f].get(), host)  # between 64 guard bytes on both sides
        crc = torch.zeros(1, dtype=torch.int32, device="cuda")
        W.crc32_buffer(end.file[f].t, total, crc)
        assert int(u32(crc)[0]) == O.crc32(host)
    assert_no_data_error(W)


# ---- 9. the copies' edges: every length, phase, round size and scale ------------------------------------
# The kernels of wtp_tx_flows.hip are their own copies of the single-window bodies, so the edge
# suites of tests/test_gpu_retxvar.py and test_gpu_retx.py do not reach them.  The inputs are
# tests/flows_cases.py's, whose preconditions tests/test_flows_cases.py asserts on the CPU; the
# model is the loop-free path of tests/txflows_model.py, held there to the per-flow path.
FAST = functools.partial(T.retransmit_var_flows, fast=True)


def case_batch(c, base_off=0):
    return Batch(c["base"], c["offs"], c["lens"], base_off=base_off, base_bytes=int(c["lens"].sum()))


def build_case(W, b, c, sent, max_sel, now=C.NOW, timeout=C.TIMEOUT, flags=0, model=FAST, **kw):
    return build(W, b, c["lens"].size, c["seq0"], c["rec0"], c["rec_end"], c["nflows"], c["window"], c["acked"], sent, now, timeout,
                 flags, max_sel, model=model, **kw)


@pytest.mark.parametrize("pattern", C.PATTERNS)
def test_every_length_due_patterns_and_rings(W, pattern):
    """1457 records, every length 0 .. 1456 once, permuted and packed (all 16 source phases, from
    d_base at byte 0 and 1 of its allocation), over 5 flows x window 300 of which the last has 257
    records and one wraps its sequence numbers; none, one, about 10 %, 50 % and all of them due;
    rings of due, due - 1 (then the call again on the timers that call left: the one slot left),
    due + 70 and S entries; on the vector path and on the bytewise one (wire at +1, stride 1473)."""
    c = C.every_length_case(pattern)
    d = c["d"]
    for base_off in (0, 1):
        b = case_batch(c, base_off)
        assert b.phases() == set(range(16))
        for wire_off, stride in ((0, STRIDE), (1, 1473)):
            for max_sel in c["rings"]:
                want = build_case(W, b, c, c["sent"], max_sel, wire_off=wire_off, wire_stride=stride)
                assert want[5] == (min(d, max_sel), d)
                if max_sel == d - 1:  # the call again: the last due slot alone, in a ring of one entry where d - 1 == 0
                    again = build_case(W, b, c, want[4], max(d - 1, 1), wire_off=wire_off, wire_stride=stride)
                    assert again[5] == (1, 1) and again[1][0] == np.flatnonzero(c["due"])[-1]
    assert_no_data_error(W)


def _count_case(W, count, rec_len, max_sel):
    c = C.count_case(count, rec_len)
    want = build_case(W, case_batch(c), c, c["sent"], max_sel)
    assert want[5] == (count, count) and np.array_equal(want[1][:count], c["due"])


@pytest.mark.parametrize("threshold", C.THRESHOLDS)
def test_each_side_of_every_round_size_change(W, threshold):
    """The capped grid of k_txf_emit (see flows_cases.THRESHOLDS): `threshold` datagrams run with
    G, one more with 2 G, the due slots spread evenly over 3 windows that are no multiple of 64.
    4-byte records at every threshold; up to 20 480 also a ring fitted to the count and full-size
    records."""
    for count in (threshold, threshold + 1):
        _count_case(W, count, 4, count + 9)
        if threshold <= 4 * C.CAP_WAVES:
            _count_case(W, count, 4, count)
            _count_case(W, count, MAXP, count + 9)
    assert_no_data_error(W)


def test_400000_short_records_all_due(W):
    """400 000 records of at most 8 bytes over 3 flows, all due: G = 64 and 6250 rounds over 5120
    waves, so waves run their loop a second time or leave it.  Compared on the device with the
    builder's rings of the three flows' records (byte-identity), and on the host: the sentinel
    tails, the headers and CRCs against the oracle, the payload bytes against the source."""
    c = C.many_short_records()
    n, nf, w, S = c["n"], c["nflows"], c["window"], c["S"]
    b = case_batch(c)
    want = torch.full((n * STRIDE,), 0xA5, dtype=torch.uint8, device="cuda")
    for f in range(nf):
        lo = f * w
        W.build_data_packets_var(b.base, b.base_bytes, b.o[lo:], b.l.t[lo:], min(w, n - lo), int(c["seq0"][f]), want[lo * STRIDE:],
                                 STRIDE)
    whole = Bytes(fill=0xA5, size=n * STRIDE, front=64, back=64, guard=0xA5)
    ins = [Words(c[k]) for k in ("seq0", "rec0", "rec_end")]
    acked, sent, counts = Words(0, S), Words(C.OLD, S), Words(0x99, 2)
    sel, wl, crc = Words(12345, n), Words(12345, n), Words(12345, n)
    work = torch.empty(W.tx_work_bytes(S, n), dtype=torch.uint8, device="cuda")
    W.tx_build_retransmit_var_flows(b.base, b.base_bytes, b.o, b.l.t, n, ins[0].t, ins[1].t, ins[2].t, nf, w, acked.t, sent.t, C.NOW,
                                    C.TIMEOUT, 0, whole.t, STRIDE, n, sel.t, wl.t, crc.t, counts.t, work=work)
    torch.cuda.synchronize()
    assert W.LIB.wtp_last_kernel().decode() == "k_txf_emit"
    assert torch.equal(whole.payload, want)
    del want
    slots = whole.payload.view(n, STRIDE)
    assert bool((slots[:, 24:] == 0xA5).all())
    whole.check_guards()
    assert counts.get().tolist() == [n, n] and np.array_equal(sel.get(), np.arange(n))
    assert np.array_equal(sent.get(), np.concatenate([np.full(n, C.NOW, np.uint32), np.full(S - n, C.OLD, np.uint32)]))
    assert np.array_equal(wl.get(), c["lens"] + 16) and np.array_equal(crc.get(), O.batch_var(c["base"], c["offs"], c["lens"]))
    front = slots[:, :24].cpu().numpy()
    head = np.ascontiguousarray(front[:, :16]).view(">u4")  # the headers against the oracle
    k = np.arange(n)
    assert (head[:, 0] == 2).all() and np.array_equal(head[:, 1], (c["seq0"][k // w].astype(np.int64) + k % w) & M32)
    assert np.array_equal(head[:, 2], c["lens"]) and np.array_equal(head[:, 3], crc.get())
    at = c["offs"].astype(np.int64)[:, None] + np.arange(8)
    inside = np.arange(8) < c["lens"][:, None]
    assert np.array_equal(front[:, 16:][inside], c["base"][np.minimum(at, c["base"].size - 1)][inside])
    assert (front[:, 16:][~inside] == 0xA5).all()
    b.check_untouched()
    assert_no_data_error(W)


@pytest.mark.parametrize("nflows,window", C.SCALE_SHAPES)
def test_selection_at_scale(W, nflows, window):
    """S = 2^20 slots, the documented limit: 1024 block counts, one per lane of k_txf_select,
    summed per wave and then over 16 waves; and S = 65 537: 65 block counts, one lane in the
    second wave of that sum.  A sparse due set that holds global slots 0, 63, 64, 1023, 1024,
    65 535, 65 536 and 2^20 - 1 and the first and last slot of several flows, into a ring with
    room for all of it and into one that ends inside a flow."""
    c = C.scale_case(nflows, window)
    b, d = case_batch(c), c["d"]
    full = build_case(W, b, c, c["sent"], d + 50)
    assert full[5] == (d, d) and np.array_equal(full[1][:d], np.flatnonzero(c["due"]))
    cut = C.cut_inside_a_flow(full[1], d, window)
    part = build_case(W, b, c, c["sent"], cut)
    assert part[5] == (cut, d) and np.array_equal(part[1], full[1][:cut])  # a prefix of the first call's
    assert_no_data_error(W)


@pytest.mark.parametrize("now,timeout", C.TIMER_CASES)
def test_timers_clock_wrap_and_retx_all(W, now, timeout):
    """uint32(now - sent) > timeout in every flow of three, with timers of age timeout - 1,
    timeout, timeout + 1 and timers in the future, across the clock's wrap, at timeout 0 and
    0xFFFFFFFF, without WTP_RETX_ALL and with it; the model is the per-flow one, and the
    selection is also the rule's own."""
    c = C.timer_case(now, timeout)
    b = case_batch(c)
    for flags, sel in ((0, c["due"]), (T.RETX_ALL, c["all"])):
        got = build_case(W, b, c, c["sent"], c["S"], now=now, timeout=timeout, flags=flags, model=T.retransmit_var_flows)
        assert got[5] == (sel.size, sel.size) and np.array_equal(got[1][:sel.size], sel)
    assert_no_data_error(W)


@pytest.mark.parametrize("mode", MODES)
def test_ack_batch_over_many_workgroups(W, mode):
    """About 70 000 shuffled ACKs over 300 flows x window 100, some 280 workgroups of
    k_txf_ingest: 20 000 for three slots of one flow and 20 000 of one value for another (the
    atomics' hot spots), damaged checksums, other types, unknown flows, the sequence numbers on
    both sides of every window, and a prior state that makes flow_fresh differ from the hits."""
    c = C.ack_batch(mode)
    got = ingest(W, c["ring"], 16, c["rl"], c["flow"], mode, c["seq0"], c["rec0"], c["rec_end"], c["nflows"], c["window"], c["acked0"],
                 model=functools.partial(T.ingest_flows, fast=True))
    C.check_ack_batch(c, got)
    assert_no_data_error(W)


@pytest.mark.parametrize("window", C.SLIDE_WINDOWS)
def test_slide_by_every_kind_of_advance(W, window):
    """7 flows whose flow_adv cycles through 0, 1, window - 1, window, window + 1 and 0xFFFFFFFF,
    with bases that wrap 2^32 in the slide, and without the base arrays."""
    c = C.slide_case(window)
    got = advance(W, c["acked"], c["sent"], 7, window, c["adv"], c["fill"], c["seq0"], c["rec0"])
    C.check_slide(c, got)
    advance(W, c["acked"], c["sent"], 7, window, c["adv"], c["fill"], c["seq0"], c["rec0"], bases=False)
    assert_no_data_error(W)


def test_slide_at_the_slot_limit(W):
    c = C.slide_case(1024, nflows=1024)
    got = advance(W, c["acked"], c["sent"], 1024, 1024, c["adv"], c["fill"], c["seq0"], c["rec0"],
                  model=functools.partial(T.advance_flows, fast=True))
    C.check_slide(c, got)
    assert_no_data_error(W)
