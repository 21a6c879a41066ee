"""wtp_tx_build_retransmit_var without a GPU: the sequential model (tests/retxvar_model.py)
that the GPU tests compare the call with is checked against a literal slot-by-slot loop, the
fixed-chunk model and the builder's model; the sender-window stream loop is confirmed to finish
on the models alone; and the entry point validates its arguments before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import buildvar_model as B
import oracle as O
import retx_model as R
import retxvar_model as M

MAXP, STRIDE, M32 = M.MAXP, M.STRIDE, M.M32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def literal(base, base_bytes, offs, lens, seq0, inflight, acked, sent, now, timeout, flags, wire, stride, max_sel):
    """One slot at a time, written from the header: returns (wire, sel, wire_len, crc, sent, counts)."""
    wire, sent = bytearray(wire.tobytes()), [int(x) for x in sent]
    sel, wl, crc, due = [], [], [], 0
    for s in range(inflight):
        if acked[s] != 0 or not ((flags & 1) or ((now - sent[s]) & M32) > timeout):
            continue
        due += 1
        if len(sel) == max_sel:
            continue
        k = len(sel)
        sel.append(s)
        sent[s] = now & M32
        off, ln = int(offs[s]), int(lens[s])
        if ln > MAXP or off > base_bytes or ln > base_bytes - off:
            wl.append(0)
            crc.append(0)
            continue
        payload = bytes(base[off:off + ln])
        c = O.crc32(payload)
        hdr = b"".join(int(v).to_bytes(4, "big") for v in (2, (seq0 + s) & M32, ln, c))
        wire[k * stride:k * stride + 16 + ln] = hdr + payload
        wl.append(16 + ln)
        crc.append(c)
    return np.frombuffer(bytes(wire), np.uint8), sel, wl, crc, sent, (len(sel), due)


def _trace(rng, inflight):
    """A seeded window: records in any order, some overlapping, some invalid; a mixed state."""
    base_bytes = int(rng.integers(1, 6000))
    base = O.synth_fill_np(base_bytes, start_byte=int(rng.integers(0, 256)))
    lens = O.zipf_lengths(max(inflight, 1), seed=int(rng.integers(1, 1 << 30)))[:inflight].astype(np.uint32)
    lens = np.minimum(lens, base_bytes).astype(np.uint32)
    offs = np.array([rng.integers(0, base_bytes - int(ln) + 1) for ln in lens], dtype=np.uint64)
    for s in range(inflight):
        kind = rng.random()
        if kind < 0.05:
            lens[s] = MAXP + 1
        elif kind < 0.08:
            lens[s] = 0xFFFFFFFF
        elif kind < 0.11:
            offs[s] = base_bytes + 1
        elif kind < 0.14:
            offs[s], lens[s] = base_bytes - 1, 2
        elif kind < 0.2:
            lens[s] = 0
    acked = (rng.random(inflight) < 0.4).astype(np.uint32) * rng.integers(1, 3, inflight).astype(np.uint32)
    return base, base_bytes, offs, lens, acked


@pytest.mark.parametrize("seed", range(12))
def test_model_equals_the_literal_loop(seed):
    """Seeded traces with sequence wrap and clock wrap; every ring size from none to the window."""
    rng = np.random.default_rng(seed)
    inflight = int(rng.integers(0, 90))
    base, base_bytes, offs, lens, acked = _trace(rng, inflight)
    seq0 = (0xFFFFFFFF - int(rng.integers(0, 60))) & M32
    now = int(rng.integers(0, 40))  # sent times lie before the wrap
    sent = ((now - rng.integers(0, 1200, inflight)) & M32).astype(np.uint32)
    for flags in (0, M.RETX_ALL):
        for max_sel in (0, 1, inflight // 2, inflight, inflight + 7):
            prior = np.full((max_sel + 1) * STRIDE, 0xA5, np.uint8)
            z = np.full(max_sel + 1, 12345, np.uint32)
            want = literal(base, base_bytes, offs, lens, seq0, inflight, acked, sent, now, 500, flags, prior, STRIDE, max_sel)
            for vec in (False, True):
                wire, sel, wl, crc, s2, counts = M.retransmit_var(base, base_bytes, offs, lens, seq0, inflight, acked, sent,
                                                                  now, 500, flags, prior, STRIDE, max_sel, z, z, z,
                                                                  vectorised=vec)
                e = counts[0]
                assert counts == want[5] and np.array_equal(wire, want[0]) and s2.tolist() == want[4]
                assert sel[:e].tolist() == want[1] and wl[:e].tolist() == want[2] and crc[:e].tolist() == want[3]
                assert (sel[e:] == 12345).all() and (wl[e:] == 12345).all() and (crc[e:] == 12345).all()
            assert M.retransmit_var(base, base_bytes, offs, lens, seq0, inflight, acked, sent, now, 500, flags, prior, STRIDE,
                                    max_sel)[1:4] == (None, None, None)


@pytest.mark.parametrize("short", [0, 100, 1455])
def test_chunked_buffer_equals_the_fixed_model(short):
    """A buffer cut into 1456-byte chunks: sel, datagrams, timers and counts of retx_model."""
    n = 70
    total = n * MAXP - short
    src = O.synth_fill_np(total, start_byte=short & 0xFF)
    offs = (np.arange(n, dtype=np.uint64) * MAXP).astype(np.uint64)
    lens = np.minimum(MAXP, total - offs.astype(np.int64)).astype(np.uint32)
    rng = np.random.default_rng(short)
    acked = (rng.random(n) < 0.5).astype(np.uint32)
    sent = rng.integers(0, 1000, n).astype(np.uint32)
    for max_sel in (n, 9):
        sel, dgrams, s_f, c_f = R.retransmit(src, total, 0xFFFFFFF0, n, acked, sent, 1200, 500, 0, max_sel)
        wire, sel_v, wl, _, s_v, c_v = M.retransmit_var(src, total, offs, lens, 0xFFFFFFF0, n, acked, sent, 1200, 500, 0,
                                                        np.zeros(n * STRIDE, np.uint8), STRIDE, max_sel, np.zeros(n, np.uint32),
                                                        np.zeros(n, np.uint32))
        assert c_v == c_f and np.array_equal(sel_v[:c_f[0]], sel) and np.array_equal(s_v, s_f) and c_f[0] > 0
        for k, d in enumerate(dgrams):
            assert wire[k * STRIDE:k * STRIDE + int(wl[k])].tobytes() == d


def test_all_due_equals_the_builders_model():
    n = 120
    lens = O.zipf_lengths(n, seed=5).astype(np.uint32)
    lens[[0, 3, 50]] = [0, MAXP, MAXP + 1]
    offs = B.packed_offsets(np.minimum(lens, MAXP))
    total = int(np.minimum(lens, MAXP).sum())
    src = O.synth_fill_np(total, start_byte=9)
    prior = np.full(n * 1488, 0x5A, np.uint8)
    want = B.build(src, total, offs, lens, 0xFFFFFFC0, prior, 1488)
    got = M.retransmit_var(src, total, offs, lens, 0xFFFFFFC0, n, np.zeros(n, np.uint32), np.zeros(n, np.uint32), 7, 0,
                           M.RETX_ALL, prior, 1488, n, np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2])
    assert got[1].tolist() == list(range(n)) and got[5] == (n, n) and (got[4] == 7).all()


def test_invalid_due_records_are_selected_and_leave_their_slots():
    base = O.synth_fill_np(3000)
    offs = np.array([0, 3001, 2999, 10, 0, 1 << 40], dtype=np.uint64)
    lens = np.array([MAXP + 1, 0, 2, 0xFFFFFFFF, 5, 1], dtype=np.uint32)
    prior = np.full(6 * STRIDE, 0xA5, np.uint8)
    wire, sel, wl, crc, sent, counts = M.retransmit_var(base, 3000, offs, lens, 10, 6, np.zeros(6), np.zeros(6), 100, 50, 0, prior,
                                                        STRIDE, 6, np.zeros(6), np.ones(6), np.ones(6))
    assert counts == (6, 6) and sel.tolist() == [0, 1, 2, 3, 4, 5] and (sent == 100).all()  # selected, timers reset
    assert wl.tolist() == [0, 0, 0, 0, 21, 0] and crc.tolist() == [0, 0, 0, 0, O.crc32(base[:5].tobytes()), 0]
    untouched = np.ones(6 * STRIDE, bool)
    untouched[4 * STRIDE:4 * STRIDE + 21] = False
    assert (wire[untouched] == 0xA5).all() and wire[4 * STRIDE:4 * STRIDE + 21].tobytes() == O.build_datagram(14, base[:5].tobytes())


# ---- the sender-window stream loop on the models alone --------------------------------------------
@pytest.fixture(scope="module")
def stream_log():
    lens, offs, total, host = M.stream_records()
    end = M.ModelEnd(host, total, offs, lens, M.STREAM_SEQ0, M.STREAM_WINDOW)
    return M.stream_rounds(end), end, (lens, offs, total, host)


def test_stream_loop_finishes_on_the_models(stream_log):
    log, end, (lens, offs, total, host) = stream_log
    print(f"rounds {len(log)}, emitted {sum(r[0] for r in log)} datagrams for {M.STREAM_RECORDS} records")
    assert len(log) == M.STREAM_ROUNDS <= 60 and M.STREAM_MAX_ROUNDS == 2 * M.STREAM_ROUNDS
    assert np.array_equal(end.rx.stream, host)
    assert np.array_equal(np.array(end.rx.offs, np.uint64), offs) and np.array_equal(np.array(end.rx.lens, np.uint32), lens)
    assert sum(r[3] for r in log) == M.STREAM_RECORDS == sum(r[7] for r in log)
    # retransmissions happened, first sends and retransmits shared selections, and both wrapped
    assert sum(r[0] for r in log) > M.STREAM_RECORDS
    assert (M.STREAM_SEQ0 + M.STREAM_RECORDS) > M32 and M.STREAM_NOW0 + len(log) > M32


def test_stream_loop_sends_first_and_again_in_one_selection(stream_log):
    log = stream_log[0]
    sbase, seen, mixed = 0, set(), 0
    for emitted, _due, sel, *_rest, adv in log:
        absolute = [sbase + s for s in sel]
        assert absolute == sorted(absolute)  # slot order, whatever the age
        again = [a for a in absolute if a in seen]
        mixed += bool(again) and len(again) < len(absolute)
        seen.update(absolute)
        sbase += adv
    assert seen == set(range(M.STREAM_RECORDS)) and mixed > 0


# ---- the C-ABI without a device --------------------------------------------------------------------
def test_symbol_binding_and_header():
    import wtp_crc32 as W
    assert "wtp_tx_build_retransmit_var" in W.EXPORTED and hasattr(W.LIB, "wtp_tx_build_retransmit_var")
    assert callable(W.tx_build_retransmit_var)
    decl = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    m = re.search(r"int\s+wtp_tx_build_retransmit_var\s*\(([^)]*)\)", decl)
    assert m, "wtp_tx_build_retransmit_var is not declared"
    names = [re.sub(r"[\s*]+", " ", p).split()[-1] for p in m.group(1).split(",")]
    assert names == ["d_base", "base_bytes", "d_offsets", "d_lengths", "seq0", "inflight", "d_acked", "d_sent_ms", "now_ms",
                     "timeout_ms", "flags", "d_wire", "wire_stride", "max_sel", "d_sel", "d_wire_len", "d_crc_out", "d_counts",
                     "d_work", "work_bytes", "stream"]
    assert len(W.LIB.wtp_tx_build_retransmit_var.argtypes) == len(names)
    assert decl.index("wtp_tx_build_retransmit(") < decl.index("wtp_tx_build_retransmit_var(") < decl.index("wtp_rx_build_acks(")
    assert "wtp_tx_build_retransmit_var" in decl[decl.index("/* wtp_tx_advance slides"):decl.index("int wtp_tx_advance(")]


def test_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    buf = (C.c_uint32 * 64)()
    a = C.addressof(buf)

    def call(**kw):
        args = dict(base=a, base_bytes=100, offs=a, lens=a, seq0=0, inflight=4, acked=a, sent=a, now=0, timeout=500, flags=0,
                    wire=a, stride=1472, max_sel=4, sel=None, wire_len=None, crc_out=None, counts=a, work=a,
                    work_bytes=W.tx_work_bytes(4, 4))  # wtp_tx_work_bytes is the scratch size: no other function
        args.update(kw)
        return L.wtp_tx_build_retransmit_var(*args.values(), None)

    messages = set()

    def refused(word, **kw):
        assert call(**kw) == -1
        msg = L.wtp_last_error()
        assert word in msg, msg
        messages.add(msg.split(b":")[0] if word == b"null" else msg)
        return msg

    refused(b"wire_stride", stride=1471)
    refused(b"inflight", inflight=W.TX_MAX_INFLIGHT + 1, work_bytes=1 << 30)
    refused(b"work_bytes", work_bytes=W.tx_work_bytes(4, 4) - 1)
    refused(b"work_bytes", max_sel=5, inflight=5, work_bytes=W.tx_work_bytes(4, 4) - 1)
    for hole in ("counts", "work"):
        assert b"d_counts or d_work" in refused(b"null", **{hole: None})
    for hole in ("base", "offs", "lens", "acked", "sent"):
        assert b"d_base, d_offsets" in refused(b"null", **{hole: None})
    assert b"d_wire" in refused(b"null", wire=None)
    assert len({m for m in messages}) >= 5  # each case its own message
    # the order of the checks: stride, inflight, work_bytes, then the pointers
    assert b"wire_stride" in refused(b"wire_stride", stride=0, inflight=W.TX_MAX_INFLIGHT + 1, work_bytes=0, counts=None)
    assert b"work_bytes" in refused(b"work_bytes", work_bytes=0, counts=None, wire=None)
    # no total_bytes check: an empty buffer and records that reach nowhere are the device's business
    # (not called here: a valid call launches)


def test_tx_work_bytes_is_the_scratch_size():
    """The same function and contract as the fixed call: a size it accepts is accepted here."""
    import wtp_crc32 as W
    L = W.LIB
    buf = (C.c_uint32 * 4)()
    a = C.addressof(buf)
    for inflight, max_sel in ((1, 1), (1000, 10), (70000, 70000), (W.TX_MAX_INFLIGHT, 0xFFFFFFFF)):
        need = W.tx_work_bytes(inflight, max_sel)
        # one byte less is refused with the size in the message; a NULL d_counts stops the accepted size before a launch
        assert L.wtp_tx_build_retransmit_var(a, 0, a, a, 0, inflight, a, a, 0, 0, 0, a, 1472, max_sel, None, None, None, a, a,
                                             need - 1, None) == -1
        assert str(need).encode() in L.wtp_last_error()
        assert L.wtp_tx_build_retransmit_var(a, 0, a, a, 0, inflight, a, a, 0, 0, 0, a, 1472, max_sel, None, None, None, None, a,
                                             need, None) == -1
        assert b"null" in L.wtp_last_error()
