"""Device-side sender window without a GPU: the sequential model (tests/retx_model.py) that
the GPU tests compare wtp_tx_ingest_acks / wtp_tx_build_retransmit with is checked against
a literal per-packet loop over a deque (the reference's cpp/src/opt/Window.cpp:45-75,
opt/Sender.cpp:121-139 and base/Sender.cpp:107-109), the end-to-end transfer of
tests/test_gpu_retx.py is confirmed to finish on the model alone, and the entry points
validate their arguments before they touch a device."""
import ctypes as C
from collections import deque

import numpy as np
import pytest

import oracle as O
import retx_model as M


# ---- the literal loop ---------------------------------------------------------------------
def literal_acks(window, acks, mode):
    """One ACK at a time over a deque of {seq, acked, sent}; returns (advance, newly)."""
    newly = 0
    for valid, seq in acks:
        if not valid:
            continue
        if mode == M.SELECTIVE:
            for p in window:  # Window::markPacketAsAcked
                if p["seq"] == seq:
                    newly += not p["acked"]
                    p["acked"] = True
                    break
        elif window:
            count = (seq - window[0]["seq"]) & M.M32  # base/Sender.cpp:107-109
            if 0 < count <= len(window):
                for k in range(count):  # removeAcknowledgedPackets, as marks: the batch keeps its window
                    newly += not window[k]["acked"]
                    window[k]["acked"] = True
    advance = 0  # Window::determineWindowAdvance
    for p in window:
        if not p["acked"]:
            break
        advance += 1
    return advance, newly


def literal_timeout(window, now, timeout, resend_all, max_sel):
    """opt/Sender.cpp:121-127 (base/Sender.cpp:101-105 with resend_all); returns the seqs
    re-sent, at most max_sel, and the number that were due."""
    out, due = [], 0
    for p in window:
        if not p["acked"] and (resend_all or ((now - p["sent"]) & M.M32) > timeout):
            due += 1
            if len(out) < max_sel:
                out.append(p["seq"])
                p["sent"] = now
    return out, due


def _ack_batch(rng, seq0, inflight, nmax=30):
    """One seeded ACK batch in a stride-16 ring: seqNums from three below the window to three
    past it.  kind 0: bad checksum, 1: DATA type, else a valid ACK."""
    n = int(rng.integers(0, nmax))
    seqs = (seq0 + rng.integers(-3, inflight + 4, n)) & M.M32
    kind = rng.integers(0, 8, n)
    dg = [M.ack_datagram(int(s), ptype=2 if k == 1 else 3, checksum=int(k == 0)) for s, k in zip(seqs, kind)]
    return (seqs, kind) + M.make_ring(dg, 16)


@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
def test_model_equals_literal_loop(mode):
    rng = np.random.default_rng(0x7E57 + mode)
    for trace in range(300):
        inflight = int(rng.integers(0, 40))
        seq0 = int(rng.choice([0, 5, 0xFFFFFFF0, 0xFFFFFFFF - inflight // 2]))
        now = int(rng.choice([100000, 0x100, 0xFFFFFFF0]))
        acked = (rng.random(inflight) < 0.3).astype(np.uint32)
        sent = ((now - rng.integers(0, 1200, inflight)) & M.M32).astype(np.uint32)
        total = max(inflight - 1, 0) * M.MAXP + int(rng.integers(1, M.MAXP + 1)) if inflight else 0
        src = O.synth_fill_np(total, start_byte=trace)
        window = deque({"seq": (seq0 + s) & M.M32, "acked": bool(acked[s]), "sent": int(sent[s])} for s in range(inflight))
        for batch in range(3):
            seqs, kind, ring, rl = _ack_batch(rng, seq0, inflight)
            ok, hit, acked2, (adv, newly) = M.ingest(ring, 16, rl, mode, seq0, inflight, acked)
            want = literal_acks(window, [(k > 1, int(s)) for s, k in zip(seqs, kind)], mode)
            assert (adv, newly) == want
            assert acked2.tolist() == [int(p["acked"]) for p in window]
            assert ok.tolist() == [int(k != 0) for k in kind]
            assert ((hit != M.NOT_PLACED) <= (kind > 1)).all()
            acked = acked2
            now = (now + int(rng.integers(0, 700))) & M.M32
            max_sel = int(rng.integers(0, inflight + 3))
            resend_all = bool(rng.integers(0, 4) == 0)
            sel, dgrams, sent2, (emitted, due) = M.retransmit(src, total, seq0, inflight, acked, sent, now, 500,
                                                              M.RETX_ALL if resend_all else 0, max_sel)
            lseq, ldue = literal_timeout(window, now, 500, resend_all, max_sel)
            assert [(seq0 + int(s)) & M.M32 for s in sel] == lseq and (emitted, due) == (len(lseq), ldue)
            assert sent2.tolist() == [p["sent"] for p in window]
            for s, d in zip(sel, dgrams):
                assert d == O.build_datagram((seq0 + int(s)) & M.M32, src[int(s) * M.MAXP:(int(s) + 1) * M.MAXP].tobytes())
            sent = sent2


BIG_WINDOWS = (1023, 1024, 1025, 2048, 2049, 2050, 3000)  # around k_tx_window's 1024-lane fill and two of its steps


@pytest.mark.parametrize("mode", [M.SELECTIVE, M.CUMULATIVE])
def test_vectorised_model_equals_literal_model(mode):
    """The numpy paths of the model (what the GPU tests of 2^20-slot windows compare with)
    against its literal loops (pinned to the deque above), on 320 traces of three carried
    batches each from the same generator; every 16th trace has a window of BIG_WINDOWS with
    a pre-ACKed leading run.  The classes of datagrams and the window edges the traces
    reach are counted, so a change of the generator cannot empty one unnoticed."""
    rng = np.random.default_rng(0xBEC7 + mode)
    seen = dict(dup=0, outside=0, edge=0, bad=0, wrong_type=0, lead_past_1024=0, lead_past_2049=0, top_past_1024=0,
                ring_short=0)
    for trace in range(320):
        big = trace % 16 == 0
        inflight = BIG_WINDOWS[(trace // 16) % len(BIG_WINDOWS)] if big else int(rng.integers(0, 40))
        seq0 = int(rng.choice([0, 5, 0xFFFFFFF0, 0xFFFFFFFF - inflight // 2]))
        now = int(rng.choice([100000, 0x100, 0xFFFFFFF0]))
        acked = (rng.random(inflight) < 0.3).astype(np.uint32)
        if big:
            acked[:min(int(rng.choice([0, 1023, 1024, 1025, 2049, inflight - 1, inflight])), inflight)] = 1
        sent = ((now - rng.integers(0, 1200, inflight)) & M.M32).astype(np.uint32)
        total = max(inflight - 1, 0) * M.MAXP + int(rng.integers(1, M.MAXP + 1)) if inflight else 0
        src = O.synth_fill_np(total, start_byte=trace)
        for batch in range(3):
            seqs, kind, ring, rl = _ack_batch(rng, seq0, inflight, 60 if big else 30)
            ok, hit, acked2, counts = M.ingest(ring, 16, rl, mode, seq0, inflight, acked)
            v_ok, v_hit, v_acked, v_counts = M.ingest(ring, 16, rl, mode, seq0, inflight, acked, vectorised=True)
            assert np.array_equal(v_ok, ok) and np.array_equal(v_hit, hit) and v_hit.dtype == hit.dtype
            assert np.array_equal(v_acked, acked2) and v_acked.dtype == acked2.dtype and v_counts == counts
            # the classes, from the generator's own facts
            d = (seqs.astype(np.int64) - seq0) & M.M32
            valid = kind > 1
            seen["bad"] += int((kind == 0).sum())
            seen["wrong_type"] += int((kind == 1).sum())
            seen["outside"] += int((valid & (hit == M.NOT_PLACED)).sum())
            at_end = valid & (d == inflight) & (inflight > 0)
            seen["edge"] += int(at_end.sum())
            assert (hit[at_end] == (inflight if mode == M.CUMULATIVE else M.NOT_PLACED)).all()
            marked, top = set(np.flatnonzero(acked).tolist()), 0
            for i in np.flatnonzero(hit != M.NOT_PLACED):  # an ACK that marks nothing new
                a = int(hit[i])
                seen["dup"] += int(a in marked if mode == M.SELECTIVE else a <= top)
                marked.add(a)
                top = max(top, a)
            seen["top_past_1024"] += int(mode == M.CUMULATIVE and top > 1024)
            seen["lead_past_1024"] += int(counts[0] > 1024)
            seen["lead_past_2049"] += int(counts[0] >= 2049)
            acked = acked2
            now = (now + int(rng.integers(0, 700))) & M.M32
            max_sel = int(rng.choice([0, 7, 64, inflight + 3])) if big else int(rng.integers(0, inflight + 3))
            flags = M.RETX_ALL if rng.integers(0, 4) == 0 else 0
            build = max_sel <= 64
            sel, dgrams, sent2, c = M.retransmit(src, total, seq0, inflight, acked, sent, now, 500, flags, max_sel, build=build)
            v_sel, v_dgrams, v_sent, v_c = M.retransmit(src, total, seq0, inflight, acked, sent, now, 500, flags, max_sel,
                                                        build=build, vectorised=True)
            assert np.array_equal(v_sel, sel) and v_sel.dtype == sel.dtype and v_dgrams == dgrams and v_c == c
            assert np.array_equal(v_sent, sent2) and v_sent.dtype == sent2.dtype
            assert len(dgrams) == (c[0] if build else 0)
            seen["ring_short"] += int(c[0] < c[1])
            sent = sent2
    # 320 traces x 3 batches x ~15 datagrams: an eighth each with a bad checksum and the wrong
    # type; of the valid ones about a fifth fall outside a ~20-slot window and one in ~27
    # names seq0 + inflight; a batch of 15 over 20 slots repeats itself several times
    assert min(seen["bad"], seen["wrong_type"], seen["outside"], seen["dup"]) > 1000 and seen["edge"] > 100, seen
    # (a cumulative batch leaves little un-ACKed, so rings shorter than the due set are rarer there)
    assert seen["ring_short"] > 10 and seen["lead_past_1024"] > 0 and seen["lead_past_2049"] > 0, seen
    assert seen["top_past_1024"] > 0 or mode == M.SELECTIVE, seen


def test_payload_limit_is_in_both_paths_of_the_model():
    """verify_limited: the oracle's verdict up to 4096 payload bytes, not ok and crc 0 above
    (include/wtp_crc32.h); the oracle itself has no limit.  Literal and vectorised ingest
    both take ok from it."""
    dg, lens = M.limit_corpus(5000, 3, 22, 5, 64)
    ring, rl = M.make_ring(dg, 5000)
    o_ok, o_crc = O.verify_datagrams(ring, 5000, rl)
    ok, crc = M.verify_limited(ring, 5000, rl)
    assert sorted(set(lens.tolist())) == [0, 1, 3, 4, 255, 1456, 1457, 4095, 4096, 4097, 4984]
    assert (o_ok[lens > 4096].sum(), ok[lens > 4096].sum()) == (4, 0) and (crc[lens > 4096] == 0).all()
    assert np.array_equal(ok[lens <= 4096], o_ok[lens <= 4096]) and np.array_equal(crc[lens <= 4096], o_crc[lens <= 4096])
    assert (ok[lens == 4096] == 1).sum() == 2 and (ok == 0).sum() == 6 + 3  # over the limit, and the corrupt ones below
    for vec in (False, True):
        m_ok, hit, acked, counts = M.ingest(ring, 5000, rl, M.SELECTIVE, 0, 64, np.zeros(64, np.uint32), vectorised=vec)
        assert np.array_equal(m_ok, ok) and np.array_equal(hit != M.NOT_PLACED, ok != 0) and counts[1] == len(set(hit[ok != 0]))
    short, slens = M.limit_corpus(5000, 3, 22, 5, 64, over=False)
    assert short == [d for d, ln in zip(dg, lens) if ln <= 4096] and slens.max() == 4096


def test_model_ok_is_the_oracles_and_hit_rules():
    pay = O.synth_fill_np(32).tobytes()
    dg = [M.ack_datagram(7), M.ack_datagram(7, checksum=1), M.ack_datagram(8, ptype=2),
          M.ack_datagram(9, checksum=O.crc32(pay), payload=pay), M.ack_datagram(9, checksum=O.crc32(pay) ^ 1, payload=pay),
          M.ack_datagram(6), M.ack_datagram(11), M.ack_datagram(12), M.ack_datagram(7)[:12], M.ack_datagram(7)]
    ring, rl = M.make_ring(dg, 48)
    rl[9] = 49  # recv_len > stride
    want_ok = O.verify_datagrams(ring, 48, rl)[0]
    assert want_ok.tolist() == [1, 0, 1, 1, 0, 1, 1, 1, 0, 0]
    ok, hit, acked, counts = M.ingest(ring, 48, rl, M.SELECTIVE, 7, 4, np.zeros(4, np.uint32))
    assert np.array_equal(ok, want_ok)
    N = M.NOT_PLACED
    assert hit.tolist() == [0, N, N, 2, N, N, N, N, N, N] and acked.tolist() == [1, 0, 1, 0] and counts == (1, 2)
    ok, hit, acked, counts = M.ingest(ring, 48, rl, M.CUMULATIVE, 7, 4, np.array([0, 0, 0, 1], np.uint32))
    assert hit.tolist() == [N, N, N, 2, N, N, 4, N, N, N] and acked.tolist() == [1, 1, 1, 1] and counts == (4, 3)


@pytest.mark.parametrize("mode,seq_base", [(M.SELECTIVE, 0), (M.SELECTIVE, 0xFFFFFF80), (M.CUMULATIVE, 0),
                                           (M.CUMULATIVE, 0xFFFFFF80)])
def test_transfer_finishes_on_the_model(mode, seq_base):
    """The end-to-end cases of tests/test_gpu_retx.py, on the model alone: each finishes
    within the 40 rounds that the GPU test allows, with an exact image."""
    nchunks, total = M.E2E_CHUNKS, M.E2E_CHUNKS * M.MAXP - M.E2E_SHORT
    src = O.synth_fill_np(total, seed=M.E2E_SEED)
    end = M.ModelEnd(src, nchunks, M.E2E_WINDOW, seq_base)
    rounds, sets = M.transfer(end, nchunks, M.E2E_WINDOW, seq_base, mode, M.E2E_SEED, M.E2E_LOSS)
    assert 3 <= rounds < 40 and any(sets)
    assert np.array_equal(end.img[:total], src) and (end.img[total:nchunks * M.MAXP] == 0xA5).all()
    assert end.acked[:nchunks].all()


# ---- the C-ABI without a device --------------------------------------------------------------
def test_tx_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    for name in ("wtp_tx_ingest_acks", "wtp_tx_work_bytes", "wtp_tx_build_retransmit"):
        assert name in W.EXPORTED and hasattr(L, name)
    buf = (C.c_uint32 * 64)()
    a = C.addressof(buf)

    def ingest(**kw):
        args = dict(dgrams=a, stride=16, recv_len=a, n=1, mode=0, seq0=0, inflight=4, acked=a, ok=a, hit=None, counts=a)
        args.update(kw)
        return L.wtp_tx_ingest_acks(*args.values(), None)

    for hole in ("dgrams", "recv_len", "ok", "acked", "counts"):
        assert ingest(**{hole: None}) == -1 and b"null" in L.wtp_last_error()
    assert ingest(stride=15) == -1 and b"stride" in L.wtp_last_error()
    assert ingest(mode=2) == -1 and b"mode" in L.wtp_last_error()
    assert ingest(n=1 << 31) == -1 and b"2^31" in L.wtp_last_error()
    assert ingest(inflight=W.TX_MAX_INFLIGHT + 1) == -1 and b"inflight" in L.wtp_last_error()
    assert ingest(n=0, counts=None) == -1

    big = 1 << 30

    def retx(**kw):
        args = dict(payloads=a, total=4 * 1456, seq0=0, inflight=4, acked=a, sent=a, now=0, timeout=500, flags=0, wire=a,
                    stride=1472, max_sel=4, sel=None, wire_len=None, counts=a, work=a, work_bytes=big)
        args.update(kw)
        return L.wtp_tx_build_retransmit(*args.values(), None)

    assert retx(stride=1471) == -1 and b"wire_stride" in L.wtp_last_error()
    assert retx(inflight=W.TX_MAX_INFLIGHT + 1, total=1 << 40) == -1 and b"inflight" in L.wtp_last_error()
    assert retx(total=3 * 1456) == -1 and b"total_bytes" in L.wtp_last_error()  # slot 3 would be empty
    assert retx(total=0) == -1
    assert retx(work_bytes=W.tx_work_bytes(4, 4) - 1) == -1 and b"work_bytes" in L.wtp_last_error()
    for hole in ("payloads", "acked", "sent", "wire", "counts", "work"):
        assert retx(**{hole: None}) == -1 and b"null" in L.wtp_last_error()


def test_tx_work_bytes_is_monotone_and_bounded():
    """include/wtp_crc32.h: at most 64 KiB + 16 bytes per max_sel entry."""
    import wtp_crc32 as W
    sizes = [0, 1, 63, 64, 65, 1000, 1024, 1025, 70000, W.TX_MAX_INFLIGHT]
    for i in sizes:
        prev = 0
        for m in sizes + [0xFFFFFFFF]:
            b = W.tx_work_bytes(i, m)
            assert prev <= b <= 65536 + 16 * m
            prev = b
    for m in sizes:
        col = [W.tx_work_bytes(i, m) for i in sizes]
        assert col == sorted(col)
