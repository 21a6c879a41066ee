"""Device-side receive without a GPU: the sequential model (tests/accept_model.py) that
the GPU tests compare wtp_accept_data_packets with reassembles a golden file from
shuffled, duplicated and corrupted datagrams, and the entry point validates its
arguments before it touches a device (like test_capi.py's validation test)."""
import ctypes as C
import os

import numpy as np

import accept_model as M
import oracle as O

STRIDE = 1472


def _ring(dgrams, stride=STRIDE):
    ring = np.zeros(len(dgrams) * stride, dtype=np.uint8)
    rl = np.zeros(len(dgrams), dtype=np.uint32)
    for i, d in enumerate(dgrams):
        ring[i * stride:i * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
        rl[i] = len(d)
    return ring, rl


def _input3(golden_dir):
    data = open(os.path.join(golden_dir, "input3.txt"), "rb").read()
    assert len(data) == 7 * 1456 + 10
    chunks = [data[o:o + 1456] for o in range(0, len(data), 1456)]
    return data, [O.build_datagram(s, c) for s, c in enumerate(chunks)]


def _state(window):
    return np.full(window * M.MAXP, 0xA5, dtype=np.uint8), np.full(window, M.EMPTY, dtype=np.uint32)


def test_model_reassembles_golden_file(golden_dir):
    data, dg = _input3(golden_dir)
    assert len(dg) == 8
    bad = bytearray(dg[3])
    bad[16 + 700] ^= 0x10  # seq 3 arrives corrupt ...
    # shuffled, seq 5 and seq 0 twice, and (last) the retransmit of seq 3
    arrivals = [dg[6], dg[5], bytes(bad), dg[0], dg[7], dg[5], dg[2], dg[1], dg[0], dg[4], dg[3]]
    ring, rl = _ring(arrivals)
    out0, sl0 = _state(8)
    ok, place, out, sl, ack = M.accept(ring, STRIDE, rl, 0, 8, out0, sl0)
    assert ok.tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert place.tolist() == [6, 5, M.NOT_PLACED, 0, 7, M.NOT_PLACED, 2, 1, M.NOT_PLACED, 4, 3]
    assert ack == 8
    assert out[:len(data)].tobytes() == data
    assert sl.tolist() == [1456] * 7 + [10]
    assert (out[len(data):] == 0xA5).all()  # the short last slot keeps its old tail
    assert (out0 == 0xA5).all() and (sl0 == M.EMPTY).all()  # the entry state is not modified


def test_model_leaves_a_gap_without_the_retransmit(golden_dir):
    data, dg = _input3(golden_dir)
    bad = bytearray(dg[3])
    bad[12] ^= 0x01  # checksum field
    arrivals = [dg[6], dg[5], bytes(bad), dg[0], dg[7], dg[5], dg[2], dg[1], dg[0], dg[4]]
    ring, rl = _ring(arrivals)
    ok, place, out, sl, ack = M.accept(ring, STRIDE, rl, 0, 8, *_state(8))
    assert ok[2] == 0 and place[2] == M.NOT_PLACED
    assert ack == 3 and sl[3] == M.EMPTY
    assert (out[3 * 1456:4 * 1456] == 0xA5).all()
    assert out[:3 * 1456].tobytes() == data[:3 * 1456] and out[4 * 1456:len(data)].tobytes() == data[4 * 1456:]
    # a second batch carrying the retransmit closes the gap on the carried-over state
    ring2, rl2 = _ring([dg[3]])
    _, place2, out2, sl2, ack2 = M.accept(ring2, STRIDE, rl2, 0, 8, out, sl)
    assert place2.tolist() == [3] and ack2 == 8 and out2[:len(data)].tobytes() == data


def test_model_window_wrap_types_and_lengths():
    seq0 = 0xFFFFFFFE
    pay = [bytes([i]) * (i + 1) for i in range(6)]
    arrivals = [O.build_datagram((seq0 + 2) & M.M32, pay[2]),       # slot 2 (seq 0 after the wrap)
                O.build_datagram((seq0 - 1) & M.M32, pay[1]),       # below the window
                O.build_datagram(seq0, pay[0], ptype=3),            # an ACK: never placed
                O.build_datagram(seq0, b""),                        # empty DATA payload: placed, length 0
                O.build_datagram((seq0 + 4) & M.M32, pay[4]),       # == seq0 + window: outside
                O.build_datagram((seq0 + 3) & M.M32, b"x" * 1457)]  # ok, but longer than a chunk
    ring, rl = _ring(arrivals, 1504)
    ok, place, out, sl, ack = M.accept(ring, 1504, rl, seq0, 4, *_state(4))
    assert ok.tolist() == [1] * 6
    assert place.tolist() == [2, M.NOT_PLACED, M.NOT_PLACED, 0, M.NOT_PLACED, M.NOT_PLACED]
    assert sl.tolist() == [0, M.EMPTY, 3, M.EMPTY] and ack == 0xFFFFFFFF
    assert out[2 * 1456:2 * 1456 + 3].tobytes() == pay[2] and (out[:2 * 1456] == 0xA5).all()
    # window == 0: nothing is placed, ack == seq0
    ok, place, out, sl, ack = M.accept(ring, 1504, rl, seq0, 0, *_state(0))
    assert (place == M.NOT_PLACED).all() and ack == seq0


def test_fuzz_corpus_is_not_vacuous():
    """The corpus of test_gpu_accept.py's test_fuzz_against_the_model, judged by the model
    alone: every batch of 8 or more datagrams carries every kind its stride permits; per seed,
    over its three calls, every kind has a datagram made for that kind alone on which the
    model's verdict is the one the kind stands for; the seeds cover every stride and offset,
    a window across the 2^32 wrap, n == 0 and n == 8; at least 3 seeds copy every payload with
    16-B vectors, 3 none and 2 some of each batch; and in at least 8 of the 12 seeds the final
    ACK lies strictly inside the window."""
    inside, seen_n, shapes, wraps, copies = 0, set(), set(), 0, []
    for seed in M.FUZZ_SEEDS:
        rng, window, seq0, stride, ring_off, out_off, ns = M.fuzz_case(seed)
        assert 1 <= window <= 700 and stride in M.FUZZ_STRIDES and len(ns) == 3
        assert seq0 >= 0xFFFFFD00 if seed % 2 else 0 <= seq0 < 1 << 32
        shapes |= {("stride", stride), ("ring", ring_off), ("out", out_off)}
        # which datagrams take the 16-B vector copy (the buffers are 16-B aligned before their offsets)
        vec = {(ring_off + i * stride) % 16 == 0 and out_off == 0 for i in range(8)}
        copies.append("all" if vec == {True} else "none" if vec == {False} else "mixed")
        wraps += seq0 + window > 1 << 32
        out, sl = _state(window)
        shown = set()
        for n in ns:
            ring, rl, kinds = M.fuzz_batch(rng, seq0, window, stride, sl, n)
            assert rl.size == n and ring.size == n * stride and (n == 0 or 8 <= n <= 600)
            seen_n.add(n)
            if n:
                assert set().union(*kinds) == set(M.fuzz_kinds(stride))
            ok, place, out, sl, ack = M.accept(ring, stride, rl, seq0, window, out, sl)
            for i, k in enumerate(kinds):
                if len(k) == 1:
                    placed = place[i] != M.NOT_PLACED
                    kind = next(iter(k))
                    if M.fuzz_verdict(kind, bool(ok[i]), placed, int(rl[i]), int(sl[place[i]]) if placed else None):
                        shown.add(kind)
        assert shown == set(M.fuzz_kinds(stride)), (seed, set(M.fuzz_kinds(stride)) - shown)
        inside += 0 < ((ack - seq0) & M.M32) < window
    assert inside >= 8
    assert 0 in seen_n and 8 in seen_n
    assert shapes == {("stride", s) for s in M.FUZZ_STRIDES} | {("ring", 0), ("ring", 1), ("ring", 8), ("out", 0), ("out", 4)}
    assert wraps >= 1
    assert copies.count("all") >= 3 and copies.count("mixed") >= 2 and copies.count("none") >= 3


def test_fuzz_batch_deals_every_kind_to_a_small_batch():
    """n == 8: the 17 kinds share 8 datagrams, no datagram holds two kinds of one group, and
    the in-batch duplicate follows its original with the same seqNum and another length."""
    rng = np.random.default_rng(1)
    ring, rl, kinds = M.fuzz_batch(rng, 100, 50, 1504, np.full(50, M.EMPTY, np.uint32), 8)
    assert set().union(*kinds) == set(M.FUZZ_KINDS)
    groups = [set(M.FUZZ_KINDS[:7]), set(M.FUZZ_KINDS[7:11]), set(M.FUZZ_KINDS[11:15]), set(M.FUZZ_KINDS[15:])]
    assert all(len(k & g) <= 1 for k in kinds for g in groups)
    first = next(i for i, k in enumerate(kinds) if "placeable" in k)
    dup = next(i for i, k in enumerate(kinds) if "dup_batch" in k)
    assert first < dup and ring[first * 1504 + 4:first * 1504 + 8].tobytes() == ring[dup * 1504 + 4:dup * 1504 + 8].tobytes()
    assert ring[first * 1504 + 8:first * 1504 + 12].tobytes() != ring[dup * 1504 + 8:dup * 1504 + 12].tobytes()  # length


def test_accept_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    assert "wtp_accept_data_packets" in W.EXPORTED
    buf = (C.c_uint32 * 8)()
    a = C.addressof(buf)
    # n == 0 with nothing to report: no device touched
    assert L.wtp_accept_data_packets(None, 1472, None, 0, 0, 0, None, None, None, None, None, None) == 0
    assert L.wtp_accept_data_packets(None, 1472, None, 0, 7, 64, None, None, None, None, None, None) == 0
    # a null required pointer with n > 0 -> WTP_EINVAL (-1) and a message
    for hole in range(5):
        args = [a, 1472, a, 1, 0, 1, a, a, a, None, None, None]
        args[(0, 2, 6, 7, 8)[hole]] = None
        assert L.wtp_accept_data_packets(*args) == -1
        assert b"null" in L.wtp_last_error()
    assert L.wtp_accept_data_packets(a, 8, a, 1, 0, 1, a, a, a, None, None, None) == -1
    assert b"stride" in L.wtp_last_error()
    assert L.wtp_accept_data_packets(a, 1472, a, 1 << 31, 0, 1, a, a, a, None, None, None) == -1
    assert b"2^31" in L.wtp_last_error()
