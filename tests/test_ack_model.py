"""Device-side ACK generation without a GPU: the sequential model (tests/ack_model.py) that
the GPU tests compare wtp_rx_build_acks with is checked against a literal receiver loop (the
std::map + `expected` loop of cpp/src/wReceiver.cpp:224-240 and the own-seqNum reply of the
reference's cpp/src/opt/Receiver.cpp:211-237, with the window held fixed per batch), its
vectorised path against its own loop, the end-to-end transfer of tests/test_gpu_ack.py is
run on the model alone, and the entry point validates its arguments before it touches a
device."""
import ctypes as C

import numpy as np
import pytest

import accept_model
import ack_model as A
import oracle as O
import retx_model as R

STRIDES = (1472, 1504)  # 1504 holds the oversize datagrams whole, so they verify


# ---- the literal loop ---------------------------------------------------------------------
def literal_receiver(facts, mode, seq0, window, slot_len):
    """One datagram at a time; returns [(index, ACK seqNum)]."""
    lead = 0
    while lead < window and slot_len[lead] != A.EMPTY:
        lead += 1
    expected = (seq0 + lead) & A.M32
    pending = {(seq0 + s) & A.M32 for s in range(lead, window) if slot_len[s] != A.EMPTY}
    acks = []
    for i, (intact, ptype, seq, plen) in enumerate(facts):
        if not intact or ptype != 2 or plen > A.MAXP:
            continue  # corrupted: drop, no ACK; not DATA; longer than a chunk
        d = (seq - seq0) & A.M32
        if window <= d < (1 << 31):
            continue  # h.seqNum >= expected + window: drop (the window is the batch's)
        if mode == A.SELECTIVE:
            acks.append((i, seq))
            continue
        if d < window and ((seq - expected) & A.M32) < (1 << 31):  # h.seqNum >= expected
            pending.add(seq)
        while expected in pending:
            pending.remove(expected)
            expected = (expected + 1) & A.M32
        acks.append((i, expected))
    return acks


def _case(rng, trace_no):
    window = int(rng.integers(0, 40))
    n = int(rng.integers(0, 60))
    seq0 = int(rng.choice([0, 5, 0xFFFFFFF0, 0xFFFFFFFF - window // 2]))
    stride = STRIDES[trace_no % 2]
    sl0 = A.prefilled(rng, window)
    dgrams, facts = A.trace(rng, n, seq0, window, sl0, stride)
    ring, rl = R.make_ring([d[:stride] for d in dgrams], stride)
    rl = np.array([len(d) for d in dgrams], dtype=np.uint32)
    img = np.zeros(window * A.MAXP, dtype=np.uint8)
    ok, place, _, sl, ack = accept_model.accept(ring, stride, rl, seq0, window, img, sl0)
    return dict(window=window, n=n, seq0=seq0, stride=stride, sl0=sl0, facts=facts, ring=ring, rl=rl, ok=ok, place=place,
                sl=sl, ack=ack)


@pytest.mark.parametrize("mode", [A.SELECTIVE, A.CUMULATIVE])
def test_model_equals_literal_receiver(mode):
    rng = np.random.default_rng(0xACC + mode)
    answered = below = dup = 0
    for t in range(300):
        c = _case(rng, t)
        assert c["ok"].tolist() == [int(f[0]) for f in c["facts"]]
        want = literal_receiver(c["facts"], mode, c["seq0"], c["window"], c["sl0"])
        for vec in (False, True):
            seq, src, counts = A.build_acks(c["ring"], c["stride"], c["rl"], mode, c["seq0"], c["window"], c["place"],
                                            c["sl"], vectorised=vec)
            assert list(zip(src.tolist(), seq.tolist())) == want and counts == (len(want), len(want))
        answered += len(want)
        below += sum(((c["facts"][i][2] - c["seq0"]) & A.M32) >= (1 << 31) for i, _ in want)
        dup += sum(c["place"][i] == A.NOT_PLACED and ((c["facts"][i][2] - c["seq0"]) & A.M32) < c["window"] for i, _ in want)
        # with accept's outputs the last eligible datagram's cumulative ACK is accept's, if
        # it is the batch's last datagram
        if mode == A.CUMULATIVE and want and want[-1][0] == c["n"] - 1:
            assert want[-1][1] == c["ack"]
    assert answered > 2000 and below > 100 and dup > 100  # the traces reach every class


def test_eligibility_rules():
    """One datagram of each kind against the header's list."""
    seq0, window, stride = 0xFFFFFFFE, 4, 1504
    pay = O.synth_fill_np(20).tobytes()
    big = O.synth_fill_np(1457).tobytes()
    good = O.build_datagram(0, pay)  # slot 2
    dg = [good, good, O.build_datagram(0xFFFFFFFD, pay), O.build_datagram(2, pay), O.build_datagram(1, pay),
          O.build_datagram(1, big), O.build_datagram(1, pay, 3), good[:12], good[:13] + bytes([good[13] ^ 1]) + good[14:],
          O.build_datagram(0xFFFFFFFF, pay)]
    ring, rl = R.make_ring(dg, stride)
    sl0 = np.array([A.EMPTY, 7, A.EMPTY, A.EMPTY], dtype=np.uint32)
    ok, place, _, sl, ack = accept_model.accept(ring, stride, rl, seq0, window, np.zeros(4 * A.MAXP, np.uint8), sl0)
    assert ok.tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0, 1]
    seq, src, counts = A.build_acks(ring, stride, rl, A.SELECTIVE, seq0, window)
    assert src.tolist() == [0, 1, 2, 4, 9] and seq.tolist() == [0, 0, 0xFFFFFFFD, 1, 0xFFFFFFFF] and counts == (5, 5)
    seq, src, counts = A.build_acks(ring, stride, rl, A.CUMULATIVE, seq0, window, place, sl)
    # slots: 0 = 0xFFFFFFFE (never), 1 = 0xFFFFFFFF (filled before, duplicated by datagram 9)
    assert src.tolist() == [0, 1, 2, 4, 9] and seq.tolist() == [seq0] * 5 and ack == seq0
    # the same batch on a window one lower: the run grows as the batch arrives
    seq0 = 0xFFFFFFFF
    sl0 = np.full(4, A.EMPTY, dtype=np.uint32)
    ok, place, _, sl, ack = accept_model.accept(ring, stride, rl, seq0, window, np.zeros(4 * A.MAXP, np.uint8), sl0)
    seq, src, _ = A.build_acks(ring, stride, rl, A.CUMULATIVE, seq0, window, place, sl)
    assert src.tolist() == [0, 1, 2, 3, 4, 9] and seq.tolist() == [seq0, seq0, seq0, seq0, seq0, 3] and ack == 3


@pytest.mark.parametrize("mode", [A.SELECTIVE, A.CUMULATIVE])
def test_arbitrary_place_vectorised_equals_loop(mode):
    """d_place is any input: entries >= window, repeated slots, slots that d_slot_len calls
    empty."""
    rng = np.random.default_rng(0xA2B + mode)
    for t in range(200):
        c = _case(rng, t)
        w, n = c["window"], c["n"]
        place = rng.integers(0, w + 5, n).astype(np.uint32)
        place[rng.random(n) < 0.3] = A.NOT_PLACED
        sl = A.prefilled(rng, w)
        okx = (rng.random(n) < 0.8).astype(np.uint8) & c["ok"]
        a = A.build_acks(c["ring"], c["stride"], c["rl"], mode, c["seq0"], w, place, sl, ok=okx)
        b = A.build_acks(c["ring"], c["stride"], c["rl"], mode, c["seq0"], w, place, sl, ok=okx, vectorised=True)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2]


@pytest.mark.parametrize("mode", [A.SELECTIVE, A.CUMULATIVE])
def test_pages_concatenate(mode):
    rng = np.random.default_rng(0x9A6E + mode)
    for t in range(40):
        c = _case(rng, t)
        args = (c["ring"], c["stride"], c["rl"], mode, c["seq0"], c["window"], c["place"], c["sl"])
        seq, src, (_, total) = A.build_acks(*args)
        for page in (1, 3, max(total, 1), total + 2):
            got_seq, got_src = [], []
            for skip in range(0, total + page, page):
                s, i, counts = A.build_acks(*args, skip=skip, max_acks=page)
                assert counts == (min(max(total - skip, 0), page), total)
                got_seq += s.tolist()
                got_src += i.tolist()
            assert got_seq == seq.tolist() and got_src == src.tolist()
        assert A.build_acks(*args, skip=1, max_acks=0)[2] == (0, total)


@pytest.mark.parametrize("mode,seq_base", [(A.SELECTIVE, 0), (A.SELECTIVE, 0xFFFFFF80), (A.CUMULATIVE, 0),
                                           (A.CUMULATIVE, 0xFFFFFF80)])
def test_transfer_on_the_model(mode, seq_base):
    """The end-to-end cases of tests/test_gpu_ack.py on the model alone.  Selective mode sends
    the ACK lists of retx_model.transfer, so it returns exactly that function's result (33
    rounds); cumulative mode sends running ACKs, takes whatever the model gives under the
    same seeds, and finishes within the loop's 40 rounds."""
    nchunks, total = R.E2E_CHUNKS, R.E2E_CHUNKS * R.MAXP - R.E2E_SHORT
    src = O.synth_fill_np(total, seed=R.E2E_SEED)
    end = A.ModelEnd(src, nchunks, R.E2E_WINDOW, seq_base)
    rounds, sets = A.transfer(end, nchunks, R.E2E_WINDOW, seq_base, mode, R.E2E_SEED, R.E2E_LOSS)
    old = R.transfer(R.ModelEnd(src, nchunks, R.E2E_WINDOW, seq_base), nchunks, R.E2E_WINDOW, seq_base, mode, R.E2E_SEED,
                     R.E2E_LOSS)
    if mode == A.SELECTIVE:
        assert (rounds, sets) == old and rounds == 33
    else:
        assert 3 <= rounds < 40 and any(sets)
    assert np.array_equal(end.img[:total], src) and (end.img[total:nchunks * R.MAXP] == 0xA5).all()
    assert end.acked[:nchunks].all()


def test_ack_bytes_are_the_endpoints_ack_datagram():
    seqs = [0, 1, 0x01020304, 0xFFFFFFFF]
    got = A.ack_bytes(seqs)
    for k, s in enumerate(seqs):
        assert got[k].tobytes() == R.ack_datagram(s) == O.build_datagram(s, b"", 3)


# ---- the C-ABI without a device --------------------------------------------------------------
def test_rx_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    for name in ("wtp_rx_ack_work_bytes", "wtp_rx_build_acks"):
        assert name in W.EXPORTED and hasattr(L, name)
    buf = (C.c_uint32 * 64)()
    a = C.addressof(buf)
    big = 1 << 30

    def acks(**kw):
        args = dict(dgrams=a, stride=16, recv_len=a, n=1, mode=1, seq0=0, window=4, ok=a, place=a, slot_len=a, wire=a,
                    ack_stride=16, skip=0, max_acks=4, src=None, counts=a, work=a, work_bytes=big)
        args.update(kw)
        return L.wtp_rx_build_acks(*args.values(), None)

    assert acks(n=W.RX_MAX_BATCH + 1) == -1 and b"n " in L.wtp_last_error()
    assert acks(window=W.RX_MAX_WINDOW + 1) == -1 and b"window" in L.wtp_last_error()
    assert acks(mode=2) == -1 and b"mode" in L.wtp_last_error()
    assert acks(stride=15) == -1 and b"stride" in L.wtp_last_error()
    assert acks(ack_stride=15) == -1 and b"ack_stride" in L.wtp_last_error()
    for mode in (0, 1):
        for n, window in ((1, 4), (5000, 70000)):
            need = W.rx_ack_work_bytes(n, window, mode)
            assert acks(mode=mode, n=n, window=window, work_bytes=need - 1) == -1 and b"work_bytes" in L.wtp_last_error()
        for hole in ("dgrams", "recv_len", "ok", "wire", "counts", "work"):
            assert acks(mode=mode, **{hole: None}) == -1 and b"null" in L.wtp_last_error()
        assert acks(mode=mode, n=0, counts=None) == -1 and acks(mode=mode, n=0, work=None) == -1
    for hole in ("place", "slot_len"):
        assert acks(**{hole: None}) == -1 and b"null" in L.wtp_last_error()


def test_rx_ack_work_bytes_is_monotone_and_bounded():
    """include/wtp_crc32.h: at most 64 KiB + 4 bytes per 1024 datagrams + 4 bytes per window
    slot, the window term in cumulative mode only."""
    import wtp_crc32 as W
    ns = [0, 1, 1023, 1024, 1025, 70000, 1 << 20, W.RX_MAX_BATCH]
    ws = [0, 1, 63, 64, 65, 1023, 1024, 1025, 70000, W.RX_MAX_WINDOW]
    for mode in (0, 1):
        grid = [[W.rx_ack_work_bytes(n, w, mode) for w in ws] for n in ns]
        for r, n in enumerate(ns):
            for c, w in enumerate(ws):
                assert grid[r][c] <= 65536 + 4 * ((n + 1023) // 1024) + (4 * w if mode else 0)
            assert grid[r] == sorted(grid[r])
        for c in range(len(ws)):
            col = [grid[r][c] for r in range(len(ns))]
            assert col == sorted(col)
    assert W.rx_ack_work_bytes(5000, 70000, 0) == W.rx_ack_work_bytes(5000, 0, 0)
