"""CPU checks of the in-order flush (wtp_rx_deliver): the sequential model against a stream
cut and slotted by hand, its run endings and cuts, and the C-ABI's argument validation,
which needs no device."""
import ctypes as C
import os
import re

import numpy as np

import deliver_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, MAXP, EMPTY = 0xA5, M.MAXP, M.EMPTY


def _file(golden_dir):
    return np.frombuffer(open(os.path.join(golden_dir, "input3.txt"), "rb").read(), dtype=np.uint8)


def _cut(data, seed=0xD11):
    """`data` cut into irregular records, empty and full ones among them."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 1456, 3, 0, 0, 17]
    while sum(lens) + 1456 < data.size:
        lens.append(int(rng.integers(0, 1457)))
    lens += [data.size - sum(lens), 0]
    assert max(lens) <= 1456 and sum(lens) == data.size and len(lens) > 8
    ends = np.cumsum(lens)
    return [data[e - ln:e].tobytes() for e, ln in zip(ends, lens)], np.array(lens, dtype=np.uint32)


def test_model_turns_a_slotted_image_back_into_the_bytes(golden_dir):
    data = _file(golden_dir)
    recs, lens = _cut(data)
    n = lens.size
    # slotted by hand: record s at byte s * 1456 of an image with other bytes behind it
    img = np.full(n * MAXP, 0x3C, dtype=np.uint8)
    for s, r in enumerate(recs):
        img[s * MAXP:s * MAXP + len(r)] = np.frombuffer(r, dtype=np.uint8)
    off = 5
    prior = np.full(off + data.size + 9, SENT, dtype=np.uint8)
    po, pl = np.full(n + 2, 77, np.uint64), np.full(n + 2, 77, np.uint32)
    stream, offs, out_lens, counts = M.deliver(img, lens, n, n, prior, off + data.size, off, po, pl)
    assert (prior == SENT).all() and (po == 77).all()  # the model does not touch the caller's arrays
    assert np.array_equal(stream[off:off + data.size], data)
    assert (stream[:off] == SENT).all() and (stream[off + data.size:] == SENT).all()
    want_offs = off + np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    assert np.array_equal(offs[:n], want_offs) and np.array_equal(out_lens[:n], lens)
    assert (offs[n:] == 77).all() and (out_lens[n:] == 77).all()
    assert counts.tolist() == [n, n, data.size, data.size]
    for s in range(n):  # record by record: the (base, offsets, lengths) layout
        assert stream[int(offs[s]):int(offs[s]) + int(out_lens[s])].tobytes() == recs[s]
    img2, sl2 = M.slot_image(recs)
    assert np.array_equal(img2, img) and np.array_equal(sl2, lens)


def test_model_run_endings():
    recs = [bytes([i]) * ln for i, ln in enumerate([5, 0, 1456, 7, 9, 11])]
    img, sl = M.slot_image(recs, window=8)
    total = 5 + 1456 + 7 + 9 + 11
    prior = np.full(4000, SENT, np.uint8)
    assert M.deliver(img, sl, 8, 8, prior, 4000, 0)[3].tolist() == [6, 6, total, total]  # EMPTY behind the records
    for bad in (EMPTY, 1457, 0x80000005, 0x7FFFFFFF):
        s2 = sl.copy()
        s2[3] = bad  # slots 4, 5 hold valid lengths and are not delivered
        stream, _, _, counts = M.deliver(img, s2, 8, 8, prior, 4000, 0)
        assert counts.tolist() == [3, 3, 1461, 1461]
        assert stream[:1461].tobytes() == b"".join(recs[:3]) and (stream[1461:] == SENT).all()
    s2 = sl.copy()
    s2[0] = EMPTY
    stream, _, _, counts = M.deliver(img, s2, 8, 8, prior, 4000, 0)
    assert counts.tolist() == [0, 0, 0, 0] and (stream == SENT).all()
    assert M.deliver(img, sl, 0, 8, prior, 4000, 0)[3].tolist() == [0, 0, 0, 0]  # window == 0


def test_model_cuts():
    lens = [10, 0, 20, 0, 0, 30, 0, 40]
    recs = [bytes([i + 1]) * ln for i, ln in enumerate(lens)]
    img, sl = M.slot_image(recs, window=9)
    prior = np.full(200, SENT, np.uint8)
    po, pl = np.full(9, 77, np.uint64), np.full(9, 77, np.uint32)

    def run(max_slots, stream_bytes, off=0):
        return M.deliver(img, sl, 9, max_slots, prior, stream_bytes, off, po, pl)

    # max_slots
    for m, k, pk in ((0, 0, 0), (1, 1, 10), (2, 2, 10), (3, 3, 30), (8, 8, 100), (50, 8, 100)):
        stream, offs, ol, counts = run(m, 200)
        assert counts.tolist() == [k, 8, pk, 100]  # run and P_run do not depend on the cut
        assert stream[:pk].tobytes() == b"".join(recs[:k]) and (stream[pk:] == SENT).all()
        assert (offs[k:] == 77).all() and (ol[k:] == 77).all() and ol[:k].tolist() == lens[:k]
    # capacity exactly at a record boundary: the record fits, and so do the empty records behind it
    assert run(9, 7 + 30, 7)[3].tolist() == [5, 8, 30, 100]
    assert run(9, 7 + 10, 7)[3].tolist() == [2, 8, 10, 100]
    # one byte short of it: whole records only
    stream, offs, ol, counts = run(9, 7 + 29, 7)
    assert counts.tolist() == [2, 8, 10, 100] and (stream[17:] == SENT).all() and offs[:2].tolist() == [7, 17]
    # stream_off == stream_bytes: nothing with a byte fits; here slot 0 has 10
    assert run(9, 50, 50)[3].tolist() == [0, 8, 0, 100]
    # trailing zero-length records at the max_slots cut and at the end of the run
    assert run(5, 200)[3].tolist() == [5, 8, 30, 100]
    img0, sl0 = M.slot_image([b"", b"", b"abc"], window=3)
    stream, offs, ol, counts = M.deliver(img0, sl0, 3, 3, prior, 60, 60, po, pl)
    assert counts.tolist() == [2, 3, 0, 3] and offs[:2].tolist() == [60, 60] and ol[:2].tolist() == [0, 0]
    assert (stream == SENT).all()


def test_deliver_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    for name in ("wtp_rx_deliver_work_bytes", "wtp_rx_deliver"):
        assert name in W.EXPORTED and hasattr(L, name)
    buf = (C.c_uint64 * 4096)()
    a = C.addressof(buf)

    def call(**kw):
        args = dict(img=a, slot_len=a, window=4, max_slots=4, stream=a, stream_bytes=4096, stream_off=0, offsets_out=a,
                    lengths_out=a, counts=a, work=a, work_bytes=32768)
        args.update(kw)
        return L.wtp_rx_deliver(*args.values(), None)

    big = W.RX_MAX_WINDOW + 1
    assert call(window=big, work_bytes=1 << 30) == -1 and b"window 1048577 > 1048576" in L.wtp_last_error()
    assert call(stream_off=4097) == -1 and b"stream_off 4097 > stream_bytes 4096" in L.wtp_last_error()
    need = L.wtp_rx_deliver_work_bytes(4)
    assert call(work_bytes=need - 1) == -1
    assert f"work_bytes {need - 1} < {need}".encode() in L.wtp_last_error()
    for hole in ("counts", "work"):
        assert call(**{hole: None}) == -1 and f"null pointer: d_{hole}".encode() in L.wtp_last_error(), hole
    for hole in ("img", "slot_len"):
        assert call(**{hole: None}) == -1 and f"null pointer: d_{hole} with window 4".encode() in L.wtp_last_error(), hole
    assert call(stream=None) == -1 and b"null pointer: d_stream with window 4 and max_slots 4" in L.wtp_last_error()
    # the checks that do not depend on the window come first, also for window == 0
    assert call(window=0, counts=None, img=None, slot_len=None, stream=None) == -1 and b"d_counts" in L.wtp_last_error()
    assert call(window=0, stream_off=5000) == -1 and b"stream_off 5000" in L.wtp_last_error()


def test_deliver_work_bytes_is_monotone_and_bounded():
    import wtp_crc32 as W
    sizes = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4096, 70000, (1 << 20) - 1, 1 << 20]
    got = [W.rx_deliver_work_bytes(w) for w in sizes]
    assert all(b >= a for a, b in zip(got, got[1:])) and got[0] > 0
    assert all(g <= (64 << 10) + 8 * w for g, w in zip(got, sizes))
    assert W.rx_deliver_work_bytes(1 << 21) == got[-1]  # beyond the limit: the call refuses the window


def test_deliver_is_declared_in_the_header():
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+wtp_rx_deliver\s*\(([^)]*)\)", decl)
    assert m, "wtp_rx_deliver is not declared"
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["d_img", "d_slot_len", "window", "max_slots", "d_stream", "stream_bytes", "stream_off",
                      "d_offsets_out", "d_lengths_out", "d_counts", "d_work", "work_bytes", "stream"]
    m = re.search(r"size_t\s+wtp_rx_deliver_work_bytes\s*\(([^)]*)\)", decl)
    assert m and m.group(1).split()[-1] == "window"
    assert "k_deliver_copy" in src and "k_deliver_scan" in src
