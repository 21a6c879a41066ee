"""CPU checks of the window slides (wtp_rx_advance, wtp_tx_advance): the sequential models on
hand-made windows, the C-ABI's argument validation, which needs no device, and the
bounded-window streaming loop of tests/test_gpu_advance.py on the models alone, which is
where its loss pattern is shown to end within the round limit."""
import ctypes as C
import os
import re

import numpy as np

import advance_model as M
import buildvar_model as B
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXP, EMPTY = M.MAXP, M.EMPTY


def _window():
    """Six slots: 5 bytes, empty, full, a claim pattern, 0 bytes, 7 bytes."""
    lens = [5, EMPTY, MAXP, 0x80000003, 0, 7]
    img = np.arange(6 * MAXP, dtype=np.uint32).astype(np.uint8)  # every slot's bytes differ from its neighbours'
    img[:: 7] ^= 0x5A
    return img, np.array(lens, dtype=np.uint32)


def test_rx_model_on_a_hand_made_window():
    img, sl = _window()
    w = 6
    prior_img, prior_sl = np.full(w * MAXP, 0xEE, np.uint8), np.full(w + 2, 12345, np.uint32)
    for a, moved in ((0, 6), (2, 4), (6, 0), (7, 0), (1 << 32, 0), ((1 << 64) - 1, 0)):
        out, nsl = M.rx_advance(img, sl, w, a, prior_img, prior_sl)
        assert (prior_img == 0xEE).all() and (prior_sl == 12345).all()  # the model does not touch the caller's arrays
        assert nsl[:moved].tolist() == sl[w - moved:].tolist()  # every value as it is, the claim pattern too
        assert (nsl[moved:w] == EMPTY).all() and (nsl[w:] == 12345).all()
        for s in range(w):
            v = int(nsl[s])
            slot = out[s * MAXP:(s + 1) * MAXP]
            if v <= MAXP:
                t = s + min(a, w)
                assert np.array_equal(slot[:v], img[t * MAXP:t * MAXP + v])
                assert (slot[v:] == 0xEE).all()  # the tail of a placed slot stays
            else:
                assert (slot == 0xEE).all()  # a slot that receives no record stays whole
        fast = M.rx_advance_fast(img, sl, w, a, prior_img, prior_sl[:w])
        assert np.array_equal(fast[0], out) and np.array_equal(fast[1], nsl[:w])
    # the middle value by hand: slots 2 .. 5 land in 0 .. 3
    out, nsl = M.rx_advance(img, sl, w, 2, prior_img, prior_sl)
    assert nsl[:w].tolist() == [MAXP, 0x80000003, 0, 7, EMPTY, EMPTY]
    assert np.array_equal(out[:MAXP], img[2 * MAXP:3 * MAXP]) and np.array_equal(out[3 * MAXP:3 * MAXP + 7], img[5 * MAXP:5 * MAXP + 7])
    assert (out[MAXP:3 * MAXP] == 0xEE).all() and (out[3 * MAXP + 7:] == 0xEE).all()
    # state only, and a window of no slots
    assert M.rx_advance(None, sl, w, 2, None, prior_sl)[0] is None
    assert np.array_equal(M.rx_advance(None, sl, w, 2, None, prior_sl)[1], nsl)
    out, nsl = M.rx_advance(img, sl, 0, 3, prior_img, prior_sl)
    assert (out == 0xEE).all() and (nsl == 12345).all()


def test_tx_model_on_a_hand_made_window():
    acked = np.array([1, 1, 0, 1, 0, 2], dtype=np.uint32)
    sent = np.array([10, 20, 30, 40, 0xFFFFFFFF, 60], dtype=np.uint32)
    pa, ps = np.full(8, 777, np.uint32), np.full(8, 888, np.uint32)
    fill = 0xFFFFFFF0
    for a, moved in ((0, 6), (2, 4), (6, 0), (7, 0), (0xFFFFFFFF, 0)):
        ak, sm = M.tx_advance(acked, sent, 6, a, fill, pa, ps)
        assert (pa == 777).all() and (ps == 888).all()
        assert ak[:moved].tolist() == acked[6 - moved:].tolist() and (ak[moved:6] == 0).all() and (ak[6:] == 777).all()
        assert sm[:moved].tolist() == sent[6 - moved:].tolist() and (sm[moved:6] == fill).all() and (sm[6:] == 888).all()
        fast = M.tx_advance_fast(acked, sent, 6, a, fill, pa, ps)
        assert np.array_equal(fast[0], ak) and np.array_equal(fast[1], sm)
    ak, sm = M.tx_advance(acked, sent, 6, 2, fill, pa, ps)
    assert ak[:6].tolist() == [0, 1, 0, 2, 0, 0] and sm[:6].tolist() == [30, 40, 0xFFFFFFFF, 60, fill, fill]
    ak, sm = M.tx_advance(acked, sent, 0, 2, fill, pa, ps)
    assert (ak == 777).all() and (sm == 888).all()


def test_rx_advance_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    assert "wtp_rx_advance" in W.EXPORTED and hasattr(L, "wtp_rx_advance") and callable(W.rx_advance)
    w = 4
    buf = (C.c_uint8 * (1 << 16))()
    a = (C.addressof(buf) + 15) & ~15
    img, img_next = a, a + w * MAXP  # they touch: the first byte of one is the byte after the other's last
    sl, sl_next, adv = a + 32768, a + 32768 + 4 * w, a + 49152

    def call(**kw):
        args = dict(img=img, slot_len=sl, window=w, adv=adv, img_next=img_next, slot_len_next=sl_next)
        args.update(kw)
        return L.wtp_rx_advance(*args.values(), None)

    err = lambda: L.wtp_last_error().decode()  # noqa: E731
    assert call(window=W.RX_MAX_WINDOW + 1) == -1 and "window 1048577 > 1048576" in err()
    assert call(img=None) == -1 and "null pointer: d_img without d_img_next" in err()
    assert call(img_next=None) == -1 and "null pointer: d_img_next without d_img" in err()
    assert call(window=0, img=None) == -1 and "d_img without d_img_next" in err()  # whatever the window
    for hole in ("adv", "slot_len", "slot_len_next"):
        assert call(**{hole: None}) == -1 and f"null pointer: d_{hole} with window 4" in err(), hole
    # ranges that overlap by one element, either way round
    assert call(slot_len_next=sl_next - 4) == -1 and "d_slot_len_next overlaps d_slot_len (window 4)" in err()
    assert call(slot_len=sl_next, slot_len_next=sl + 4) == -1 and "d_slot_len_next overlaps d_slot_len" in err()
    assert call(slot_len_next=sl) == -1 and "d_slot_len_next overlaps d_slot_len" in err()
    assert call(img_next=img_next - 1) == -1 and "d_img_next overlaps d_img (window 4)" in err()
    assert call(img=img_next, img_next=img + 1) == -1 and "d_img_next overlaps d_img" in err()
    assert call(img_next=img) == -1 and "d_img_next overlaps d_img" in err()
    # the window's limit comes first, the state's overlap before the image's
    assert call(window=W.RX_MAX_WINDOW + 1, img=None, adv=None) == -1 and "window 1048577" in err()
    assert call(slot_len_next=sl, img_next=img) == -1 and "d_slot_len_next" in err()
    # a window of no slots launches nothing and needs no pointer
    assert L.wtp_rx_advance(None, None, 0, None, None, None, None) == 0


def test_touching_ranges_pass_the_checks_and_reach_the_launch():
    """Ranges that touch without sharing a byte are valid: with no device the call then fails
    at the launch (WTP_EHIP), with one it runs; either way it is not WTP_EINVAL."""
    import wtp_crc32 as W
    L = W.LIB
    if L.wtp_device_count() > 0:
        import pytest
        pytest.skip("a device is present: the valid call would launch on host memory")
    w = 4
    buf = (C.c_uint8 * (1 << 16))()
    a = (C.addressof(buf) + 15) & ~15
    assert L.wtp_rx_advance(a, a + 32768, w, a + 49152, a + w * MAXP, a + 32768 + 4 * w, None) == -2
    assert "k_rx_advance" in L.wtp_last_error().decode()
    assert L.wtp_rx_advance(a + w * MAXP, a + 32768 + 4 * w, w, a + 49152, a, a + 32768, None) == -2
    s = a + 32768
    assert L.wtp_tx_advance(s, s + 16, w, a + 49152, 0, s + 32, s + 48, None) == -2
    assert "k_tx_advance" in L.wtp_last_error().decode()


def test_tx_advance_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    assert "wtp_tx_advance" in W.EXPORTED and hasattr(L, "wtp_tx_advance") and callable(W.tx_advance)
    n = 4
    buf = (C.c_uint32 * 4096)()
    a = C.addressof(buf)
    acked, sent, acked_next, sent_next, adv = a, a + 4 * n, a + 8 * n, a + 12 * n, a + 8192  # four arrays back to back

    def call(**kw):
        args = dict(acked=acked, sent_ms=sent, slots=n, adv=adv, fill_ms=7, acked_next=acked_next, sent_ms_next=sent_next)
        args.update(kw)
        return L.wtp_tx_advance(*args.values(), None)

    err = lambda: L.wtp_last_error().decode()  # noqa: E731
    assert call(slots=W.TX_MAX_INFLIGHT + 1) == -1 and "slots 1048577 > 1048576" in err()
    for hole in ("adv", "acked", "sent_ms", "acked_next", "sent_ms_next"):
        assert call(**{hole: None}) == -1 and f"null pointer: d_{hole} with slots 4" in err(), hole
    assert call(acked_next=sent + 4 * n - 4) == -1 and "d_acked_next overlaps d_sent_ms (slots 4)" in err()  # by one element
    assert call(acked_next=acked) == -1 and "d_acked_next overlaps d_acked" in err()
    z = a + 2048  # away from the four arrays: one element shared at either end
    assert call(acked=z, acked_next=z + 4 * n - 4) == -1 and "d_acked_next overlaps d_acked (slots 4)" in err()
    assert call(acked=z, acked_next=z - 4 * n + 4) == -1 and "d_acked_next overlaps d_acked (slots 4)" in err()
    assert call(sent_ms=z, sent_ms_next=z + 4 * n - 4) == -1 and "d_sent_ms_next overlaps d_sent_ms (slots 4)" in err()
    assert call(acked=z, sent_ms_next=z - 4 * n + 4) == -1 and "d_sent_ms_next overlaps d_acked (slots 4)" in err()
    assert call(acked_next=z, sent_ms_next=z + 4 * n - 4) == -1 and "d_sent_ms_next overlaps d_acked_next (slots 4)" in err()
    assert L.wtp_tx_advance(None, None, 0, None, 0, None, None, None) == 0


def test_both_calls_are_declared_in_the_header():
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+wtp_rx_advance\s*\(([^)]*)\)", decl)
    assert m, "wtp_rx_advance is not declared"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == [
        "d_img", "d_slot_len", "window", "d_adv", "d_img_next", "d_slot_len_next", "stream"]
    assert "const uint64_t *d_adv" in m.group(1)
    m = re.search(r"int\s+wtp_tx_advance\s*\(([^)]*)\)", decl)
    assert m, "wtp_tx_advance is not declared"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == [
        "d_acked", "d_sent_ms", "slots", "d_adv", "fill_ms", "d_acked_next", "d_sent_ms_next", "stream"]
    assert "const uint32_t *d_adv" in m.group(1)
    assert decl.index("wtp_rx_deliver(") < decl.index("wtp_rx_advance(") < decl.index("wtp_tx_advance(")
    assert "k_rx_advance" in src and "k_tx_advance" in src


def stream_source():
    """The records of the streaming round trip and their datagrams from the builder's model."""
    n, seq0 = M.STREAM_RECORDS, M.STREAM_SEQ0
    lens = O.zipf_lengths(n, seed=77)
    lens[5:9] = [0, 1456, 0, 1]
    offs = B.packed_offsets(lens)
    total = int(lens.sum())
    host = O.synth_fill_np(total, start_byte=3)
    stride = 1472
    wire, wl, _ = B.build(host, total, offs, lens, seq0, np.zeros(n * stride, np.uint8), stride)
    return host, offs, lens, wire, wl, stride


def test_bounded_window_stream_on_the_models():
    """2000 records, sequence numbers that wrap, through a receiver of two 256-slot window
    states and 5 % loss: the loop ends within its round limit and gives the source stream."""
    host, offs, lens, wire, wl, stride = stream_source()
    end = M.ModelStreamEnd(wire, wl, stride, M.STREAM_SEQ0, M.STREAM_WINDOW, host.size)
    rounds = M.stream_rounds(end)
    assert len(rounds) <= M.STREAM_MAX_ROUNDS and sum(r[0] for r in rounds) == M.STREAM_RECORDS
    assert len(rounds) > M.STREAM_RECORDS // M.STREAM_WINDOW  # the losses cost rounds
    assert max(r[0] for r in rounds) <= M.STREAM_WINDOW and any(r[0] < M.STREAM_WINDOW // 2 for r in rounds)
    assert np.array_equal(end.stream, host)
    assert np.array_equal(np.array(end.offs, np.uint64), offs) and np.array_equal(np.array(end.lens, np.uint32), lens)
    assert all(a.size == M.STREAM_WINDOW * MAXP for a in end.img) and all(s.size == M.STREAM_WINDOW for s in end.sl)
