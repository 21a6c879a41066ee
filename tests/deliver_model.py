"""Sequential model of wtp_rx_deliver (include/wtp_crc32.h), written from the header's
semantics: the reference receiver's in-order flush (cpp/src/base/Receiver.cpp:208-237) over
accept's window state, one slot at a time.  The caller's arrays are never modified: copies
are returned."""
import numpy as np

MAXP = 1456
EMPTY = 0xFFFFFFFF


def slot_image(records, window=None, fill=0x3C):
    """(img, slot_len) of a window holding `records` (byte strings) in its leading slots."""
    window = len(records) if window is None else window
    img = np.full(window * MAXP, fill, dtype=np.uint8)
    slot_len = np.full(window, EMPTY, dtype=np.uint32)
    for s, r in enumerate(records):
        img[s * MAXP:s * MAXP + len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
        slot_len[s] = len(r)
    return img, slot_len


def deliver(img, slot_len, window, max_slots, stream, stream_bytes, stream_off, offsets_out=None, lengths_out=None):
    """Returns (stream, offsets_out, lengths_out, counts) after the call; counts = (k, run,
    P_k, P_run).  offsets_out / lengths_out: the prior arrays, or None."""
    assert stream_off <= stream_bytes <= len(stream) and len(slot_len) >= window and len(img) >= window * MAXP
    stream = np.array(stream, dtype=np.uint8, copy=True)
    offs = None if offsets_out is None else np.array(offsets_out, dtype=np.uint64, copy=True)
    lens = None if lengths_out is None else np.array(lengths_out, dtype=np.uint32, copy=True)
    run = 0
    while run < window and int(slot_len[run]) <= MAXP:
        run += 1
    P = [0]
    for s in range(run):
        P.append(P[-1] + int(slot_len[s]))
    k = 0
    while k < min(run, max_slots) and stream_off + P[k + 1] <= stream_bytes:
        k += 1
    for s in range(k):
        ln, at = int(slot_len[s]), stream_off + P[s]
        stream[at:at + ln] = img[s * MAXP:s * MAXP + ln]
        if offs is not None:
            offs[s] = at
        if lens is not None:
            lens[s] = ln
    return stream, offs, lens, np.array([k, run, P[k], P[run]], dtype=np.uint64)
