"""Sequential model of wtp_accept_data_packets (include/wtp_crc32.h): the arrival-order
loop of the reference's receiver (cpp/src/base/Receiver.cpp:25-35, :208-237) over a
window the caller owns.  ok comes from oracle.verify_datagrams, pinned to the reference."""
import numpy as np

import oracle as O

MAXP = 1456
EMPTY = 0xFFFFFFFF
NOT_PLACED = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def accept(ring, stride, recv_len, seq0, window, out, slot_len):
    """Returns (ok, place, out, slot_len, ack); `out` / `slot_len` are the window state on
    entry (not modified: copies are returned)."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    n = recv_len.size
    out, slot_len = out.copy(), slot_len.copy()
    ok = O.verify_datagrams(ring, stride, recv_len)[0] if n else np.zeros(0, np.uint8)
    place = np.full(n, NOT_PLACED, dtype=np.uint32)
    for i in range(n):
        if not ok[i]:
            continue
        d = ring[i * stride:i * stride + int(recv_len[i])]
        ln = d.size - 16
        s = (int.from_bytes(d[4:8].tobytes(), "big") - seq0) & M32
        if int.from_bytes(d[0:4].tobytes(), "big") != 2 or ln > MAXP or s >= window or slot_len[s] != EMPTY:
            continue
        out[s * MAXP:s * MAXP + ln] = d[16:]
        slot_len[s] = ln
        place[i] = s
    lead = 0
    while lead < window and slot_len[lead] != EMPTY:
        lead += 1
    return ok, place, out, slot_len, (seq0 + lead) & M32
