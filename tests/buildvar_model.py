"""Sequential model of the mixed-length DATA builder (include/wtp_crc32.h:
wtp_build_data_packets_var), written from the header's semantics: one entry at a time over
oracle.crc32 / oracle.build_datagram, both pinned to the reference.  The caller's wire image
is never modified: a copy is returned."""
import numpy as np

import oracle as O

MAXP = 1456
HDR = 16
M32 = 0xFFFFFFFF


def is_valid(off, ln, base_bytes):
    """The header's validity rule, in unbounded integers."""
    return ln <= MAXP and off <= base_bytes and ln <= base_bytes - off


def build(base, base_bytes, offsets, lengths, seq0, wire, wire_stride):
    """Returns (wire, wire_len, crc) after the call: `wire` is the prior image of at least
    n * wire_stride bytes; entry i's slot is wire[i * wire_stride ..).  Valid entries get the
    datagram of (seq0 + i, payload) at the slot's start and (16 + len, crc32(payload));
    invalid entries leave the slot as it was and get (0, 0)."""
    base = np.asarray(base, dtype=np.uint8)
    assert base_bytes <= base.size
    n = len(offsets)
    wire = np.array(wire, dtype=np.uint8, copy=True)
    assert wire.size >= n * wire_stride
    wire_len = np.zeros(n, dtype=np.uint32)
    crc = np.zeros(n, dtype=np.uint32)
    for i in range(n):
        off, ln = int(offsets[i]), int(lengths[i])
        if not is_valid(off, ln, base_bytes):
            continue
        payload = base[off:off + ln].tobytes()
        d = O.build_datagram((seq0 + i) & M32, payload)
        assert len(d) == HDR + ln
        at = i * wire_stride
        wire[at:at + len(d)] = np.frombuffer(d, dtype=np.uint8)
        wire_len[i] = len(d)
        crc[i] = O.crc32(payload)
    return wire, wire_len, crc


def packed_offsets(lengths):
    """Back-to-back payloads: the exclusive prefix sum of the lengths, as u64."""
    lengths = np.asarray(lengths, dtype=np.uint64)
    return np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.uint64)]).astype(np.uint64) if lengths.size \
        else np.zeros(0, np.uint64)
