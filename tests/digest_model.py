"""The sequential statement of wtp_rx_digest_flows (include/wtp_crc32.h) in numpy, on the
oracle's crc32 and combine and never on a library call: the fold of every flow's delivered
range into its running (crc, bytes), then the report gather, then the reset."""
import numpy as np

import oracle as O

M64 = (1 << 64) - 1
NO_BYTES = M64  # d_report_bytes of an id >= nflows


def valid(b, nbytes, stream_bytes):
    """wtp_build_data_packets_var's rule, in unbounded integers: no overflow to think about."""
    return b <= stream_bytes and nbytes <= stream_bytes - b


def digest(stream, stream_bytes, info, flow_crc, flow_bytes, reset=None, reset_count=0, max_reset=0, report=None,
           report_count=0, max_report=0, report_crc=None, report_bytes=None, seg_crc=None):
    """One call.  `stream`: the host copy of d_stream (at least stream_bytes bytes); `info`:
    (nflows, 4) u64, columns 2 and 3 = B_f and bytes_f; flow_crc (u32) and flow_bytes (u64): the
    state on entry.  reset / report: sequences of ids or None (list absent), with their counts
    as the device words would hold them.  report_crc / report_bytes: the output arrays on
    entry (max_report entries or more).  seg_crc(b, n), if given, replaces crc32(stream[b : b +
    n]) (a stream too large for the host).  Returns (flow_crc, flow_bytes, report_crc,
    report_bytes, counts), all new arrays; counts = [bytes folded, flows folded, ranges refused,
    reports written]."""
    info = np.asarray(info, dtype=np.uint64).reshape(-1, 4)
    nflows = info.shape[0]
    crc, nb = np.array(flow_crc, dtype=np.uint32), np.array(flow_bytes, dtype=np.uint64)
    assert crc.size == nflows and nb.size == nflows
    if seg_crc is None:
        seg_crc = lambda b, n: O.crc32(stream[b:b + n])  # noqa: E731
    folded_bytes = folded = refused = 0
    for f in range(nflows):
        b, n = int(info[f, 2]), int(info[f, 3])
        if not valid(b, n, stream_bytes):
            refused += 1
        elif n > 0:
            # combine(0, c, n) == c for every n; the oracle's combine takes time linear in n, so a
            # zeroed state does not go through it (a range of 4 GiB would take it ten seconds)
            crc[f] = O.combine(int(crc[f]), seg_crc(b, n), n) if crc[f] else seg_crc(b, n)
            nb[f] = (int(nb[f]) + n) & M64
            folded_bytes, folded = folded_bytes + n, folded + 1
    rc = None if report_crc is None else np.array(report_crc, dtype=np.uint32)
    rb = None if report_bytes is None else np.array(report_bytes, dtype=np.uint64)
    written = 0
    if report is not None:
        written = min(int(report_count), max_report)
        for q in range(written):
            g = int(report[q])
            rc[q], rb[q] = (crc[g], nb[g]) if g < nflows else (0, NO_BYTES)
    if reset is not None:
        for j in range(min(int(reset_count), max_reset)):
            g = int(reset[j])
            if g < nflows:
                crc[g], nb[g] = 0, 0
    return crc, nb, rc, rb, np.array([folded_bytes & M64, folded, refused, written], dtype=np.uint64)


def info_of(ranges):
    """(nflows, 4) u64 from (B, bytes) pairs; words 0 and 1, which the call does not read, hold a
    pattern."""
    a = np.full((len(ranges), 4), 0x7E7E7E7E7E7E7E7E, dtype=np.uint64)
    for f, (b, n) in enumerate(ranges):
        a[f, 2], a[f, 3] = b & M64, n & M64
    return a


def scratch_bytes(nflows, max_flows=1 << 20):
    """The header's formula of wtp_rx_digest_scratch_bytes."""
    return 16432 + 12 * min(nflows, max_flows)
