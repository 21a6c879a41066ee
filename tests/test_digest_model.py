"""tests/digest_model.py against the oracle alone: the per-flow result over several rounds is
the CRC of each flow's whole file, fold -> report -> reset happen in that order, refused ranges
and list clamping are what include/wtp_crc32.h states."""
import numpy as np

import digest_model as M
import oracle as O


def rounds_of(files, cuts, rng):
    """Per round the (B, bytes) of every flow in one packed stream: flow f delivers bytes
    cuts[f][r] .. cuts[f][r + 1] of its file, the flows in a shuffled order with gaps between."""
    out = []
    for r in range(len(cuts[0]) - 1):
        parts, ranges, at = [], [None] * len(files), 0
        for f in rng.permutation(len(files)):
            seg = files[f][cuts[f][r]:cuts[f][r + 1]]
            gap = rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8)
            parts += [gap, seg]
            ranges[f] = (at + gap.size, seg.size)
            at += gap.size + seg.size
        out.append((np.concatenate(parts) if at else np.zeros(0, np.uint8), ranges))
    return out


def test_rounds_give_each_files_crc():
    rng = np.random.default_rng(1)
    files = [rng.integers(0, 256, n, dtype=np.uint8) for n in (0, 1, 2, 4096, 70001, 1456 * 9 + 5)]
    # rounds that deliver nothing for a flow, or for every flow (round 2), and one that delivers everything
    cuts = [sorted([0, n] + rng.integers(0, n + 1, 3).tolist()) + [n] for n in (f.size for f in files)]
    for c in cuts:
        c.insert(2, c[2])
    ref = O.ref_lib()
    crc, nb = np.zeros(len(files), np.uint32), np.zeros(len(files), np.uint64)
    total = 0
    for stream, ranges in rounds_of(files, cuts, rng):
        crc, nb, _, _, counts = M.digest(stream, stream.size, M.info_of(ranges), crc, nb)
        total += int(counts[0])
        assert int(counts[0]) == sum(n for _, n in ranges) and int(counts[1]) == sum(n > 0 for _, n in ranges) and counts[2] == 0
    assert total == sum(f.size for f in files)
    for f, data in enumerate(files):
        assert int(crc[f]) == O.crc32(data) and int(nb[f]) == data.size
        if ref is not None:  # the reference's own crc32
            assert int(crc[f]) == int(ref.ref_crc32(data.ctypes.data, data.size)) & 0xFFFFFFFF
    assert crc[0] == 0  # the empty file


def test_fold_then_report_then_reset():
    stream = np.arange(100, dtype=np.uint8)
    info = M.info_of([(0, 10), (10, 0), (50, 50)])
    crc0, nb0 = np.array([0, 7, 9], np.uint32), np.array([0, 70, 1 << 40], np.uint64)
    sent = dict(report_crc=np.full(5, 0xAAAA, np.uint32), report_bytes=np.full(5, 0xBBBB, np.uint64))
    crc, nb, rc, rb, counts = M.digest(stream, 100, info, crc0, nb0, reset=[2, 2, 9, 0], reset_count=3, max_reset=4,
                                       report=[2, 1, 3, 0], report_count=3, max_report=5, **sent)
    folded2 = O.combine(9, O.crc32(stream[50:]), 50)
    # the report sees the folded values, the reset comes after it; ids >= nflows report (0, ~0) and reset nothing
    assert rc.tolist() == [folded2, 7, 0, 0xAAAA, 0xAAAA] and rb.tolist() == [(1 << 40) + 50, 70, M.NO_BYTES, 0xBBBB, 0xBBBB]
    assert crc.tolist() == [O.crc32(stream[:10]), 7, 0] and nb.tolist() == [10, 70, 0]  # flow 0 is past reset_count
    assert counts.tolist() == [60, 2, 0, 3]
    assert crc0.tolist() == [0, 7, 9]  # the inputs are not modified


def test_refused_ranges_and_clamping():
    stream = np.arange(64, dtype=np.uint8)
    big = (1 << 64) - 1
    ranges = [(65, 0), (64, 0), (64, 1), (0, 65), (big, big), (big - 3, 8), (60, 4), (0, 64)]
    crc0 = np.arange(1, 9, dtype=np.uint32)
    crc, nb, rc, rb, counts = M.digest(stream, 64, M.info_of(ranges), crc0, np.full(8, 3, np.uint64), report=[6] * 4, report_count=9,
                                       max_report=2, report_crc=np.zeros(4, np.uint32), report_bytes=np.zeros(4, np.uint64),
                                       reset=[7, 6], reset_count=1, max_reset=0)
    assert counts.tolist() == [68, 2, 5, 2]  # (64, 0) is valid and empty; the report count is clamped to max_report
    assert crc[:6].tolist() == [1, 2, 3, 4, 5, 6] and nb[:6].tolist() == [3] * 6
    assert int(crc[6]) == O.combine(7, O.crc32(stream[60:]), 4) and int(crc[7]) == O.combine(8, O.crc32(stream), 64)  # max_reset 0
    assert rc.tolist() == [int(crc[6])] * 2 + [0, 0] and rb.tolist() == [7, 7, 0, 0]
    # absent lists write nothing and count nothing
    out = M.digest(stream, 64, M.info_of(ranges), crc0, np.full(8, 3, np.uint64))
    assert out[2] is None and out[3] is None and out[4].tolist() == [68, 2, 5, 0]
    assert M.digest(stream, 64, M.info_of([]), [], [], report=[0], report_count=1, max_report=1, report_crc=[5],
                    report_bytes=[5])[2:4] == (np.array([0], np.uint32), np.array([M.NO_BYTES], np.uint64))


def test_one_flow_is_the_whole_buffer_crc():
    """nflows == 1, zeroed state, any rounds: the CRC of the concatenation."""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 30000, dtype=np.uint8)
    crc, nb = [0], [0]
    cuts = [0, 0, 1, 1457, 1457, 20000, 30000]
    for a, e in zip(cuts, cuts[1:]):
        crc, nb = M.digest(data, data.size, M.info_of([(a, e - a)]), crc, nb)[:2]
    assert int(crc[0]) == O.crc32(data) and int(nb[0]) == 30000
    # the identity behind the model's shortcut for a zeroed state
    for c, n in ((0x12345678, 1), (0xFFFFFFFF, 1456), (1, 70001), (O.crc32(data), 1 << 20)):
        assert O.combine(0, c, n) == c
