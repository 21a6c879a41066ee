"""CPU checks of the multi-connection flush and slide (wtp_rx_deliver_flows,
wtp_rx_advance_flows): the sequential model of tests/flows_flush_model.py against
deliver_model and advance_model for one flow and for flows that all fit, its cuts and run
endings by hand, and the four-connection transfer with one flush per round, which is where
that loop is shown to take flows_model.ModelEnd's rounds."""
import numpy as np

import advance_model as V
import deliver_model as D
import flows_flush_model as M
import flows_model as F
import test_advance_model as TA
import test_deliver_model as TD

MAXP, EMPTY, SENT = M.MAXP, M.EMPTY, 0xA5


def state(lens_per_flow, window, seed=1):
    """(img, slot_len, records[f][s]) of flows whose leading slots hold records of these lengths
    (a value above 1456 is stored as it is and holds no record); every byte differs by flow."""
    rng = np.random.default_rng(seed)
    nf = len(lens_per_flow)
    img = np.full(nf * window * MAXP, 0x3C, np.uint8)
    sl = np.full(nf * window, EMPTY, np.uint32)
    recs = []
    for f, lens in enumerate(lens_per_flow):
        recs.append([])
        for s, ln in enumerate(lens):
            g = f * window + s
            sl[g] = ln
            r = rng.integers(0, 256, ln if ln <= MAXP else 0, dtype=np.uint8)
            img[g * MAXP:g * MAXP + r.size] = r
            recs[f].append(r.tobytes())
    return img, sl, recs


def test_one_flow_is_deliver_model_on_its_corpus(golden_dir):
    data = TD._file(golden_dir)
    recs, lens = TD._cut(data)
    img, sl = D.slot_image(recs, window=lens.size + 3)
    w = lens.size + 3
    sl[lens.size + 1] = 7  # behind the run's end
    prior = np.full(data.size + 40, SENT, np.uint8)
    po, pl = np.full(w + 2, 77, np.uint64), np.full(w + 2, 77, np.uint32)
    for max_slots, cap, off in ((w, data.size + 9, 9), (5, data.size, 0), (w, data.size - 1, 0), (w, 3000, 1500), (0, 50, 50)):
        want = D.deliver(img, sl, w, max_slots, prior, cap, off, po, pl)
        got = M.deliver_flows(img, sl, 1, w, max_slots, prior, cap, off, po, pl)
        assert all(np.array_equal(a, b) for a, b in zip(want[:3], got[:3]))
        assert np.array_equal(got[5], want[3]) and got[3].tolist() == [int(want[3][0])]
        assert got[4].tolist() == [[int(want[3][1]), 0, off, int(want[3][2])]]
    assert (prior == SENT).all() and (po == 77).all()  # the model does not touch the caller's arrays


def test_one_flow_is_advance_model_on_its_corpus():
    img, sl = TA._window()
    w = 6
    prior_img, prior_sl = np.full(w * MAXP, 0xEE, np.uint8), np.full(w, 12345, np.uint32)
    for a in (0, 2, 6, 7, 1 << 32, (1 << 64) - 1):
        want = V.rx_advance(img, sl, w, a, prior_img, prior_sl)
        for fast in (False, True):
            got = M.advance_flows(img, sl, 1, w, [a], [0xFFFFFFFE], prior_img, prior_sl, [5], fast=fast)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert got[2].tolist() == [(0xFFFFFFFE + min(a, w)) & 0xFFFFFFFF]
        got = M.advance_flows(None, sl, 1, w, [a], None, None, prior_sl, None)
        assert got[0] is None and got[2] is None and np.array_equal(got[1], want[1])
    out, nsl, sq = M.advance_flows(img, sl, 3, 0, [1, 1, 1], [7, 8, 9], prior_img, prior_sl, [1, 2, 3])
    assert (out == 0xEE).all() and (nsl == 12345).all() and sq.tolist() == [1, 2, 3]  # no slots: nothing is written


LENS3 = ([10, 0, 20], [0, 30, 0, 40, 5], [7, 1456])  # flow 1 has zero-length records around its bytes
TOTAL3 = [30, 75, 1463]


def test_everything_fits_is_the_per_flow_loop():
    w = 6
    img, sl, recs = state(LENS3, w)
    sl[0 * w + 4], sl[2 * w + 3] = 9, 0  # behind each run's end
    cap, off = 4000, 11
    prior = np.full(cap + 8, SENT, np.uint8)
    stream, offs, lens, adv, info, counts = M.deliver_flows(img, sl, 3, w, w, prior, cap, off, np.full(20, 77, np.uint64),
                                                            np.full(20, 77, np.uint32))
    loop, at, rank = prior, off, 0
    for f in range(3):
        loop, o, ln, c = D.deliver(img[f * w * MAXP:(f + 1) * w * MAXP], sl[f * w:(f + 1) * w], w, w, loop, cap, at,
                                   np.zeros(w, np.uint64), np.zeros(w, np.uint32))
        k = int(c[0])
        assert k == len(LENS3[f]) == int(adv[f]) and info[f].tolist() == [k, rank, at, TOTAL3[f]]
        assert np.array_equal(offs[rank:rank + k], o[:k]) and np.array_equal(lens[rank:rank + k], ln[:k])
        at, rank = at + int(c[2]), rank + k
    assert np.array_equal(stream, loop) and counts.tolist() == [10, 10, sum(TOTAL3), sum(TOTAL3)]
    assert stream[off:at].tobytes() == b"".join(b"".join(r) for r in recs) and (stream[at:] == SENT).all()
    assert (offs[10:] == 77).all() and (lens[10:] == 77).all()
    # the sums of flow_info are d_counts
    assert info[:, 0].sum() == counts[1] and info[:, 3].sum() == counts[2] and adv.sum() == counts[0]
    assert info[2, 1] + adv[2] == counts[0] and info[2, 2] + info[2, 3] == off + counts[2]


def test_capacity_cuts():
    w = 6
    img, sl, recs = state(LENS3, w)
    prior = np.full(5000, SENT, np.uint8)
    off = 3

    def run(room):
        r = M.deliver_flows(img, sl, 3, w, w, prior, off + room, off, np.full(12, 77, np.uint64), np.full(12, 77, np.uint32))
        stream, offs, lens, adv, info, counts = r
        K, qk = int(counts[0]), int(counts[2])
        assert (stream[:off] == SENT).all() and (stream[off + qk:] == SENT).all() and (offs[K:] == 77).all()
        assert counts[1] == 10 and counts[3] == sum(TOTAL3)  # the runs do not depend on the cut
        assert info[:, 3].sum() == qk and adv.sum() == K and info[:, 0].tolist() == [3, 5, 2]
        return adv.tolist(), info[:, 1:].tolist(), [K, qk]

    # inside flow 1 at a record boundary: its 30 bytes fit exactly, and so does the empty record behind them
    assert run(60) == ([3, 3, 0], [[0, off, 30], [3, off + 30, 30], [6, off + 60, 0]], [6, 60])
    # one byte short: flow 1 keeps its leading empty record; flow 2 delivers nothing though its 7 bytes would fit
    assert run(59) == ([3, 1, 0], [[0, off, 30], [3, off + 30, 0], [4, off + 30, 0]], [4, 30])
    assert run(99) == ([3, 3, 0], [[0, off, 30], [3, off + 30, 30], [6, off + 60, 0]], [6, 60])  # 40 do not fit, 7 would
    # exactly at a flow boundary: all of flow 1, nothing of flow 2
    assert run(105) == ([3, 5, 0], [[0, off, 30], [3, off + 30, 75], [8, off + 105, 0]], [8, 105])
    assert run(111) == ([3, 5, 0], [[0, off, 30], [3, off + 30, 75], [8, off + 105, 0]], [8, 105])
    assert run(112) == ([3, 5, 1], [[0, off, 30], [3, off + 30, 75], [8, off + 105, 7]], [9, 112])
    # no room at all: flow 0's first record has bytes
    assert run(0) == ([0, 0, 0], [[0, off, 0], [0, off, 0], [0, off, 0]], [0, 0])
    # the bytes delivered are the records' in flow order
    stream = M.deliver_flows(img, sl, 3, w, w, prior, off + 59, off)[0]
    assert stream[off:off + 30].tobytes() == b"".join(recs[0])


def test_the_loop_free_plan_is_the_model():
    rng = np.random.default_rng(0x91A)
    for nf, w in ((1, 9), (4, 7), (9, 1), (0, 5), (5, 0), (6, 13)):
        sl = rng.choice([0, 1, 2, 40, 1456, 1457, EMPTY, 0x80000002], nf * w, p=[.2, .2, .1, .15, .15, .05, .1, .05]).astype(np.uint32)
        img = rng.integers(0, 256, nf * w * MAXP, dtype=np.uint8)
        for max_slots, room, off in ((w, 1 << 20, 0), (3, 1 << 20, 5), (w, 1500, 9), (w, 41, 0), (w, 0, 7), (0, 99, 1)):
            prior = np.full(off + min(room, 30000) + 8, SENT, np.uint8)
            cap = prior.size - 8
            _, offs, lens, adv, info, counts = M.deliver_flows(img, sl, nf, w, max_slots, prior, cap, off, np.zeros(nf * w, np.uint64),
                                                               np.zeros(nf * w, np.uint32))
            g, Q, ln, adv2, info2, counts2 = M.deliver_flows_plan(sl, nf, w, max_slots, cap, off)
            K = int(counts[0])
            assert np.array_equal(counts, counts2) and np.array_equal(adv, adv2) and np.array_equal(info, info2)
            assert g.size == K and np.array_equal(offs[:K], (Q + off).astype(np.uint64)) and np.array_equal(lens[:K], ln)
            assert all(int(sl[x]) == int(v) for x, v in zip(g, ln))


def test_max_slots_cuts_every_flow():
    w = 6
    img, sl, recs = state(LENS3, w)
    prior = np.full(5000, SENT, np.uint8)
    for m, ks in ((0, [0, 0, 0]), (1, [1, 1, 1]), (2, [2, 2, 2]), (3, [3, 3, 2]), (w, [3, 5, 2]), (50, [3, 5, 2])):
        stream, _, lens, adv, info, counts = M.deliver_flows(img, sl, 3, w, m, prior, 5000, 0, None, np.zeros(10, np.uint32))
        assert adv.tolist() == ks and info[:, 0].tolist() == [3, 5, 2] and counts[1] == 10 and counts[3] == sum(TOTAL3)
        want = b"".join(b"".join(recs[f][:ks[f]]) for f in range(3))
        assert stream[:len(want)].tobytes() == want and counts[2] == len(want) and (stream[len(want):] == SENT).all()
        assert lens[:sum(ks)].tolist() == [ln for f in range(3) for ln in LENS3[f][:ks[f]]]


def test_run_endings_per_flow():
    w = 4
    for bad in (EMPTY, 1457, 0x80000005):
        img, sl, recs = state(([5, 6, 7, 8], [5, 6, 7, 8], [5, 6, 7, 8], [5, 6, 7, 8]), w)
        sl[0 * w + 0], sl[1 * w + 2], sl[3 * w + 3] = bad, bad, bad  # at slot 0, in the middle, nowhere, at the last slot
        _, _, _, adv, info, counts = M.deliver_flows(img, sl, 4, w, w, np.full(200, SENT, np.uint8), 200, 0)
        assert adv.tolist() == [0, 2, 4, 3] and info[:, 0].tolist() == [0, 2, 4, 3]
        assert counts.tolist() == [9, 9, 11 + 26 + 18, 11 + 26 + 18]
        assert info[:, 1].tolist() == [0, 0, 2, 6] and info[:, 2].tolist() == [0, 0, 11, 37]


def test_advance_of_every_kind_in_one_call():
    w = 5
    lens = ([3, 4, EMPTY, 1456, 0], [1, 2, 3, 4, 5], [0x80000001, 9, 9, 9, 9], [6, EMPTY, 6, EMPTY, 6], [1456] * 5)
    img, sl, _ = state(lens, w)
    advs = [0, 1, w, w + 1, 1 << 40]
    seq0 = np.array([0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFC, 5], np.uint32)  # within 3 of 2^32: they wrap
    prior_img, prior_sl, prior_sq = np.full(5 * w * MAXP, 0xEE, np.uint8), np.full(5 * w, 12345, np.uint32), np.full(5, 9, np.uint32)
    out, nsl, sq = M.advance_flows(img, sl, 5, w, advs, seq0, prior_img, prior_sl, prior_sq)
    assert (prior_img == 0xEE).all() and (prior_sq == 9).all()
    assert sq.tolist() == [0xFFFFFFFD, 0, 3, 1, 10]
    assert nsl.tolist() == [3, 4, EMPTY, 1456, 0] + [2, 3, 4, 5, EMPTY] + [EMPTY] * 15
    assert np.array_equal(out[:3], img[:3]) and (out[3:MAXP] == 0xEE).all() and (out[2 * MAXP:3 * MAXP] == 0xEE).all()
    assert np.array_equal(out[5 * MAXP:5 * MAXP + 2], img[6 * MAXP:6 * MAXP + 2]) and (out[10 * MAXP:] == 0xEE).all()
    assert np.array_equal(M.advance_flows(img, sl, 5, w, advs, seq0, prior_img, prior_sl, prior_sq, fast=True)[0], out)


def test_transfer_with_one_flush_per_round_takes_the_same_rounds():
    for mode in (F.SELECTIVE, F.CUMULATIVE):
        ref, new = F.ModelEnd(), M.FlushEnd()
        want, _ = F.transfer(ref, mode)
        got, _ = F.transfer(new, mode)
        assert got == want and len(got) <= F.XFER_MAX_ROUNDS
        for f in range(F.XFER_FLOWS):
            lens, offs, total, host = new.rec[f]
            assert np.array_equal(new.stream[f], host) and np.array_equal(new.stream[f], ref.stream[f])
            assert new.offs[f] == ref.offs[f] == offs.tolist() and new.lens[f] == ref.lens[f] == lens.tolist()
