"""CPU tests of tests/flows_model.py, the models of wtp_accept_data_packets_flows and
wtp_rx_build_acks_flows: the properties that define the calls, the conditions on the fuzz
corpus that keep the GPU fuzz from passing vacuously, and the multi-flow transfer on the
models alone."""
import numpy as np
import pytest

import accept_model
import ack_model as A
import flows_model as F
import oracle as O

MAXP, EMPTY, M32 = F.MAXP, F.EMPTY, F.M32


@pytest.fixture(scope="module")
def corpus():
    return {seed: F.fuzz_calls(seed) for seed in F.FUZZ_SEEDS}


def test_reinterleaving_flows_changes_nothing_but_the_order(corpus):
    """Another arrival order with every flow's own order kept: the same image, slot_len and
    ACKs; ok and place move with their datagrams."""
    for seed, (calls, (nflows, window, seq0, stride, _, _)) in corpus.items():
        rng = np.random.default_rng(seed)
        for c in calls:
            perm = F.reinterleave(rng, c["flow"])
            assert not np.array_equal(perm, np.arange(perm.size))
            got = F.accept_flows(F.rows(c["ring"], stride, perm), stride, c["rl"][perm], c["flow"][perm], seq0, nflows, window,
                                 c["out0"], c["sl0"])
            ok, place, out, sl, ack = c["want"]
            assert np.array_equal(got[0], ok[perm]) and np.array_equal(got[1], place[perm])
            assert np.array_equal(got[2], out) and np.array_equal(got[3], sl) and np.array_equal(got[4], ack)


def test_one_flow_is_accept_and_selective_build_acks():
    for seed in accept_model.FUZZ_SEEDS:
        rng, window, seq0, stride, _, _, ns = accept_model.fuzz_case(seed)
        out, sl = np.full(window * MAXP, 0xA5, np.uint8), np.full(window, EMPTY, np.uint32)
        for n in ns:
            ring, rl, _ = accept_model.fuzz_batch(rng, seq0, window, stride, sl, n)
            want = accept_model.accept(ring, stride, rl, seq0, window, out, sl)
            got = F.accept_flows(ring, stride, rl, np.zeros(n, np.uint32), [seq0], 1, window, out, sl)
            for g, w in zip(got[:4], want[:4]):
                assert np.array_equal(g, w)
            assert got[4].tolist() == [want[4]]
            for skip, max_acks in ((0, None), (3, 5)):
                a = F.build_acks_flows(ring, stride, rl, np.zeros(n, np.uint32), F.SELECTIVE, [seq0], 1, window, want[0],
                                       skip=skip, max_acks=max_acks)
                b = A.build_acks(ring, stride, rl, A.SELECTIVE, seq0, window, ok=want[0], skip=skip, max_acks=max_acks)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            out, sl = want[2], want[3]


def test_cumulative_acks_carry_the_flows_ack(corpus):
    for calls, (nflows, window, seq0, stride, _, _) in corpus.values():
        for c in calls:
            ok, _, _, _, ack = c["want"]
            seq, src, (emitted, total) = F.build_acks_flows(c["ring"], stride, c["rl"], c["flow"], F.CUMULATIVE, seq0, nflows,
                                                            window, ok, ack)
            assert emitted == total > nflows
            assert np.array_equal(seq, ack[c["flow"][src]])
            assert set(c["flow"][src].tolist()) == set(range(nflows))  # every flow is answered, no other
            sel = F.build_acks_flows(c["ring"], stride, c["rl"], c["flow"], F.SELECTIVE, seq0, nflows, window, ok)
            assert np.array_equal(sel[1], src) and np.array_equal(sel[0], A.headers(c["ring"], stride, c["rl"].size)[1][src])


def test_datagrams_of_no_connection_are_verified_and_nothing_else(corpus):
    for calls, (nflows, *_rest) in corpus.values():
        for c in calls:
            ok, place = c["want"][0], c["want"][1]
            none = c["flow"] >= nflows
            assert none.any() and ok[none].any() and (place[none] == F.NOT_PLACED).all()
            assert {int(f) for f in c["flow"][none]} <= {nflows, F.NO_FLOW}


def test_corpus_conditions(corpus):
    """What the GPU fuzz relies on: every kind of datagram occurs, alone on a datagram and with
    the verdict it stands for, in at least two different flows; some seqNum is placed in two
    flows in one batch; some flow's base lies within 3 of 2^32."""
    seen = {k: set() for k in accept_model.FUZZ_KINDS}
    same_seq = near_wrap = 0
    for seed, (calls, (nflows, window, seq0, stride, _, _)) in corpus.items():
        near_wrap += any((1 << 32) - int(s) <= 3 for s in seq0)
        for c in calls:
            ok, place, _, sl, _ = c["want"]
            _, seqs = A.headers(c["ring"], stride, c["rl"].size)
            placed = {}
            for i, kinds in enumerate(c["kinds"]):
                f = int(c["flow"][i])
                if f >= nflows:
                    continue
                was_placed = place[i] != F.NOT_PLACED
                if was_placed:
                    placed.setdefault(int(seqs[i]), set()).add(f)
                if len(kinds) == 1:
                    kind = next(iter(kinds))
                    stored = int(sl[f * window + place[i]]) if was_placed else None
                    if accept_model.fuzz_verdict(kind, bool(ok[i]), was_placed, int(c["rl"][i]), stored):
                        seen[kind].add((seed, f))  # "dup_filled" finds a filled slot from the second call on
            same_seq += any(len(fl) > 1 for fl in placed.values())
    assert all(len({f for _, f in s}) >= 2 for s in seen.values()), {k: len(s) for k, s in seen.items()}
    assert same_seq >= 1 and near_wrap >= 1


def test_ring_limits_of_the_ack_model(corpus):
    calls, (nflows, window, seq0, stride, _, _) = corpus[0]
    c = calls[0]
    ok, ack = c["want"][0], c["want"][4]
    seq, src, (e, _) = F.build_acks_flows(c["ring"], stride, c["rl"], c["flow"], F.CUMULATIVE, seq0, nflows, window, ok, ack)
    for skip, max_acks in ((0, 0), (1, 3), (e - 1, 5), (e, 1), (e + 2, 1)):
        s, i, counts = F.build_acks_flows(c["ring"], stride, c["rl"], c["flow"], F.CUMULATIVE, seq0, nflows, window, ok, ack,
                                          skip=skip, max_acks=max_acks)
        assert counts == (min(max(e - skip, 0), max_acks), e)
        assert np.array_equal(s, seq[skip:skip + max_acks]) and np.array_equal(i, src[skip:skip + max_acks])


@pytest.mark.parametrize("mode", [F.SELECTIVE, F.CUMULATIVE])
def test_transfer_on_the_models(mode):
    """The chosen seed finishes within the round cap, every flow sees a loss, a duplicate and an
    out-of-order arrival, and the four delivered streams are the sources."""
    end = F.ModelEnd()
    log, stats = F.transfer(end, mode)
    assert len(log) <= F.XFER_MAX_ROUNDS and (stats >= 1).all(), (len(log), stats)
    for f in range(F.XFER_FLOWS):
        lens, offs, total, host = end.rec[f]
        assert np.array_equal(end.stream[f], host)
        assert np.array_equal(np.array(end.offs[f], np.uint64), offs) and np.array_equal(np.array(end.lens[f], np.uint32), lens)
    assert O.crc32(end.stream[1]) == O.crc32(end.rec[1][3])
