"""CPU tests of tests/conn_model.py, the sequential model of wtp_flows_classify and
wtp_flows_control: against a second restatement that keeps one wReceiver.cpp-style connection
record per key (open, start_seq) and handles one datagram at a time, over the fuzz corpus and
the directed cases; every verdict is reached; with the library's wtp_conn_bucket the corpus
overflows no bucket, so the GPU test's exact comparison applies to every fuzz round."""
import numpy as np
import pytest

import conn_model as M


def lib_bucket():
    import wtp_crc32 as W
    return W.conn_bucket


def low_bits(key, nbuckets):
    """A bucket function of the tests' own: the port's low bits."""
    return key[3] & (nbuckets - 1)


class Conn:
    """One key's connection as wReceiver.cpp keeps it (199-254: open, start_seq), and what
    this batch did to it."""

    def __init__(self, flow=None, start_seq=None):
        self.open, self.flow, self.start_seq = flow is not None, flow, start_seq
        self.was_open = self.open          # the entry snapshot: d_flow[i] < nflows
        self.refused = None                # the first START's refusal in this batch
        self.closed_now = False


def restate(st, ring, stride, keys, ok, bucket_of, max_acks):
    """The same call, one datagram at a time on per-key records: (verdict, ack_src, opened,
    closed, table, free ids in FIFO order)."""
    n, nflows, window, nb = len(keys), st.nflows, st.window, st.nbuckets
    conns = {k: Conn(f, int(st.flow_start[f])) for k, f in st.table.items()}
    used = [0] * nb
    for k in conns:
        used[bucket_of(k, nb)] += 1
    ids = st.free_ids()
    returned, opened, closed = [], [], []
    verdict = [M.NONE] * n
    for kind in (M.START, M.END):
        for i in range(n):
            if not ok[i]:
                continue
            ptype, seq = M.header(ring, stride, i)
            if ptype != kind:
                continue
            c = conns.setdefault(keys[i], Conn())
            if kind == M.START:
                if c.open:  # "if (open && h.seqNum != start_seq) continue;", else the ACK goes out again
                    verdict[i] = M.START_DUP if seq == c.start_seq else M.START_OTHER
                elif c.refused is not None:
                    verdict[i] = c.refused
                elif nflows and used[bucket_of(keys[i], nb)] == M.WAYS:
                    verdict[i] = c.refused = M.REFUSED_BUCKET
                elif not ids:
                    verdict[i] = c.refused = M.REFUSED_FULL
                else:  # "if (!open) { open = true; start_seq = h.seqNum; expected = 0; ... }"
                    c.open, c.start_seq, c.flow = True, seq, ids.pop(0)
                    used[bucket_of(keys[i], nb)] += 1
                    opened.append(c.flow)
                    verdict[i] = M.OPENED
            else:
                if not c.was_open:  # also a connection opened by this batch: its datagrams carry no flow
                    verdict[i] = M.END_STALE
                elif seq != c.start_seq:  # "if (h.seqNum != start_seq) continue;"
                    verdict[i] = M.END_OTHER
                elif window and st.slot_len[c.flow * window] != M.EMPTY:
                    verdict[i] = M.END_BUSY
                elif c.closed_now:  # "if (!open) { send_ack(...); continue; }"
                    verdict[i] = M.END_STALE
                else:
                    c.open, c.closed_now = False, True
                    returned.append(c.flow)
                    closed.append(c.flow)
                    verdict[i] = M.CLOSED
    ans = [i for i in range(n) if verdict[i] in M.ANSWERED]
    table = {k: c.flow for k, c in conns.items() if c.open}
    return verdict, ans[:max_acks], opened, closed, table, ids + returned


def compare(entry, ring, stride, keys, ok, flow, max_acks, want, bucket_of):
    verdict, ack_src, opened, closed, table, ids = restate(entry, ring, stride, keys, ok, bucket_of, max_acks)
    assert verdict == want["verdict"].tolist()
    assert ack_src == want["ack_src"].tolist() and opened == want["opened"].tolist() and closed == want["closed"].tolist()
    after = want["state"]
    assert table == after.table and ids == after.free_ids()
    assert want["counts"].tolist()[:4] == [len(ack_src), sum(v in M.ANSWERED for v in verdict), len(opened), len(closed)]
    # what the header promises about the state
    assert sorted(list(after.table.values()) + after.free_ids()) == list(range(entry.nflows))  # every id is live or free, once
    for r, g in enumerate(want["opened"]):
        i = int(want["opened_src"][r])
        assert after.flow_start[g] == M.header(ring, stride, i)[1] and after.seq0[g] == 0
        assert (after.slot_len[g * entry.window:(g + 1) * entry.window] == M.EMPTY).all()
    same = np.setdiff1d(np.arange(entry.nflows), want["opened"])
    assert np.array_equal(after.seq0[same], entry.seq0[same]) and np.array_equal(after.flow_start[same], entry.flow_start[same])
    w = entry.window
    assert all(np.array_equal(after.slot_len[f * w:(f + 1) * w], entry.slot_len[f * w:(f + 1) * w]) for f in same)


@pytest.mark.parametrize("bucket", ["library", "low bits"])
def test_model_against_the_restatement(bucket):
    bucket_of = lib_bucket() if bucket == "library" else low_bits
    seen = set()
    for r in M.fuzz_rounds(bucket_of):
        compare(r["entry"], r["ring"], r["stride"], r["keys"], r["ok"], r["flow"], r["max_acks"], r["want"], bucket_of)
        seen |= set(r["want"]["verdict"].tolist())
    for case in M.directed_cases(bucket_of):
        got = M.run_case(case, bucket_of, call=lambda *a: compare(*a, bucket_of))
        for want in got:
            seen |= set(want["verdict"].tolist())
    assert seen == set(range(10)), [M.VERDICTS[v] for v in set(range(10)) - seen]


def test_corpus_is_exact_and_reaches_every_verdict():
    """With the library's hash no fuzz round overflows a bucket; the corpus reaches every verdict
    but REFUSED_BUCKET, which needs a full bucket and comes from the directed cases, every batch
    of which is one the header determines."""
    bucket_of = lib_bucket()
    rounds = M.fuzz_rounds(bucket_of)
    assert len(rounds) == M.FUZZ_ROUNDS and max(r["n"] for r in rounds) > 150 and min(r["n"] for r in rounds) == 0
    assert not any(r["want"]["overflow"] for r in rounds) and all(r["want"]["exact"] for r in rounds)
    seen = np.bincount(np.concatenate([r["want"]["verdict"] for r in rounds]), minlength=10)
    assert (np.delete(seen, M.REFUSED_BUCKET) >= 5).all() and seen[M.REFUSED_BUCKET] == 0, dict(zip(M.VERDICTS, seen))
    assert any(0 < r["want"]["counts"][0] < r["want"]["counts"][1] for r in rounds)  # an ACK ring that is cut
    assert sum(len(set(r["keys"])) < len(r["keys"]) for r in rounds) > 20  # one key several times in a batch
    assert len({bucket_of(k, M.FUZZ_BUCKETS) for k in M.fuzz_keys()}) == M.FUZZ_BUCKETS
    # every id is reused
    opens = np.bincount(np.concatenate([r["want"]["opened"] for r in rounds]).astype(np.int64), minlength=M.FUZZ_FLOWS)
    assert (opens >= 2).all()
    directed = [w for case in M.directed_cases(bucket_of) for w in M.run_case(case, bucket_of)]
    assert all(w["exact"] for w in directed) and any(w["overflow"] for w in directed)
    assert sum(int(w["counts"][5]) for w in directed) >= 3


def by_name(bucket_of, name):
    case = next(c for c in M.directed_cases(bucket_of) if c[0] == name)
    return M.run_case(case, bucket_of)


def test_directed_verdicts():
    b = lib_bucket()
    assert tuple(c[0] for c in M.directed_cases(b)) == M.CASE_NAMES
    assert by_name(b, "duplicates, equal seqNums")[0]["verdict"].tolist() == [M.OPENED, M.START_DUP, M.START_DUP]
    assert by_name(b, "duplicates, differing seqNums")[0]["verdict"].tolist() == [M.OPENED, M.START_OTHER, M.START_DUP]
    full = by_name(b, "free ids run out")
    assert full[0]["verdict"].tolist() == [M.OPENED] * 3 + [M.REFUSED_FULL] * 2 and full[0]["opened"].tolist() == [0, 1, 2]
    assert len(full[0]["state"].table) == 3 and full[0]["counts"].tolist() == [3, 3, 3, 0, 2, 0]
    assert full[1]["verdict"].tolist() == [M.CLOSED] and full[2]["verdict"].tolist() == [M.OPENED, M.REFUSED_FULL]
    assert full[2]["opened"].tolist() == [0]  # the id that the close gave back
    assert by_name(b, "refused followers")[0]["verdict"].tolist() == [M.OPENED] + [M.REFUSED_FULL] * 3
    one = by_name(b, "bucket full, one bucket")
    assert one[0]["counts"].tolist() == [16, 16, 16, 0, 0, 0] and one[1]["counts"].tolist() == [0, 0, 0, 0, 0, 2]
    assert one[1]["overflow"] and one[1]["state"].table == one[0]["state"].table
    assert one[3]["verdict"].tolist() == [M.OPENED, M.START_DUP] and one[3]["opened"].tolist() == [16]
    four = by_name(b, "bucket full, four buckets")
    assert four[1]["verdict"].tolist() == [M.REFUSED_BUCKET, M.OPENED] and four[3]["verdict"].tolist() == [M.OPENED]
    busy = by_name(b, "busy")
    assert busy[1]["verdict"].tolist() == [M.END_BUSY, M.END_OTHER]
    assert busy[2]["verdict"].tolist() == [M.CLOSED, M.END_STALE, M.END_STALE]
    cut = by_name(b, "acks cut")
    assert cut[1]["counts"].tolist()[:4] == [2, 4, 0, 2] and len(cut[1]["state"].table) == 2
    assert by_name(b, "no flows")[0]["verdict"].tolist() == [M.REFUSED_FULL, M.END_STALE, M.NONE]


def test_ring_wrap():
    """The head at nflows - 1 (the ring holds ids 0, 1, 2, 3 from cell 3 on): three opens pop
    cells 3, 0, 1; two closes push behind the four ids the ring held, at cells 3 and 0 again;
    the next opens take id 3 and then the two ids that came back, in the order of their closes."""
    got = by_name(lib_bucket(), "ring wrap")
    assert M.State(4, 1, 2, 3).free_ids() == [0, 1, 2, 3] and M.State(4, 1, 2, 3).free_pos.tolist() == [3, 4]
    assert got[0]["opened"].tolist() == [0, 1, 2] and got[0]["state"].free_pos.tolist() == [2, 1]
    assert got[1]["closed"].tolist() == [0, 1] and got[1]["state"].free_pos.tolist() == [2, 3]
    assert got[1]["state"].free_ids() == [3, 0, 1]
    assert got[2]["opened"].tolist() == [3, 0, 1] and got[2]["state"].free_pos.tolist() == [1, 0]
    assert sorted(got[2]["state"].table.values()) == [0, 1, 2, 3]


@pytest.mark.parametrize("seed", [1, 2])
def test_lifecycles_over_the_models(seed):
    """The lifecycle driver on the models of all six calls: eight transfers over four flows end
    with every file equal to its source, every id reused, STARTs refused while all ids were
    taken, and the stale DATA of closed connections never placed."""
    life = M.run_life(seed, M.ModelReceiver(lib_bucket()))
    assert 8 <= life.step <= M.LIFE_MAX_STEPS
    verdicts = np.bincount(np.concatenate([np.array(h[4]) for h in life.log]), minlength=10)
    assert all(verdicts[v] > 0 for v in (M.OPENED, M.START_DUP, M.REFUSED_FULL, M.CLOSED, M.END_STALE))
