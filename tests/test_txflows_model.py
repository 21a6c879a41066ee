"""CPU tests of tests/txflows_model.py, the models of wtp_tx_ingest_acks_flows,
wtp_tx_advance_flows and wtp_tx_build_retransmit_var_flows: the conditions on the fuzz corpus
that keep the GPU fuzz from passing vacuously, the single-flow identities, the flow-major cut,
and the whole transfer on the models alone, whose round count is the bound the device loop is
held to."""
import numpy as np
import pytest

import advance_model as V
import flows_model as F
import oracle as O
import retx_model as R
import retxvar_model as RV
import txflows_model as T

MODES = (T.SELECTIVE, T.CUMULATIVE)
M32 = T.M32


@pytest.fixture(scope="module")
def corpus():
    return {(seed, mode): T.fuzz_calls(seed, mode) for seed in T.FUZZ_SEEDS for mode in MODES}


def test_corpus_shapes(corpus):
    """12 seeds, 2 .. 5 flows, windows of 3 .. 90 slots, two rounds per state; odd seeds put
    flow 0 within 3 of the wrap, seeds divisible by 3 give two flows one seq0; every seed has a
    flow with fewer records than slots, and over the corpus every role of T.ROLES occurs."""
    roles = set()
    assert len(T.FUZZ_SEEDS) == 12
    for (seed, _), (calls, case) in corpus.items():
        assert 2 <= case["nflows"] <= 5 and 3 <= case["window"] <= 90 and len(calls) == T.FUZZ_CALLS == 2
        seq0, rec0, rec_end, w = case["seq0"], case["rec0"], case["rec_end"], case["window"]
        assert seed % 2 == 0 or (1 << 32) - int(seq0[0]) <= 3
        assert seed % 3 or seq0[0] == seq0[1]
        infl = [T.inflight_of(rec0, rec_end, f, w) for f in range(case["nflows"])]
        assert any(0 < i < w for i in infl) and infl[0] == w
        for f, role in enumerate(case["roles"]):
            roles.add(role)
            assert {"full": infl[f] == w, "short": 0 < infl[f] < w, "empty": rec0[f] == rec_end[f],
                    "past": rec0[f] > rec_end[f]}[role]
            assert role in ("full", "short") or infl[f] == 0
    assert roles == {"full", *T.ROLES}


def test_every_ack_kind_in_every_call_with_its_verdict(corpus):
    """Every kind of T.ACK_KINDS is dealt in every batch, and stands for what its name says."""
    for (seed, mode), (calls, case) in corpus.items():
        for c in calls:
            ok, hit = c["ingest"][0], c["ingest"][1]
            assert set(c["kinds"]) == set(T.ACK_KINDS), (seed, set(T.ACK_KINDS) - set(c["kinds"]))
            for i, kind in enumerate(c["kinds"]):
                f, placed = int(c["flow"][i]), hit[i] != T.NOT_PLACED
                inf = c["infl"][f] if f < case["nflows"] else None
                if kind in ("corrupt", "runt", "long"):
                    assert not ok[i] and not placed
                elif kind in ("noflow_n", "noflow_m"):
                    assert f >= case["nflows"] and not placed
                elif kind == "nonack":
                    assert ok[i] and not placed
                elif kind == "payload":
                    assert ok[i] and c["rl"][i] > 16 and (placed == (inf > (2 if mode == T.SELECTIVE else 0)))
                elif kind == "a0":
                    assert ok[i] and placed == (mode == T.SELECTIVE and inf > 0)
                elif kind == "a_in":
                    assert ok[i] and placed == (mode == T.CUMULATIVE and inf > 0) and (not placed or hit[i] == inf)
                elif kind == "a_in1":
                    assert ok[i] and not placed
            assert any(k == "noflow_n" and ok[i] for i, k in enumerate(c["kinds"]))
            assert len(c["kinds"]) > len(set(zip(c["flow"].tolist(), c["ring"].reshape(-1, case["stride"])[:, 4:8].view(">u4")
                                                 .reshape(-1).tolist())))  # duplicates


def test_every_record_kind_is_emitted_in_each_round_of_the_corpus(corpus):
    """Over the seeds, each of the two rounds emits every kind of T.REC_KINDS, valid ones with
    a datagram and invalid ones (1457 bytes, an offset past base_bytes, an index at or above
    nrec) with wire_len 0; each round also leaves a flow with an advance and one without."""
    for mode in MODES:
        for c_i in range(T.FUZZ_CALLS):
            seen, moved = set(), set()
            for seed in T.FUZZ_SEEDS:
                calls, case = corpus[(seed, mode)]
                c, w = calls[c_i], case["window"]
                _, sel, wl, crc, _, (emitted, due) = c["build"]
                rec0 = c["advance"][3]
                for k in range(emitted):
                    f, s = divmod(int(sel[k]), w)
                    r = int(rec0[f]) + s
                    kind = case["rec_kind"][r]
                    seen.add(kind)
                    invalid = kind in ("len1457", "off_past", "past_nrec")
                    assert (wl[k] == 0 and crc[k] == 0) if invalid else wl[k] == 16 + int(case["lens"][r])
                    if kind == "last_byte":
                        assert int(case["offs"][r]) + int(case["lens"][r]) == case["base_bytes"]
                moved |= {a > 0 for a in c["ingest"][3].tolist()}
                assert emitted == min(due, c["max_sel"])
            assert seen == set(T.REC_KINDS), (mode, c_i, set(T.REC_KINDS) - seen)
            assert moved == {True, False}
    # the second round's ring is shorter than the due set somewhere, and the cut falls inside a flow
    cuts = [(c["build"][5], case["window"], c["build"][1]) for (calls, case) in corpus.values() for c in calls[1:]]
    assert any(e < d and int(sel[e - 1]) % w != w - 1 for (e, d), w, sel in cuts)


def test_reinterleaving_changes_nothing_but_the_order(corpus):
    for (seed, mode), (calls, case) in corpus.items():
        rng = np.random.default_rng(seed)
        c = calls[0]
        perm = F.reinterleave(rng, c["flow"])
        got = T.ingest_flows(F.rows(c["ring"], case["stride"], perm), case["stride"], c["rl"][perm], c["flow"][perm], mode,
                             c["seq0"], c["rec0"], case["rec_end"], case["nflows"], case["window"], c["acked0"])
        ok, hit, acked, adv, fresh = c["ingest"]
        assert np.array_equal(got[0], ok[perm]) and np.array_equal(got[1], hit[perm])
        assert all(np.array_equal(g, x) for g, x in zip(got[2:], (acked, adv, fresh)))


@pytest.mark.parametrize("mode", MODES)
def test_one_flow_is_the_single_window_models(mode):
    """nflows == 1: the three models equal retx_model.ingest, advance_model.tx_advance and
    retxvar_model.retransmit_var on the same inputs."""
    for seed in T.FUZZ_SEEDS:
        calls, case = T.fuzz_calls(seed, mode)
        c, w, stride = calls[0], case["window"], case["stride"]
        mine = c["flow"] == 0
        ring, rl = F.rows(c["ring"], stride, np.flatnonzero(mine)), c["rl"][mine]
        seq0, rec0, rec_end = c["seq0"][:1], c["rec0"][:1], np.array([int(c["rec0"][0]) + w - 1], np.uint32)  # inflight w - 1
        acked, sent = c["acked0"][:w], c["sent0"][:w]
        ok, hit, ak, adv, fresh = T.ingest_flows(ring, stride, rl, np.zeros(rl.size, np.uint32), mode, seq0, rec0, rec_end, 1, w,
                                                 acked)
        one = R.ingest(ring, stride, rl, mode, int(seq0[0]), w - 1, acked[:w - 1])
        assert np.array_equal(ok, one[0]) and np.array_equal(hit, one[1]) and np.array_equal(ak[:w - 1], one[2])
        assert (int(adv[0]), int(fresh[0])) == one[3] and ak[w - 1] == acked[w - 1]
        junk = np.full(w, 0x77, np.uint32)
        ak2, sm2, sq, rc = T.advance_flows(ak, sent, 1, w, adv, c["fill"], seq0, rec0, junk, junk, junk[:1], junk[:1])
        a1, s1 = V.tx_advance(ak, sent, w, int(adv[0]), c["fill"], junk, junk)
        assert np.array_equal(ak2, a1) and np.array_equal(sm2, s1)
        assert (int(sq[0]), int(rc[0])) == ((int(seq0[0]) + int(adv[0])) & M32, int(rec0[0]) + int(adv[0]))
        inf = T.inflight_of(rc, rec_end, 0, w)
        for max_sel in (w, 2, 0):
            prior = (np.full(max(max_sel, 1) * T.STRIDE, 0xA5, np.uint8), *(np.full(max_sel, 9, np.uint32) for _ in range(3)))
            got = T.retransmit_var_flows(case["base"], case["base_bytes"], case["offs"], case["lens"], case["nrec"], sq, rc,
                                         rec_end, 1, w, ak2, sm2, c["now"], T.FUZZ_TIMEOUT, c["flags"], prior[0], T.STRIDE,
                                         max_sel, *prior[1:])
            r0 = int(rc[0])
            want = RV.retransmit_var(case["base"], case["base_bytes"], case["offs"][r0:], case["lens"][r0:], int(sq[0]), inf,
                                     ak2[:inf], sm2[:inf], c["now"], T.FUZZ_TIMEOUT, c["flags"], prior[0], T.STRIDE, max_sel,
                                     *prior[1:])
            for g, x in zip(got[:4], want[:4]):
                assert np.array_equal(g, x)
            assert np.array_equal(got[4][:inf], want[4]) and np.array_equal(got[4][inf:], sm2[inf:]) and got[5] == want[5]


def test_the_cut_is_flow_major_and_a_second_call_takes_up_where_it_stopped(corpus):
    calls, case = corpus[(2, T.SELECTIVE)]
    c, nf, w = calls[0], case["nflows"], case["window"]
    ak, sm, sq, rc = c["advance"]
    args = (case["base"], case["base_bytes"], case["offs"], case["lens"], case["nrec"], sq, rc, case["rec_end"], nf, w, ak)
    S = nf * w
    wire = np.full(S * T.STRIDE, 0xA5, np.uint8)
    full = T.retransmit_var_flows(*args, sm, c["now"], T.FUZZ_TIMEOUT, 0, wire, T.STRIDE, S, np.zeros(S, np.uint32))
    e = full[5][0]
    assert e == full[5][1] > 4 and np.array_equal(full[1][:e], np.sort(full[1][:e]))
    cut = e // 2
    a = T.retransmit_var_flows(*args, sm, c["now"], T.FUZZ_TIMEOUT, 0, wire, T.STRIDE, cut, np.zeros(S, np.uint32))
    b = T.retransmit_var_flows(*args, a[4], c["now"], T.FUZZ_TIMEOUT, 0, wire, T.STRIDE, S, np.zeros(S, np.uint32))
    assert a[5] == (cut, e) and b[5] == (e - cut, e - cut)  # emitted slots are no longer due
    assert np.array_equal(np.concatenate([a[1][:cut], b[1][:e - cut]]), full[1][:e])
    assert np.array_equal(a[0][:cut * T.STRIDE], full[0][:cut * T.STRIDE]) and np.array_equal(b[4], full[4])
    # with WTP_RETX_ALL every call starts at flow 0 again: a short ring starves the late flows
    x = T.retransmit_var_flows(*args, sm, c["now"], T.FUZZ_TIMEOUT, T.RETX_ALL, wire, T.STRIDE, 3, np.zeros(S, np.uint32))
    y = T.retransmit_var_flows(*args, x[4], c["now"], T.FUZZ_TIMEOUT, T.RETX_ALL, wire, T.STRIDE, 3, np.zeros(S, np.uint32))
    assert np.array_equal(x[1][:3], y[1][:3]) and x[5] == y[5]


def test_degenerate_shapes_of_the_models():
    z = np.zeros(0, np.uint32)
    one = np.zeros(1, np.uint32)
    assert [a.size for a in T.ingest_flows(np.zeros(0, np.uint8), 16, z, z, 0, z, z, z, 0, 5, z)] == [0] * 5
    ok, hit, ak, adv, fresh = T.ingest_flows(np.frombuffer(R.ack_datagram(0), np.uint8), 16, [16], [0], 0, one, one, one + 3, 1, 0, z)
    assert ok.tolist() == [1] and hit.tolist() == [T.NOT_PLACED] and adv.tolist() == fresh.tolist() == [0]
    assert T.retransmit_var_flows(np.zeros(1, np.uint8), 1, z, z, 0, one, one, one, 1, 0, z, z, 5, 1, 1, np.zeros(T.STRIDE, np.uint8),
                                  T.STRIDE, 4)[5] == (0, 0)


@pytest.fixture(scope="module")
def transfers():
    out = {}
    for mode in MODES:
        end = T.ModelEnd()
        out[mode] = (end,) + T.transfer(end, mode)
    return out


@pytest.mark.parametrize("mode", MODES)
def test_transfer_on_the_models(transfers, mode):
    """It finishes within the cap in both ACK modes, every flow sees a loss, a duplicate and an
    out-of-order arrival, and the four delivered streams, offsets and lengths are the sources."""
    end, log, stats = transfers[mode]
    assert len(log) <= F.XFER_MAX_ROUNDS and (stats >= 1).all(), (len(log), stats)
    for f in range(F.XFER_FLOWS):
        lens, offs, total, host = end.rec[f]
        assert np.array_equal(end.stream[f], host)
        assert np.array_equal(np.array(end.offs_got[f], np.uint64), offs) and np.array_equal(np.array(end.lens_got[f], np.uint32), lens)
        assert O.crc32(end.stream[f]) == O.crc32(host)
    assert end.trec[0].tolist() == end.rec_end.tolist()  # every window has passed its last record, on the bases alone


@pytest.mark.parametrize("mode", MODES)
def test_transfer_rounds_are_the_per_connection_loops(transfers, mode):
    """Seven calls per round decide what 3 * F + 2 + 2 * F calls per round decide: the batched
    loop's selections, ACKs, flushes and advances are flows_model.transfer's, round for round.
    Its round count is the bound tests/test_gpu_txflows.py holds the device loop to."""
    _, log, stats = transfers[mode]
    want, want_stats = F.transfer(F.ModelEnd(), mode)
    assert len(log) == len(want) and np.array_equal(stats, want_stats)
    for got_r, want_r in zip(log, want):
        assert got_r[0] == want_r[0] and got_r[2:] == want_r[2:]  # the ring positions differ: one packed ring here
        assert len(got_r[1]) == len(want_r[1])
