"""CPU tests of the loop-free paths of tests/txflows_model.py and of tests/flows_cases.py, the
inputs of the GPU edge tests of the multi-connection calls: the fast paths equal the per-flow
paths (the definition) on the whole fuzz corpus and on a scaled-down copy of every new case,
and the model halves of the cases are what their GPU tests rely on: every length and every
source phase occurs, the counts lie on both sides of every round-size change, flow_fresh
differs from the raw hit count, the due sets hold the named slots."""
import numpy as np
import pytest

import flows_cases as C
import flows_flush_model as FF
import flows_model as F
import txflows_model as T

MODES = (T.SELECTIVE, T.CUMULATIVE)
MAXP, STRIDE, M32 = T.MAXP, T.STRIDE, T.M32


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x == y if isinstance(x, tuple) else (x is None and y is None) or np.array_equal(x, y)


def both_builds(c, now, timeout, flags, max_sel, stride=STRIDE, optional=True):
    """The rebuild of a case's state on both paths; returns the result after asserting them equal."""
    prior = [np.full(max(max_sel, 1) * stride, 0xA5, np.uint8)] + [np.full(max_sel, 9, np.uint32) if optional else None] * 3
    args = (c["base"], c["base"].size, c["offs"], c["lens"], c["lens"].size, c["seq0"], c["rec0"], c["rec_end"], c["nflows"],
            c["window"], c["acked"], c["sent"], now, timeout, flags, prior[0], stride, max_sel, *prior[1:])
    want = T.retransmit_var_flows(*args)
    same(T.retransmit_var_flows(*args, fast=True), want)
    return want


# ---- the fast paths on the fuzz corpus -------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fast_paths_equal_the_per_flow_paths_on_the_corpus(mode):
    for seed in T.FUZZ_SEEDS:
        calls, case = T.fuzz_calls(seed, mode)
        nf, w = case["nflows"], case["window"]
        for c in calls:
            got = T.ingest_flows(c["ring"], case["stride"], c["rl"], c["flow"], mode, c["seq0"], c["rec0"], case["rec_end"], nf, w,
                                 c["acked0"], fast=True)
            same(got, c["ingest"])
            junk = np.full(nf * w, 0x77777777, np.uint32)
            got = T.advance_flows(c["ingest"][2], c["sent0"], nf, w, c["ingest"][3], c["fill"], c["seq0"], c["rec0"], junk, junk,
                                  junk[:nf], junk[:nf], fast=True)
            same(got, c["advance"])
            ak, sm, sq, rc = c["advance"]
            ms = c["max_sel"]
            for optional in (True, False):
                prior = [np.full(ms * case["wire_stride"], 0xA5, np.uint8)] + \
                    [np.full(ms, v, np.uint32) if optional else None for v in (0x5E1, 0x1E4, 0xC4C)]
                args = (case["base"], case["base_bytes"], case["offs"], case["lens"], case["nrec"], sq, rc, case["rec_end"], nf, w,
                        ak, sm, c["now"], T.FUZZ_TIMEOUT, c["flags"], prior[0], case["wire_stride"], ms, *prior[1:])
                got = T.retransmit_var_flows(*args, fast=True)
                same(got, c["build"] if optional else T.retransmit_var_flows(*args))


def test_fast_paths_on_degenerate_shapes():
    z, one = np.zeros(0, np.uint32), np.zeros(1, np.uint32)
    ack = np.frombuffer(T.R.ack_datagram(0), np.uint8)
    for args in ((np.zeros(0, np.uint8), 16, z, z, 0, z, z, z, 0, 5, z), (ack, 16, [16], [0], 0, one, one, one + 3, 1, 0, z),
                 (ack, 16, [16], [7], 1, z, z, z, 0, 9, z), (ack[:0], 16, z, z, 1, one, one, one + 3, 1, 4, [1, 1, 0, 1])):
        same(T.ingest_flows(*args, fast=True), T.ingest_flows(*args))
    args = (np.zeros(1, np.uint8), 1, z, z, 0, one, one, one, 1, 0, z, z, 5, 1, 1, np.zeros(STRIDE, np.uint8), STRIDE, 4)
    same(T.retransmit_var_flows(*args, fast=True), T.retransmit_var_flows(*args))
    args = (np.zeros(1, np.uint8), 1, z, z, 0, one, one, one + 2, 1, 2, [0, 0], [0, 0], 5, 1, 1, np.zeros(4 * STRIDE, np.uint8), STRIDE, 4)
    got = T.retransmit_var_flows(*args, fast=True)  # two due slots and no record table
    same(got, T.retransmit_var_flows(*args))
    assert got[5] == (2, 2)


# ---- 1a ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", C.PATTERNS)
def test_every_length_case(pattern):
    c = C.every_length_case(pattern)
    assert sorted(c["lens"].tolist()) == list(range(MAXP + 1)) and (c["nflows"], c["window"]) == (5, 300)
    for base_off in (0, 1):  # packed: every source phase, whatever the 16-B aligned allocation's address
        assert set(((base_off + c["offs"][c["lens"] > 0]) % 16).astype(int).tolist()) == set(range(16))
    mixed = np.abs(np.diff(c["lens"].astype(np.int64)))
    assert (mixed > 64).mean() > 0.8  # short and long records side by side in a wave's round
    infl = T.inflight_all(c["rec0"], c["rec_end"], 5, 300)
    assert infl.tolist() == [300] * 4 + [257] and int(c["seq0"][2]) + 299 > M32
    behind = ~C.inflight_mask(c["rec0"], c["rec_end"], 5, 300)
    assert behind.sum() == 43 and (c["acked"][behind] == 0).all() and (c["sent"][behind] == C.OLD).all()  # they look due
    d = c["d"]
    assert {"none": d == 0, "one": d == 1, "tenth": 100 < d < 200, "half": 600 < d < 860, "all": d == 1457}[pattern]
    assert len(c["rings"]) == (3 if d == 0 else 4) and (d == 0 or {d, d - 1, d + 70, 1500} == set(c["rings"]))
    small = C.every_length_case(pattern, top=99)  # the scaled-down copy, on both paths
    for max_sel in small["rings"]:
        want = both_builds(small, C.NOW, C.TIMEOUT, 0, max_sel)
        assert want[5] == (min(small["d"], max_sel), small["d"])
        if max_sel == small["d"] - 1:
            again = dict(small, sent=want[4])
            got = both_builds(again, C.NOW, C.TIMEOUT, 0, max(small["d"] - 1, 1), stride=1473)
            assert got[5] == (1, 1) and got[1][0] == np.flatnonzero(small["due"])[-1]


# ---- 1b ------------------------------------------------------------------------------------------
def test_round_sizes_change_at_the_thresholds():
    assert C.THRESHOLDS == [5120, 10_240, 20_480, 40_960, 81_920, 163_840] and C.TWO_ROUNDS == 327_680
    for j, t in enumerate(C.THRESHOLDS):
        for count, g in ((t, j), (t + 1, j + 1)):
            window = -(-(count + 9) // 3)
            S = 3 * (window + (window % 64 == 0))
            assert C.round_log2(count, count + 9, S) == g
            assert j > 2 or C.round_log2(count, count, S) == g
    assert C.round_log2(5200, 5200, 5200) == 1 and C.round_log2(4098, 4098, 4107) == 0  # what the suite had: g <= 1
    c = C.many_short_records()
    assert c["n"] == 400_000 > C.TWO_ROUNDS and C.round_log2(c["n"], c["S"], c["S"]) == 6 and c["window"] % 64
    assert T.inflight_all(c["rec0"], c["rec_end"], 3, c["window"]).sum() == c["n"] and c["S"] == c["n"] + 2


@pytest.mark.parametrize("count,rec_len", [(70, 4), (71, MAXP), (200, 4)])
def test_count_case_scaled_down(count, rec_len):
    c = C.count_case(count, rec_len)
    for max_sel in (count + 9, count):
        want = both_builds(c, C.NOW, C.TIMEOUT, 0, max_sel)
        assert want[5] == (count, count) and np.array_equal(want[1][:count], c["due"])
    owners = np.bincount(c["due"] // c["window"], minlength=3)
    assert owners.max() - owners.min() <= 2  # spread evenly over the three windows


# ---- 1c ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nflows,window", C.SCALE_SHAPES)
def test_scale_case_due_sets(nflows, window):
    c = C.scale_case(nflows, window)
    S = nflows * window
    assert S in (C.MAX_SLOTS, 64 * C.SELECT_BLOCK + 1) and 1000 <= c["d"] <= 2000  # 1024 block counts, and 65
    assert c["due"][[g for g in C.NAMED_SLOTS if g < S]].all()
    first, last = c["due"][::window], c["due"][window - 1::window]
    assert first.sum() >= min(4, nflows) and last.sum() >= min(3, nflows)
    infl = T.inflight_all(c["rec0"], c["rec_end"], nflows, window)
    assert window == 1 or (0 < (infl < window).sum() < nflows or nflows == 1)
    # the selection itself, on the fast path alone: the per-flow path is held to it on the small shapes below
    prior = np.full((c["d"] + 50) * STRIDE, 0xA5, np.uint8)
    args = (c["base"], c["base"].size, c["offs"], c["lens"], S, c["seq0"], c["rec0"], c["rec_end"], nflows, window, c["acked"])
    full = T.retransmit_var_flows(*args, c["sent"], C.NOW, C.TIMEOUT, 0, prior, STRIDE, c["d"] + 50, np.zeros(c["d"] + 50, np.uint32),
                                  fast=True)
    assert full[5] == (c["d"], c["d"]) and np.array_equal(full[1][:c["d"]], np.flatnonzero(c["due"]))
    cut = C.cut_inside_a_flow(full[1], c["d"], window)
    part = T.retransmit_var_flows(*args, c["sent"], C.NOW, C.TIMEOUT, 0, prior, STRIDE, cut, np.zeros(cut, np.uint32), fast=True)
    assert part[5] == (cut, c["d"]) and np.array_equal(part[1], full[1][:cut])


@pytest.mark.parametrize("nflows,window", [(4, 700), (200, 6), (1, 1100), (1100, 1)])
def test_scale_case_scaled_down(nflows, window):
    c = C.scale_case(nflows, window, extra=60)
    full = both_builds(c, C.NOW, C.TIMEOUT, 0, c["d"] + 50)
    assert full[5] == (c["d"], c["d"])
    cut = C.cut_inside_a_flow(full[1], c["d"], window)
    part = both_builds(c, C.NOW, C.TIMEOUT, 0, cut)
    assert part[5] == (cut, c["d"]) and np.array_equal(part[1][:cut], full[1][:cut])


# ---- 1d ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("now,timeout", C.TIMER_CASES)
def test_timer_case(now, timeout):
    c = C.timer_case(now, timeout)
    w = c["window"]
    for flags, want_sel in ((0, c["due"]), (T.RETX_ALL, c["all"])):
        got = both_builds(c, now, timeout, flags, c["S"])
        assert np.array_equal(got[1][:got[5][0]], want_sel) and got[5] == (want_sel.size, want_sel.size)
    sides = [(np.isin(np.arange(f * w, (f + 1) * w), c["due"]).any(), np.isin(np.arange(f * w, (f + 1) * w), c["all"]).sum()
              > np.isin(np.arange(f * w, (f + 1) * w), c["due"]).sum()) for f in range(3)]
    assert all(not_due for _, not_due in sides) and (timeout == M32 or all(due for due, _ in sides))
    if now < 1000 and timeout == 500:  # the clock has wrapped since the sends
        assert (c["sent"] > 0xF0000000).any()
    future = ((c["sent"].astype(np.int64) - now) & M32) == 3
    assert future.sum() >= 9 and (timeout >= M32 - 2 or np.isin(np.flatnonzero(future & (c["acked"] == 0))[:5], c["due"]).all())


# ---- 2a ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_ack_batch(mode):
    c = C.ack_batch(mode)
    assert 70_000 <= c["n"] <= 73_000 and c["n"] > 256 * 250  # hundreds of workgroups
    args = (c["ring"], 16, c["rl"], c["flow"], mode, c["seq0"], c["rec0"], c["rec_end"], c["nflows"], c["window"], c["acked0"])
    got = T.ingest_flows(*args, fast=True)
    C.check_ack_batch(c, got)
    assert c["n"] / (c["nflows"] * c["window"]) > 2  # every slot is ACKed about twice on average
    small = C.ack_batch(mode, nflows=30, window=20, general=1200, hot=900)
    args = (small["ring"], 16, small["rl"], small["flow"], mode, small["seq0"], small["rec0"], small["rec_end"], 30, 20, small["acked0"])
    want = T.ingest_flows(*args)
    same(T.ingest_flows(*args, fast=True), want)
    C.check_ack_batch(small, want)


# ---- 2b ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", C.SLIDE_WINDOWS)
def test_slide_case(window):
    c = C.slide_case(window)
    junk, junk_f = np.full(c["S"], 0x77777777, np.uint32), np.full(7, 0x77777777, np.uint32)
    args = (c["acked"], c["sent"], 7, window, c["adv"], c["fill"], c["seq0"], c["rec0"], junk, junk, junk_f, junk_f)
    want = T.advance_flows(*args)
    same(T.advance_flows(*args, fast=True), want)
    C.check_slide(c, want)


def test_slide_case_at_the_slot_limit():
    c = C.slide_case(1024, nflows=1024)
    assert c["S"] == C.MAX_SLOTS
    junk, junk_f = np.full(c["S"], 0x77777777, np.uint32), np.full(1024, 0x77777777, np.uint32)
    C.check_slide(c, T.advance_flows(c["acked"], c["sent"], 1024, 1024, c["adv"], c["fill"], c["seq0"], c["rec0"], junk, junk, junk_f,
                                     junk_f, fast=True))


# ---- 3 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1488, 1504, 1500])
def test_accept_case(stride):
    ring, rl, flow, seq0, order = C.accept_case(stride)
    assert sorted(order.tolist()) == list(range(1485)) and np.array_equal(rl, order + 16)
    out, sl = np.full(1500 * MAXP, 0xA5, np.uint8), np.full(1500, F.EMPTY, np.uint32)
    ok, place, out, sl, ack = F.accept_flows(ring, stride, rl, flow, seq0, 3, 500, out, sl)
    fits = order + 16 <= stride  # a datagram longer than its ring slot is not intact
    assert np.array_equal(ok != 0, fits) and (stride == 1488) == (not fits.all()) and fits[order <= MAXP].all()
    assert np.array_equal(place, np.where(order <= MAXP, order // 3, F.NOT_PLACED))
    assert np.array_equal(ack, ((seq0.astype(np.int64) + [486, 486, 485]) & M32).astype(np.uint32))
    img = out.reshape(1500, MAXP)
    for ln in (0, 1, 7, 15, 16, 17, 23, 1447, 1455):
        g = (ln % 3) * 500 + ln // 3
        assert sl[g] == ln and (img[g, ln:] == 0xA5).all()  # bytes [len, 1456) stay


def test_flush_state():
    img, sl, runs = C.flush_state(1)
    nf, w = C.FLUSH_FLOWS, C.FLUSH_WINDOW
    plan = FF.deliver_flows_plan(sl, nf, w, w, 1 << 40, 0)
    assert plan[3].tolist() == list(C.FLUSH_RUNS) and sorted(plan[2].tolist()) == list(range(MAXP + 1))
    assert int(plan[5][2]) == MAXP * (MAXP + 1) // 2
    behind = np.concatenate([sl[f * w + r:(f + 1) * w] for f, r in enumerate(runs)])
    assert behind.size == 43 and (behind == F.EMPTY).sum() == 40 and set(behind.tolist()) == {F.EMPTY, MAXP + 1, C.CLAIM, 0xFFFFFFFE}
    at = 2 * w + runs[2] // 2  # the full-size record in the middle flow
    assert sl[at] == MAXP
    before = int(sl[:w][:runs[0]].sum() + sl[w:2 * w][:runs[1]].sum() + sl[2 * w:at].sum())
    cut = FF.deliver_flows_plan(sl, nf, w, w, before + 700, 0)
    assert cut[3].tolist() == [300, 290, runs[2] // 2, 0, 0] and int(cut[5][2]) == before
