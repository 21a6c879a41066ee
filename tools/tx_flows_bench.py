#!/usr/bin/env python3
"""The multi-connection sender (wtp_tx_ingest_acks_flows + wtp_tx_advance_flows +
wtp_tx_build_retransmit_var_flows) against the single-connection calls, in one process,
interleaved and in both orders, timed with device events, once from captured graphs and once
back to back:

  state    64 Ki sender slots over 64 Ki full-size records (1456 B).  For nflows F the window is
           64 Ki / F, flow f owns records [f * window, (f + 1) * window) and its sequence numbers
           continue flow f - 1's, so record r carries SEQ0 + r whatever F is and every emitted
           datagram can be compared with row r of one reference ring.
  acks     4096 selective (or cumulative) ACKs, ACK j for flow j % F: the leading 4096 / F slots of
           every flow (F <= 4096; one slot of the first 4096 flows above), so every window slides.
  due      "all": every un-ACKed slot (WTP_RETX_ALL), a ring of 64 Ki datagrams, 96 MB of wire;
           "1pct": timers, one slot in a hundred older than the timeout.
  flows    one ingest_flows + one advance_flows + one build_flows.
  (a)      wtp_tx_ingest_acks + wtp_tx_advance + wtp_tx_build_retransmit_var on the same slots as
           ONE connection of 64 Ki slots (the ACKs name the same global slots).  Timed twice per
           repetition, as `a` and `a2`: a2 / a is the A/A spread of the run, the margin the
           nflows == 1 row is read against.
  (b)      F separate triples, one per connection, for F <= 1024: the cost the feature removes.
           The host knows every connection's advance here (the state is restored before each
           unit), so (b) is not charged the host read it needs in a real loop.

A timed unit is `inner` x (restore acked, sent_ms and the bases; ingest; advance; build); the
restore is in every variant alike.  The variants of a repetition run in turn, in rising order
on even repetitions and falling order on odd ones.  Every configuration is first checked on
the device: per-flow advances and 0 -> 1 counts, the slid state and bases, the counts, the
selection and every emitted datagram against the reference ring.

Prints one JSON line and writes it to profiles/tx_flows/tx_flows_bench.json (--out).
  python tools/tx_flows_bench.py [--reps 25] [--warmup 3] [--inner 10] [--flows 1,64,1024,16384] [--out PATH]"""
import sys

import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import wtp_crc32 as W
from bench_support import i32, stats, u32, z

S, STRIDE, MAXP, SEQ0, NACK = 1 << 16, 1472, 1456, 0xFFFF8000, 4096  # the numbering wraps 2^32
NOW, TIMEOUT = 100000, 500
MODES = (("selective", W.ACK_SELECTIVE), ("cumulative", W.ACK_CUMULATIVE))
SPLIT_MAX_FLOWS = 1024


def ack_ring(seqs):
    """16-byte ACKs htonl{3, seq, 0, 0} on the device."""
    h = np.zeros((len(seqs), 4), dtype=">u4")
    h[:, 0], h[:, 1] = 3, np.asarray(seqs, dtype=np.uint32)
    return torch.from_numpy(h.view(np.uint8).reshape(-1)).cuda()


class State:
    """One variant's own window state and outputs (so that no variant warms another's)."""

    def __init__(self, nflows, sent0):
        self.acked0, self.sent0 = z(S), i32(sent0)
        self.acked, self.sent = [z(S), z(S)], [z(S), z(S)]
        self.ok, self.wire = z(NACK, torch.uint8), torch.empty((S, STRIDE), dtype=torch.uint8, device="cuda")
        self.sel, self.wl, self.counts = z(S), z(S), z(2)
        self.adv, self.fresh = z(max(nflows, 2)), z(max(nflows, 2))

    def restore(self):
        self.acked[0].copy_(self.acked0)
        self.sent[0].copy_(self.sent0)


def case(nflows, mode_name, mode, due, table, ref, reps, warmup, inner):
    base, offs, lens = table
    window = S // nflows
    cum = mode == W.ACK_CUMULATIVE
    flags = W.RETX_ALL if due == "all" else 0
    g = np.arange(S)
    sent0 = np.where((g % 100 == 37) | (due == "all"), NOW - TIMEOUT - 1, NOW).astype(np.uint32)
    # ACK j: flow j % F, slot j / F (cumulative: a = slot + 1), as far as the flow has slots
    j = np.arange(NACK)
    a_flow, a_slot = j % nflows, j // nflows
    a_glob = a_flow * window + a_slot
    adv_h = np.minimum(np.bincount(a_flow, minlength=nflows), window).astype(np.uint32)  # every flow's leading run
    seq0_h = ((SEQ0 + np.arange(nflows, dtype=np.int64) * window) & 0xFFFFFFFF).astype(np.uint32)
    rec0_h = (np.arange(nflows) * window).astype(np.uint32)
    ring_f = ack_ring((seq0_h[a_flow].astype(np.int64) + a_slot + cum) & 0xFFFFFFFF)
    ring_a = ack_ring((SEQ0 + a_glob + cum) & 0xFFFFFFFF)
    flow, rl = i32(a_flow), i32(np.full(NACK, 16))
    rec_end = i32(rec0_h + window)
    fl, a1, a2 = State(nflows, sent0), State(1, sent0), State(1, sent0)
    seq0, rec0 = i32(seq0_h), i32(rec0_h)
    bases = [[z(nflows), z(nflows)], [z(nflows), z(nflows)]]  # seq, rec: [current, next]
    work = torch.empty(W.tx_work_bytes(S, S), dtype=torch.uint8, device="cuda")
    fill = NOW  # the entries shifted in are not due by their timers

    def flows_once():
        fl.restore()
        bases[0][0].copy_(seq0)
        bases[1][0].copy_(rec0)
        W.tx_ingest_acks_flows(ring_f, 16, rl, flow, NACK, mode, bases[0][0], bases[1][0], rec_end, nflows, window, fl.acked[0],
                               fl.ok, None, fl.adv, fl.fresh)
        W.tx_advance_flows(fl.acked[0], fl.sent[0], nflows, window, fl.adv, fill, bases[0][0], bases[1][0], fl.acked[1],
                           fl.sent[1], bases[0][1], bases[1][1])
        W.tx_build_retransmit_var_flows(base, S * MAXP, offs, lens, S, bases[0][1], bases[1][1], rec_end, nflows, window,
                                        fl.acked[1], fl.sent[1], NOW, TIMEOUT, flags, fl.wire, STRIDE, S, fl.sel, fl.wl, None,
                                        fl.counts, work=work)

    # One connection of S slots.  Its host moves the base itself, here by the advance this state always
    # has: the leading run of flow 0 (selective), the largest a (cumulative; for F > 1 that is nearly the
    # whole window, so the cumulative rows of (a) build far less than the flows do and only F == 1 compares).
    a = int(a_glob.max()) + 1 if cum else int(adv_h[0])

    def single_once(st):
        st.restore()
        W.tx_ingest_acks(ring_a, 16, rl, NACK, mode, SEQ0, S, st.acked[0], st.ok, None, st.adv)
        W.tx_advance(st.acked[0], st.sent[0], S, st.adv, fill, st.acked[1], st.sent[1])
        W.tx_build_retransmit_var(base, S * MAXP, offs[a:], lens[a:], SEQ0 + a, S - a, st.acked[1], st.sent[1], NOW, TIMEOUT,
                                  flags, st.wire, STRIDE, S, st.sel, st.wl, None, st.counts, work=work)

    variants = {"flows": flows_once, "a": lambda: single_once(a1), "a2": lambda: single_once(a2)}
    split = nflows <= SPLIT_MAX_FLOWS
    if split:
        sp = State(nflows, sent0)
        rings_b = [ack_ring((int(seq0_h[f]) + a_slot[a_flow == f] + cum) & 0xFFFFFFFF) for f in range(nflows)]
        work_b = torch.empty(W.tx_work_bytes(window, window), dtype=torch.uint8, device="cuda")
        cnt_b = z(2 * nflows)

        def split_once():
            sp.restore()
            for f in range(nflows):
                lo, hi, a, nf = f * window, (f + 1) * window, int(adv_h[f]), int((a_flow == f).sum())
                W.tx_ingest_acks(rings_b[f], 16, rl, nf, mode, int(seq0_h[f]), window, sp.acked[0][lo:hi], sp.ok, None,
                                 cnt_b[2 * f:2 * f + 2])
                W.tx_advance(sp.acked[0][lo:hi], sp.sent[0][lo:hi], window, cnt_b[2 * f:2 * f + 2], fill, sp.acked[1][lo:hi],
                             sp.sent[1][lo:hi])
                W.tx_build_retransmit_var(base, S * MAXP, offs[lo + a:], lens[lo + a:], int(seq0_h[f]) + a, window - a,
                                          sp.acked[1][lo:hi], sp.sent[1][lo:hi], NOW, TIMEOUT, flags, sp.wire[lo:hi], STRIDE,
                                          window, sp.sel[lo:hi], sp.wl[lo:hi], None, sp.counts, work=work_b)

        variants["b"] = split_once

    # ---- exactness, on the device --------------------------------------------------------------
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    s_in = g % window
    a_of = np.repeat(adv_h, window)
    keep = s_in + a_of < window
    want_sent = np.where(keep, sent0[np.minimum(g + a_of, S - 1)], fill).astype(np.uint32)
    is_due = keep & ((want_sent != NOW) | (due == "all"))  # nothing ACKed is left in a window: the runs went
    want_sel = np.flatnonzero(is_due)
    want_sent[want_sel] = NOW
    e = int(u32(fl.counts)[0])
    rec_of_sel = torch.from_numpy((want_sel + a_of[want_sel]).astype(np.int64)).cuda()
    exact = bool(np.array_equal(u32(fl.adv)[:nflows], adv_h) and np.array_equal(u32(fl.fresh)[:nflows], adv_h)
                 and not bool(fl.acked[1].any()) and np.array_equal(u32(fl.sent[1]), want_sent)
                 and np.array_equal(u32(bases[0][1]), (seq0_h + adv_h) & 0xFFFFFFFF) and np.array_equal(u32(bases[1][1]), rec0_h + adv_h)
                 and tuple(u32(fl.counts)) == (want_sel.size, want_sel.size) and np.array_equal(u32(fl.sel)[:e], want_sel)
                 and bool((fl.wl[:e] == STRIDE).all()) and torch.equal(fl.wire[:e], ref[rec_of_sel]) and bool(fl.ok.all()))
    if split:
        exact = exact and torch.equal(sp.acked[1], fl.acked[1]) and torch.equal(sp.sent[1], fl.sent[1])
        exact = exact and np.array_equal(u32(cnt_b).reshape(nflows, 2), np.stack([adv_h, adv_h], axis=1))
    if nflows == 1:
        exact = exact and torch.equal(a1.sent[1], fl.sent[1]) and torch.equal(a1.wire[:e], fl.wire[:e]) and \
            torch.equal(a1.sel[:e], fl.sel[:e]) and tuple(u32(a1.counts)) == tuple(u32(fl.counts))
    if not exact:
        raise SystemExit(f"tx_flows_bench: nflows {nflows} {mode_name} {due}: outputs are not exact")

    # ---- timing ------------------------------------------------------------------------------------
    row = {"nflows": nflows, "window": window, "mode": mode_name, "due": due, "emitted": e, "exact": exact, "slots": S, "acks": NACK}
    # a unit of the split baseline is already nflows triples
    calls = {name: (fn, max(1, inner // nflows) if name == "b" else inner) for name, fn in variants.items()}
    for how in ("graph", "back_to_back"):
        t = B.sample(B.repeated(calls, how), reps, warmup, alternate=True)
        med = {name: float(np.median(v)) for name, v in t.items()}
        res = {"unit_ms": {name: stats(v) for name, v in t.items()},
               "flows_over_a": round(med["flows"] / med["a"], 4),
               "a2_over_a": round(med["a2"] / med["a"], 4),
               "flows_over_a_paired": stats(np.divide(t["flows"], t["a"])),
               "a2_over_a_paired": stats(np.divide(t["a2"], t["a"]))}
        if split:
            res["b_over_flows"] = round(med["b"] / med["flows"], 2)
        row[how] = res
    return row


def main():
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--flows", default="1,64,1024,16384")
    ap.add_argument("--modes", default="selective,cumulative")
    ap.add_argument("--due", default="all,1pct")
    B.add_out(ap, "tx_flows")
    a = ap.parse_args()
    res = B.start("tx_flows_bench", a, min_reps=10)
    base = torch.empty(S * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(base, seed=0x7F10)
    ref = torch.empty((S, STRIDE), dtype=torch.uint8, device="cuda")
    W.build_data_packets(base, S * MAXP, SEQ0, ref, STRIDE, None)
    offs = torch.arange(S, dtype=torch.int64, device="cuda") * MAXP
    lens = torch.full((S,), MAXP, dtype=torch.int32, device="cuda")
    rows = []
    for f in a.flows.split(","):
        for name, mode in MODES:
            for due in a.due.split(","):
                if name in a.modes.split(","):
                    rows.append(case(int(f), name, mode, due, (base, offs, lens), ref, a.reps, a.warmup, a.inner))
                    print(f"tx_flows_bench: nflows {f} {name} {due} done", file=sys.stderr, flush=True)
    res.update({"inner": a.inner,
                "unit": "restore the state; ingest; advance; build over all 64 Ki slots (b: nflows triples); ms per unit",
                "cases": rows})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
