#!/usr/bin/env python3
"""Multi-connection flush and slide (wtp_rx_deliver_flows + wtp_rx_advance_flows) against the
single-connection calls, in one process, interleaved and in both orders, timed with device
events, once from captured graphs and once back to back:

  state    64 Ki DATA datagrams (full size, or Zipf(1.1) lengths) built on the device and placed
           by one wtp_accept_data_packets_flows: for nflows F the window is 64 Ki / F and arrival
           j belongs to flow j % F, so every window is full.
  unit     deliver with max_slots = window / 2, then advance by what was delivered: half of
           every window goes to the stream and the other half slides down (an advance by the whole
           window would move nothing).
  (a)      one deliver_flows + one advance_flows over the whole state, bases included.
  (b)      F pairs of wtp_rx_deliver + wtp_rx_advance on the sub-windows, each deliver at the
           stream offset the flows before it end at: the only route before these calls.  Run once
           for the exactness check at every F, timed for F <= 1024.
  (c)      the single-flow pair on the same 64 Ki slots as ONE connection (window 64 Ki,
           max_slots 32 Ki: the same bytes).  It is timed twice per repetition, as `c` and `c2`:
           c2 / c is the A/A spread of the run, which a / c at F == 1 is recorded next to.

The variants of a repetition run in turn, in rising order on even repetitions and falling order
on odd ones.  Every configuration is first checked on the device: (a)'s stream, record arrays,
next image and next slot_len are (b)'s, its d_flow_adv is window / 2 for every flow, its bases
moved by that, and at F == 1 everything equals (c) too.

Prints one JSON line and writes it to profiles/flows_flush/flows_flush_bench.json (--out).
  python tools/flows_flush_bench.py [--reps 25] [--warmup 3] [--inner 20] [--flows 1,64,1024,16384]
                                    [--lengths full,zipf] [--out PATH]"""
import sys

import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the oracle's directories on sys.path
import oracle as O
import wtp_crc32 as W
from bench_support import stats, z

N, STRIDE, MAXP, SEQ0 = 1 << 16, 1472, 1456, 0xFFFF8000
SPLIT_MAX_FLOWS = 1024


class Out:
    """One variant's own outputs (so that no variant warms another's): the stream, the record
    arrays, the counts and the second window state."""

    def __init__(self, nflows, stream_bytes):
        self.stream = z(stream_bytes + 64, torch.uint8, 0xA5)
        self.offs, self.lens = z(N, torch.int64, 77), z(N, fill=77)
        self.counts, self.adv, self.info = z(4, torch.int64), z(nflows, torch.int64), z(4 * nflows, torch.int64)
        self.img, self.sl, self.seq0 = z(N * MAXP, torch.uint8, 0xEE), z(N, fill=12345), z(nflows)

    def same(self, other):
        return bool(torch.equal(self.stream, other.stream) and torch.equal(self.offs, other.offs)
                    and torch.equal(self.lens, other.lens) and torch.equal(self.img, other.img) and torch.equal(self.sl, other.sl))


def case(nflows, kind, lens_h, wire, reps, warmup, inner):
    """`wire`: (ring, recv_len) of datagram i = SEQ0 + i with payload length lens_h[i]."""
    ring0, rl0 = wire
    window = N // nflows
    half = window // 2
    j = np.arange(N)
    perm = (j % nflows) * window + j // nflows  # arrival j is datagram perm[j]: flow j % F, slot j / F
    pick = torch.from_numpy(perm).cuda()
    ring, rl = ring0[pick].contiguous(), rl0[pick].contiguous()
    flow = torch.from_numpy((j % nflows).astype(np.int32)).cuda()
    seq0_h = ((SEQ0 + np.arange(nflows, dtype=np.int64) * window) & 0xFFFFFFFF).astype(np.uint32)
    seq0 = torch.from_numpy(seq0_h.view(np.int32)).cuda()
    img, sl = torch.empty(N * MAXP, dtype=torch.uint8, device="cuda"), z(N, fill=-1)
    ok = z(N, torch.uint8)
    W.accept_data_packets_flows(ring, STRIDE, rl, flow, N, seq0, nflows, window, img, sl, ok, None, None)
    torch.cuda.synchronize()
    del ring, rl
    if not (bool(ok.all()) and np.array_equal(sl.cpu().numpy().view(np.uint32), lens_h)):
        raise SystemExit(f"flows_flush_bench: nflows {nflows} {kind}: the state is not the batch")
    # what the first half of every window holds, and where each flow's bytes start in the stream
    per_flow = lens_h.reshape(nflows, window)[:, :half].astype(np.int64).sum(axis=1)
    at = np.concatenate([[0], np.cumsum(per_flow)])
    total = int(at[-1])
    cap = total + 16
    cap_c = int(lens_h[:N // 2].astype(np.int64).sum()) + 16  # one connection's first half: the same bytes at F == 1
    a, b, c, c2 = Out(nflows, cap), Out(nflows, cap), Out(1, cap_c), Out(1, cap_c)
    work_a = torch.empty(W.rx_deliver_flows_work_bytes(nflows, window), dtype=torch.uint8, device="cuda")
    work_b = torch.empty(W.rx_deliver_work_bytes(window), dtype=torch.uint8, device="cuda")
    work_c = torch.empty(W.rx_deliver_work_bytes(N), dtype=torch.uint8, device="cuda")

    def a_once():
        W.rx_deliver_flows(img, sl, nflows, window, half, a.stream, cap, 0, a.offs, a.lens, a.adv, a.info, a.counts, work=work_a)
        W.rx_advance_flows(img, sl, nflows, window, a.adv, seq0, a.img, a.sl, a.seq0)

    def b_once():
        for f in range(nflows):
            lo, hi = f * window, (f + 1) * window
            W.rx_deliver(img[lo * MAXP:], sl[lo:hi], window, half, b.stream, cap, int(at[f]), b.offs[f * half:], b.lens[f * half:],
                         b.counts, work=work_b)
            W.rx_advance(img[lo * MAXP:], sl[lo:hi], window, b.counts, b.img[lo * MAXP:], b.sl[lo:hi])

    def c_once(o):
        W.rx_deliver(img, sl, N, N // 2, o.stream, cap_c, 0, o.offs, o.lens, o.counts, work=work_c)
        W.rx_advance(img, sl, N, o.counts, o.img, o.sl)

    # ---- exactness, on the device --------------------------------------------------------------
    a_once()
    b_once()
    torch.cuda.synchronize()
    exact = a.same(b) and a.adv.cpu().tolist() == [half] * nflows
    exact = exact and a.counts.cpu().tolist() == [half * nflows, N, total, int(lens_h.astype(np.int64).sum())]
    exact = exact and np.array_equal(a.seq0.cpu().numpy().view(np.uint32), ((seq0_h.astype(np.int64) + half) & 0xFFFFFFFF))
    exact = exact and a.info.view(nflows, 4).cpu().numpy().tolist() == [[window, f * half, int(at[f]), int(per_flow[f])]
                                                                        for f in range(nflows)]
    exact = exact and bool((a.stream[total:] == 0xA5).all())
    variants = {"a": a_once, "c": lambda: c_once(c), "c2": lambda: c_once(c2)}
    if nflows == 1:
        c_once(c)
        torch.cuda.synchronize()
        exact = exact and a.same(c) and torch.equal(a.counts, c.counts)
    if not exact:
        raise SystemExit(f"flows_flush_bench: nflows {nflows} {kind}: outputs are not exact")
    split = nflows <= SPLIT_MAX_FLOWS
    if split:
        variants["b"] = b_once

    # ---- timing ------------------------------------------------------------------------------------
    row = {"nflows": nflows, "window": window, "lengths": kind, "exact": exact, "slots": N, "delivered_bytes": total}
    # a unit of the split baseline is already nflows call pairs
    calls = {name: (fn, max(1, inner // nflows) if name == "b" else inner) for name, fn in variants.items()}
    for how in ("graph", "back_to_back"):
        t = B.sample(B.repeated(calls, how), reps, warmup, alternate=True)
        med = {name: float(np.median(v)) for name, v in t.items()}
        res = {"unit_ms": {name: stats(v) for name, v in t.items()},
               "a_over_c": round(med["a"] / med["c"], 4),
               "c2_over_c": round(med["c2"] / med["c"], 4),
               "a_over_c_paired": stats(np.divide(t["a"], t["c"])),
               "c2_over_c_paired": stats(np.divide(t["c2"], t["c"]))}
        if split:
            res["b_over_a"] = round(med["b"] / med["a"], 2)
            res["a_below_b_by_more_than_both_iqr"] = B.below_by_more_than_both_iqr(t["a"], t["b"])
        row[how] = res
    return row


def main():
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--flows", default="1,64,1024,16384")
    ap.add_argument("--lengths", default="full,zipf")
    B.add_out(ap, "flows_flush")
    a = ap.parse_args()
    res = B.start("flows_flush_bench", a, min_reps=10)
    rows = []
    for kind in a.lengths.split(","):
        lens_h = np.full(N, MAXP, np.uint32) if kind == "full" else O.zipf_lengths(N, seed=0xF1A).astype(np.uint32)
        offs_h = np.concatenate([[0], np.cumsum(lens_h[:-1], dtype=np.uint64)]).astype(np.uint64)
        nbytes = int(lens_h.astype(np.int64).sum())
        pay = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        W.synth_fill(pay, seed=0xF10)
        ring0 = torch.empty((N, STRIDE), dtype=torch.uint8, device="cuda")
        rl0 = torch.empty(N, dtype=torch.int32, device="cuda")
        W.build_data_packets_var(pay, nbytes, torch.from_numpy(offs_h.view(np.int64)).cuda(),
                                 torch.from_numpy(lens_h.view(np.int32)).cuda(), N, SEQ0, ring0, STRIDE, rl0)
        torch.cuda.synchronize()
        del pay
        for f in a.flows.split(","):
            rows.append(case(int(f), kind, lens_h, (ring0, rl0), a.reps, a.warmup, a.inner))
            print(f"flows_flush_bench: nflows {f} {kind} done", file=sys.stderr, flush=True)
    res.update({"inner": a.inner,
                "unit": "deliver (max_slots = window / 2) + advance over the whole state (b: nflows call pairs); ms per unit",
                "cases": rows})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
