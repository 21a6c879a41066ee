#!/usr/bin/env python3
"""Multi-connection receive (wtp_accept_data_packets_flows + wtp_rx_build_acks_flows) against
the single-connection calls, in one process, interleaved and in both orders, timed with device
events, once from captured graphs and once back to back:

  batch    64 Ki full DATA datagrams in 1472-byte slots (the device builder's wire image).  For
           nflows F the window is 64 Ki / F and arrival j belongs to flow j % F, slot j / F: the
           connections arrive interleaved and every window fills up.
  flows    one accept_flows + one acks_flows over the whole batch, per ACK mode.
  (a)      wtp_accept_data_packets + wtp_rx_build_acks on the same ring as ONE connection with a
           window of 64 Ki (the same global slots, so the image and slot_len are identical).  It
           is timed twice per repetition, as `a` and `a2`: a2 / a is the A/A spread of the run,
           the margin the nflows == 1 row is held against.
  (b)      F separate accept + build_acks call pairs, one per connection, on batches already
           split by connection, for F <= 1024: the cost the feature removes.

A timed unit is `inner` x (clear d_slot_len; accept; acks), so every accept places its whole
batch; the clear is in every variant alike.  The variants of a repetition run in turn, in
rising order on even repetitions and falling order on odd ones.  Every configuration is first
checked on the device: flows' image, slot_len, d_ok and selective ACK ring are those of (a),
d_place is the slot within the flow, the per-flow ACKs are seq0[f] + window.

Prints one JSON line and writes it to profiles/flows/flows_bench.json (--out).
  python tools/flows_bench.py [--reps 25] [--warmup 3] [--inner 50] [--flows 1,64,1024,16384] [--out PATH]"""
import sys

import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import wtp_crc32 as W
from bench_support import stats, u32, z

N, STRIDE, MAXP, SEQ0 = 1 << 16, 1472, 1456, 0xFFFF8000  # the one-connection window wraps 2^32
MODES = (("selective", W.ACK_SELECTIVE), ("cumulative", W.ACK_CUMULATIVE))
SPLIT_MAX_FLOWS = 1024


class State:
    """One variant's own window state and outputs (so that no variant warms another's)."""

    def __init__(self, nflows):
        self.img, self.sl = torch.empty(N * MAXP, dtype=torch.uint8, device="cuda"), z(N)
        self.ok, self.place, self.ack = z(N, torch.uint8), z(N), z(max(nflows, 1))
        self.wire, self.src, self.counts = z(N * 16, torch.uint8), z(N), z(2)

    def clear(self):
        self.sl.fill_(-1)


def case(nflows, mode_name, mode, ordered, reps, warmup, inner):
    """`ordered`: the builder's ring and lengths, datagram i = SEQ0 + i."""
    ring0, rl = ordered
    window = N // nflows
    j = np.arange(N)
    perm = (j % nflows) * window + j // nflows  # arrival j is datagram perm[j]: flow j % F, slot j / F
    ring = ring0[torch.from_numpy(perm).cuda()].contiguous()
    flow = torch.from_numpy((j % nflows).astype(np.int32)).cuda()
    seq0_h = ((SEQ0 + np.arange(nflows, dtype=np.int64) * window) & 0xFFFFFFFF).astype(np.uint32)
    seq0 = torch.from_numpy(seq0_h.view(np.int32)).cuda()
    fl, a1, a2 = State(nflows), State(1), State(1)
    work_f = torch.empty(W.rx_ack_flows_work_bytes(N), dtype=torch.uint8, device="cuda")
    work_a = torch.empty(W.rx_ack_work_bytes(N, N, mode), dtype=torch.uint8, device="cuda")

    def flows_once():
        fl.clear()
        W.accept_data_packets_flows(ring, STRIDE, rl, flow, N, seq0, nflows, window, fl.img, fl.sl, fl.ok, fl.place, fl.ack)
        W.rx_build_acks_flows(ring, STRIDE, rl, flow, N, mode, seq0, nflows, window, fl.ok, fl.ack, fl.wire, 16, 0, N, fl.src,
                              fl.counts, work=work_f)

    def single_once(st):
        st.clear()
        W.accept_data_packets(ring, STRIDE, rl, N, SEQ0, N, st.img, st.sl, st.ok, st.place, st.ack)
        W.rx_build_acks(ring, STRIDE, rl, N, mode, SEQ0, N, st.ok, st.place, st.sl, st.wire, 16, 0, N, st.src, st.counts,
                        work=work_a)

    variants = {"flows": flows_once, "a": lambda: single_once(a1), "a2": lambda: single_once(a2)}
    split = nflows <= SPLIT_MAX_FLOWS
    if split:
        sp = State(nflows)
        work_b = torch.empty(W.rx_ack_work_bytes(window, window, mode), dtype=torch.uint8, device="cuda")

        def split_once():
            sp.clear()
            for f in range(nflows):
                lo, hi = f * window, (f + 1) * window
                W.accept_data_packets(ring0[lo:hi], STRIDE, rl[lo:hi], window, int(seq0_h[f]), window, sp.img[lo * MAXP:],
                                      sp.sl[lo:hi], sp.ok[lo:hi], sp.place[lo:hi], sp.ack[f:f + 1])
                W.rx_build_acks(ring0[lo:hi], STRIDE, rl[lo:hi], window, mode, int(seq0_h[f]), window, sp.ok[lo:hi],
                                sp.place[lo:hi], sp.sl[lo:hi], sp.wire[lo * 16:], 16, 0, window, sp.src[lo:hi], sp.counts,
                                work=work_b)

        variants["b"] = split_once

    # ---- exactness, on the device --------------------------------------------------------------
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    want_ack = ((seq0_h.astype(np.int64) + window) & 0xFFFFFFFF).astype(np.uint32)
    exact = bool(torch.equal(fl.img, a1.img) and torch.equal(fl.sl, a1.sl) and torch.equal(fl.ok, a1.ok) and bool(fl.ok.all())
                 and np.array_equal(u32(fl.place), (j // nflows).astype(np.uint32)) and np.array_equal(u32(a1.place), perm)
                 and np.array_equal(u32(fl.ack), want_ack) and tuple(u32(fl.counts)) == (N, N) == tuple(u32(a1.counts))
                 and torch.equal(fl.src, a1.src))
    if mode == W.ACK_SELECTIVE:
        exact = exact and torch.equal(fl.wire, a1.wire)
    else:  # every ACK of flow f names seq0[f] + window
        seqs = np.ascontiguousarray(fl.wire.view(N, 16)[:, 4:8].cpu().numpy()).view(">u4").reshape(-1)
        exact = exact and np.array_equal(seqs, want_ack[j % nflows])
    if split:
        exact = exact and torch.equal(sp.img, a1.img) and torch.equal(sp.sl, a1.sl) and np.array_equal(u32(sp.ack), want_ack)
    if not exact:
        raise SystemExit(f"flows_bench: nflows {nflows} {mode_name}: outputs are not exact")

    # ---- timing ------------------------------------------------------------------------------------
    row = {"nflows": nflows, "window": window, "mode": mode_name, "exact": exact, "n": N}
    # a unit of the split baseline is already nflows call pairs
    calls = {name: (fn, max(1, inner // nflows) if name == "b" else inner) for name, fn in variants.items()}
    for how in ("graph", "back_to_back"):
        t = B.sample(B.repeated(calls, how), reps, warmup, alternate=True)
        med = {name: float(np.median(v)) for name, v in t.items()}
        res = {"unit_ms": {name: stats(v) for name, v in t.items()},
               "flows_over_a": round(med["flows"] / med["a"], 4),
               "a2_over_a": round(med["a2"] / med["a"], 4),
               "flows_over_a_paired": stats(np.divide(t["flows"], t["a"])),
               "a2_over_a_paired": stats(np.divide(t["a2"], t["a"])),
               "datagrams_per_us_flows": round(N / (med["flows"] * 1e3), 1)}
        if split:
            res["b_over_flows"] = round(med["b"] / med["flows"], 2)
        row[how] = res
    return row


def main():
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--flows", default="1,64,1024,16384")
    ap.add_argument("--modes", default="selective,cumulative")
    B.add_out(ap, "flows")
    a = ap.parse_args()
    res = B.start("flows_bench", a, min_reps=10)
    pay = torch.empty(N * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(pay, seed=0xF10)
    ring0 = torch.empty((N, STRIDE), dtype=torch.uint8, device="cuda")
    rl = torch.empty(N, dtype=torch.int32, device="cuda")
    W.build_data_packets(pay, N * MAXP, SEQ0, ring0, STRIDE, rl)
    del pay
    rows = []
    for f in a.flows.split(","):
        for name, mode in MODES:
            if name in a.modes.split(","):
                rows.append(case(int(f), name, mode, (ring0, rl), a.reps, a.warmup, a.inner))
                print(f"flows_bench: nflows {f} {name} done", file=sys.stderr, flush=True)
    res.update({"inner": a.inner, "unit": "clear d_slot_len; accept; acks over the whole batch (b: nflows call pairs); ms per unit",
                "cases": rows})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
