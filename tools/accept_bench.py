#!/usr/bin/env python3
"""Device-side receive (wtp_accept_data_packets) against what a caller could do before it
existed, in one process, alternating per repetition, timed with device events:

  (a) baseline, valid for the loss-free in-order case only: wtp_crc32_verify_batch, then a
      strided device copy of the payload columns,
      out.view(n, 1456).copy_(ring.view(n, 1472)[:, 16:])
  (b) the new call (verify + claim + place + ack); its window reset (slot_len <- EMPTY)
      runs before the timed window.

Sizes: the workload's 1 M x 1472-B ring with a 1 M-slot window (3 GB moved, nothing stays
cache-resident) and 64 K datagrams (config C2).  Orders: in-order, and a seeded random
permutation of the ring slots (for which (a) would not reassemble the file; its times are
still the same traffic).  Every timed configuration is checked first: the file image,
place[] and the ACK must be exact.

Prints one JSON line and writes it to profiles/accept/accept_bench.json (--out).
Goal (in-order, 1 M): accept_ms / (verify_ms + copy_ms) <= 1.10.
  python tools/accept_bench.py [--reps 25] [--warmup 3] [--sizes 1048576,65536]
                               [--orders inorder,permuted] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import wtp_crc32 as W
from bench_support import stats

STRIDE, MAXP, SEQ0, GOAL = 1472, 1456, 1, 1.10


def case(n, order, reps, warmup):
    total = n * MAXP
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=0xACCE)
    ring = torch.empty(n * STRIDE, dtype=torch.uint8, device="cuda")
    rl = torch.empty(n, dtype=torch.int32, device="cuda")
    W.build_data_packets(src, total, SEQ0, ring, STRIDE, rl)
    want_place = torch.arange(n, dtype=torch.int32, device="cuda")
    if order == "permuted":
        perm = torch.from_numpy(np.random.default_rng(0xACCE).permutation(n)).cuda()
        ring = ring.view(n, STRIDE)[perm].contiguous().view(-1)
        want_place = perm.to(torch.int32)
    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    slot_len = torch.empty(n, dtype=torch.int32, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    place = torch.empty(n, dtype=torch.int32, device="cuda")
    ack = torch.zeros(1, dtype=torch.int32, device="cuda")

    def reset():
        slot_len.fill_(-1)

    def verify():
        W.verify_batch(ring, STRIDE, rl, n, ok)

    def copy():
        out.view(n, MAXP).copy_(ring.view(n, STRIDE)[:, 16:])

    def accept():
        W.accept_data_packets(ring, STRIDE, rl, n, SEQ0, n, out, slot_len, ok, place, ack)

    # exactness of what is timed, on this very input
    out.zero_()
    reset()
    accept()
    torch.cuda.synchronize()
    kernel = W.LIB.wtp_last_kernel().decode()
    exact = bool(torch.equal(out, src) and torch.equal(place, want_place) and bool(ok.all())
                 and int(ack.item()) & 0xFFFFFFFF == SEQ0 + n and bool((slot_len == MAXP).all()))
    if order == "inorder":
        out.zero_()
        verify()
        copy()
        torch.cuda.synchronize()
        exact = exact and bool(torch.equal(out, src) and bool(ok.all()))
    if not exact:
        raise SystemExit(f"accept_bench: n={n} {order}: outputs are not exact")
    t = B.sample({"verify": (verify, None, 1), "copy": (copy, None, 1), "accept": (accept, reset, 1)}, reps, warmup)
    base = np.asarray(t["verify"]) + np.asarray(t["copy"])
    v, c, a = (float(np.median(t[k])) for k in ("verify", "copy", "accept"))
    payload = float(total)
    return {"n": n, "order": order, "stride": STRIDE, "window": n, "exact": exact, "kernel": kernel,
            "verify_ms": round(v, 4), "copy_ms": round(c, 4), "accept_ms": round(a, 4),
            "ratio": round(a / (v + c), 4),
            "baseline_ms": stats(base), "accept_ms_stats": stats(t["accept"]), "baseline_spread": B.spread(base),
            "accept_payload_gbps": round(payload / (a * 1e-3) / 1e9, 1),
            "place_ms_estimate": round(a - v, 4)}


def main():
    ap = B.parser()
    ap.add_argument("--sizes", default="1048576,65536")
    ap.add_argument("--orders", default="inorder,permuted")
    B.add_out(ap, "accept")
    a = ap.parse_args()
    res = B.start("accept_bench", a, min_reps=20)
    cases = [case(int(n), order, a.reps, a.warmup) for n in a.sizes.split(",") for order in a.orders.split(",")]
    head = next((c for c in cases if c["n"] == 1 << 20 and c["order"] == "inorder"), None)
    res.update({"goal_ratio": GOAL, "headline_ratio": head["ratio"] if head else None,
                "goal_met": bool(head["ratio"] <= GOAL) if head else None, "cases": cases})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
