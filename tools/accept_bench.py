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
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "a3-reliable-transport_amd"))
import wtp_crc32 as W  # noqa: E402

STRIDE, MAXP, SEQ0, GOAL = 1472, 1456, 1, 1.10


def timed(fn, before=None):
    if before:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    a = np.sort(np.asarray(xs))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4),
            "p25": round(float(np.percentile(a, 25)), 4), "p75": round(float(np.percentile(a, 75)), 4)}


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
    t = {"verify": [], "copy": [], "accept": []}
    for rep in range(warmup + reps):
        tv, tc, ta = timed(verify), timed(copy), timed(accept, before=reset)
        if rep >= warmup:
            t["verify"].append(tv)
            t["copy"].append(tc)
            t["accept"].append(ta)
    base = np.asarray(t["verify"]) + np.asarray(t["copy"])
    v, c, a = (float(np.median(t[k])) for k in ("verify", "copy", "accept"))
    payload = float(total)
    return {"n": n, "order": order, "stride": STRIDE, "window": n, "exact": exact, "kernel": kernel,
            "verify_ms": round(v, 4), "copy_ms": round(c, 4), "accept_ms": round(a, 4),
            "ratio": round(a / (v + c), 4),
            "baseline_ms": stats(base), "accept_ms_stats": stats(t["accept"]),
            "baseline_spread": round(float((np.percentile(base, 75) - np.percentile(base, 25)) / np.median(base)), 4),
            "accept_payload_gbps": round(payload / (a * 1e-3) / 1e9, 1),
            "place_ms_estimate": round(a - v, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1048576,65536")
    ap.add_argument("--orders", default="inorder,permuted")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accept", "accept_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("accept_bench: needs a GPU (no CPU fallback)")
    if a.reps < 20:
        raise SystemExit("accept_bench: --reps must be at least 20")
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    cases = [case(int(n), order, a.reps, a.warmup) for n in a.sizes.split(",") for order in a.orders.split(",")]
    head = next((c for c in cases if c["n"] == 1 << 20 and c["order"] == "inorder"), None)
    res = {"tool": "accept_bench", "device": torch.cuda.get_device_name(0), "library": W.LIB.wtp_version().decode(),
           "lib_path": os.path.relpath(W.LIB_PATH, ROOT), "reps": a.reps, "warmup": a.warmup, "goal_ratio": GOAL,
           "headline_ratio": head["ratio"] if head else None,
           "goal_met": bool(head["ratio"] <= GOAL) if head else None, "cases": cases}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
