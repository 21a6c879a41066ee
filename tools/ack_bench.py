#!/usr/bin/env python3
"""Device-side ACK generation (wtp_rx_build_acks) against the call it follows, in one
process, the two in turn per repetition, timed with device events:

  accept   wtp_accept_data_packets on a batch of n full DATA datagrams in 1472-byte slots (the
           device builder's wire image, in order or in a seeded random order) into an empty
           window of n slots; d_slot_len is cleared before the timed window.  The yardstick:
           its code is what it was before this call existed.
  acks     wtp_rx_build_acks on the same batch, accept's verdicts and the window after it,
           into a ring of max_acks = n 16-byte entries, selective and cumulative mode.

Every timed configuration is checked first against the model (tests/ack_model.py, its
vectorised path): counts, d_src and every ACK byte.  Goal: accept + acks <=
1.10 x accept at 1 M datagrams in order, both modes; at 64 K the ratio is only reported.

Prints one JSON line and writes it to profiles/ack/ack_bench.json (--out).
  python tools/ack_bench.py [--reps 25] [--warmup 3] [--sizes 1048576,65536] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the model's directories on sys.path
import ack_model as A
import wtp_crc32 as W
from bench_support import stats, u32

STRIDE, MAXP, SEQ0 = 1472, 1456, 0xFFF80000
MODES = (("selective", W.ACK_SELECTIVE), ("cumulative", W.ACK_CUMULATIVE))


def case(n, permuted, reps, warmup):
    pay = torch.empty(n * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(pay, seed=0xACE)
    ring = torch.empty((n, STRIDE), dtype=torch.uint8, device="cuda")
    rl = torch.empty(n, dtype=torch.int32, device="cuda")
    W.build_data_packets(pay, n * MAXP, SEQ0, ring, STRIDE, rl)
    if permuted:
        ring = ring[torch.from_numpy(np.random.default_rng(n).permutation(n)).cuda()].contiguous()
    del pay
    img = torch.empty(n * MAXP, dtype=torch.uint8, device="cuda")
    sl = torch.empty(n, dtype=torch.int32, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    place = torch.empty(n, dtype=torch.int32, device="cuda")
    ack, counts = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    wire = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    work = torch.empty(W.rx_ack_work_bytes(n, n, W.ACK_CUMULATIVE), dtype=torch.uint8, device="cuda")

    def clear():
        sl.fill_(-1)

    def accept():
        W.accept_data_packets(ring, STRIDE, rl, n, SEQ0, n, img, sl, ok, place, ack)

    hdr = np.ascontiguousarray(ring[:, :8].cpu().numpy()).reshape(-1)
    row = {"n": n, "order": "permuted" if permuted else "in order", "stride": STRIDE, "ring_mb": round(n * STRIDE / 1e6, 1)}
    for name, mode in MODES:
        def acks():
            W.rx_build_acks(ring, STRIDE, rl, n, mode, SEQ0, n, ok, place, sl, wire, 16, 0, n, src, counts, work=work)

        clear()
        accept()
        wire.zero_()
        acks()
        torch.cuda.synchronize()
        seq, idx, (emitted, total) = A.build_acks(hdr, 8, u32(rl), mode, SEQ0, n, u32(place), u32(sl), ok=ok.cpu().numpy(),
                                                  vectorised=True)
        exact = bool(tuple(u32(counts)) == (emitted, total) == (n, n) and np.array_equal(u32(src), idx)
                     and np.array_equal(wire.cpu().numpy(), A.ack_bytes(seq))
                     and int(seq[-1]) == (int(u32(ack)[0]) if mode == W.ACK_CUMULATIVE else int(seq[-1])))
        if not exact:
            raise SystemExit(f"ack_bench: n {n} {row['order']} {name}: outputs are not exact")
        ta, tk = B.sample({"accept": (accept, clear, 1), "acks": (acks, None, 1)}, reps, warmup).values()
        ma, mk = float(np.median(ta)), float(np.median(tk))
        sa = stats(ta)
        row[name] = {"exact": exact, "kernel": W.LIB.wtp_last_kernel().decode(), "accept_ms": round(ma, 4),
                     "acks_ms": round(mk, 4), "ratio": round((ma + mk) / ma, 4),
                     "pair_ms": round(float(np.median(np.add(ta, tk))), 4),
                     "accept_iqr_pct": round(100 * (sa["p75"] - sa["p25"]) / sa["median"], 2),
                     "accept_ms_stats": sa, "acks_ms_stats": stats(tk), "acks_per_us": round(n / (mk * 1e3), 1)}
    return row


def main():
    ap = B.parser()
    ap.add_argument("--sizes", default="1048576,65536")
    B.add_out(ap, "ack")
    a = ap.parse_args()
    res = B.start("ack_bench", a, min_reps=20)
    rows = [case(int(n), permuted, a.reps, a.warmup) for n in a.sizes.split(",") for permuted in (False, True)]
    big = [r for r in rows if r["n"] == 1 << 20 and r["order"] == "in order"]
    res.update({"goal_ratio": 1.10, "goal_met": all(r[m]["ratio"] <= 1.10 for r in big for m, _ in MODES) if big else None,
                "cases": rows})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
