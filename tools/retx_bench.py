#!/usr/bin/env python3
"""Device-side sender window (wtp_tx_ingest_acks, wtp_tx_build_retransmit) against the one
yardstick that existed before it, in one process, alternating per repetition, timed with
device events:

  ingest   a window of 65 536 slots and a full batch of selective 16-byte ACKs, one per slot
           in a seeded random order (stride 16); d_acked is cleared before the timed window.
  retx     the same window with about 1 %, 10 % and 100 % of its slots due (a seeded random
           set; the others ACKed), into a ring of max_sel = inflight entries (the grids are
           sized from max_sel, so this is the dearest ring) and into one of max_sel = due
           entries; the timers are restored before the timed window.
  build    wtp_build_data_packets over the same number of contiguous chunks of the same
           buffer: the fused single-pass builder, what a first transmission of as many
           packets costs.
  crc      wtp_crc32_batch_var (the general kernel) over the same selection: what a separate
           CRC pass before the copy would cost on its own; the call itself hashes inside its
           emit kernel and reads every payload byte once.

Every timed configuration is checked first: sel, counts and every emitted datagram must
equal the builder's wire image of the same buffer.  No target ratio is fixed.

Prints one JSON line and writes it to profiles/retx/retx_bench.json (--out).
  python tools/retx_bench.py [--reps 25] [--warmup 3] [--inflight 65536] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import wtp_crc32 as W
from bench_support import i32, stats

STRIDE, MAXP, SEQ0, NOW, TIMEOUT = 1472, 1456, 0xFFFF8000, 10_000, 500


def ingest_case(inflight, reps, warmup):
    perm = np.random.default_rng(0xACC).permutation(inflight)
    hdr = np.zeros((inflight, 4), dtype=">u4")
    hdr[:, 0], hdr[:, 1] = 3, (SEQ0 + perm) & 0xFFFFFFFF
    ring = torch.from_numpy(hdr.view(np.uint8).reshape(-1)).cuda()
    rl = torch.full((inflight,), 16, dtype=torch.int32, device="cuda")
    acked = torch.zeros(inflight, dtype=torch.int32, device="cuda")
    ok = torch.zeros(inflight, dtype=torch.uint8, device="cuda")
    hit = torch.zeros(inflight, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")

    def run():
        W.tx_ingest_acks(ring, 16, rl, inflight, W.ACK_SELECTIVE, SEQ0, inflight, acked, ok, hit, counts)

    def verify():
        W.verify_batch(ring, 16, rl, inflight, ok)

    run()
    torch.cuda.synchronize()
    exact = bool(ok.all() and acked.all() and counts.tolist() == [inflight, inflight]
                 and torch.equal(hit, i32(perm)))
    if not exact:
        raise SystemExit("retx_bench: ingest outputs are not exact")
    t, tv = B.sample({"ingest": (run, acked.zero_, 1), "verify": (verify, None, 1)}, reps, warmup).values()
    return {"inflight": inflight, "n": inflight, "mode": "selective", "stride": 16, "exact": exact,
            "ingest_ms": round(float(np.median(t)), 4), "ingest_ms_stats": stats(t),
            "verify_batch_ms": round(float(np.median(tv)), 4), "acks_per_us": round(inflight / (np.median(t) * 1e3), 1)}


def retx_cases(inflight, reps, warmup):
    total = inflight * MAXP - 100
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=0x7E7)
    image = torch.zeros((inflight, STRIDE), dtype=torch.uint8, device="cuda")
    W.build_data_packets(src, total, SEQ0, image, STRIDE)
    wire = torch.empty((inflight, STRIDE), dtype=torch.uint8, device="cuda")
    ywire = torch.empty((inflight, STRIDE), dtype=torch.uint8, device="cuda")
    wlen = torch.empty(inflight, dtype=torch.int32, device="cuda")
    sel = torch.empty(inflight, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    crc = torch.empty(inflight, dtype=torch.int32, device="cuda")
    work = torch.empty(W.tx_work_bytes(inflight, inflight), dtype=torch.uint8, device="cuda")
    sent0 = torch.full((inflight,), NOW - TIMEOUT - 1, dtype=torch.int32, device="cuda")
    sent = sent0.clone()
    rows = []
    for frac in (0.01, 0.1, 1.0):
        mask = np.random.default_rng(int(frac * 1000)).random(inflight) < frac
        due_slots = np.flatnonzero(mask)
        due = int(due_slots.size)
        acked = i32(~mask)
        offs = torch.from_numpy((due_slots * MAXP).astype(np.int64)).cuda()
        lens = i32(np.minimum(MAXP, total - due_slots * MAXP))
        ybytes = min(total, due * MAXP)

        def restore():
            sent.copy_(sent0)

        def build():
            W.build_data_packets(src, ybytes, SEQ0, ywire, STRIDE, wlen)

        def crc_only():
            W.crc32_batch_var(src, total, offs, lens, due, crc)

        row = {"inflight": inflight, "fraction": frac, "due": due, "payload_mb": round(due * MAXP / 1e6, 2)}
        for label, max_sel in (("ring_inflight", inflight), ("ring_due", due)):
            def retx():
                W.tx_build_retransmit(src, total, SEQ0, inflight, acked, sent, NOW, TIMEOUT, 0, wire, STRIDE, max_sel,
                                      sel, wlen, counts, work=work)

            wire.zero_()
            restore()
            retx()
            torch.cuda.synchronize()
            kernel = W.LIB.wtp_last_kernel().decode()
            idx = torch.from_numpy(due_slots).cuda()
            exact = bool(counts.tolist() == [due, due] and torch.equal(sel[:due], idx.to(torch.int32))
                         and torch.equal(wire[:due, :16 + MAXP - 100], image[idx][:, :16 + MAXP - 100])
                         and torch.equal(wire[:due - 1], image[idx][:due - 1]))
            if not exact:
                raise SystemExit(f"retx_bench: fraction {frac} max_sel {max_sel}: outputs are not exact")
            t = B.sample({"retx": (retx, restore, 1), "build": (build, None, 1), "crc": (crc_only, None, 1)}, reps, warmup)
            r, b, c = (float(np.median(t[k])) for k in ("retx", "build", "crc"))
            row[label] = {"max_sel": max_sel, "exact": exact, "kernel": kernel,
                          "retx_ms": round(r, 4), "build_ms": round(b, 4), "ratio": round(r / b, 4),
                          "separate_crc_pass_ms": round(c, 4),
                          "retx_ms_stats": stats(t["retx"]), "build_ms_stats": stats(t["build"]),
                          "retx_payload_gbps": round(due * MAXP / (r * 1e-3) / 1e9, 1)}
        rows.append(row)
    return rows


def main():
    ap = B.parser()
    ap.add_argument("--inflight", type=int, default=65536)
    B.add_out(ap, "retx")
    a = ap.parse_args()
    res = B.start("retx_bench", a, min_reps=20)
    res.update({"ingest": ingest_case(a.inflight, a.reps, a.warmup), "retransmit": retx_cases(a.inflight, a.reps, a.warmup)})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
