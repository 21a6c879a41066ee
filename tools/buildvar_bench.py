#!/usr/bin/env python3
"""The mixed-length DATA builder (wtp_build_data_packets_var) against what a caller could
do before it existed, in one process, in turn per repetition, timed with device events:

  (a) the new call
  (b) wtp_crc32_batch_var on the same batch (the caller's first pass)
  (c) torch's contiguous device-to-device copy of as many bytes as the batch's payloads
      (a lower bound of the caller's ragged gather-copy: one pass, no scatter)
  (d) wtp_build_data_packets over the same payload byte count as 1456-B chunks

(b) + (c) is what the two-pass route costs before any header is written.  Batches: C5's 1 M
Zipf(1.1) packed payloads, 64 K of them, and 1 M x 1456 B given as offsets and lengths; 1472-B
slots.  Every timed configuration is checked exact first, on the device: d_wire_len, d_crc_out
and the 16 header bytes of every slot against the CPU oracle's CRCs, the payload bytes of
every slot against the source, and for the 1456-B batch the whole ring against (d)'s.

Prints one JSON line and writes it to profiles/buildvar/buildvar_bench.json (--out).
Goal (1 M Zipf): a / (b + c) <= 1.10, both sides from the same run.
  python tools/buildvar_bench.py [--reps 25] [--warmup 3] [--batches zipf_1m,zipf_64k,full_1m] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the oracle's directories on sys.path
import oracle as O
import wtp_crc32 as W
from bench_support import stats

STRIDE, MAXP, SEQ0, GOAL = 1472, 1456, 0xFFFFF000, 1.10
BATCHES = {"zipf_1m": (1 << 20, "zipf"), "zipf_64k": (1 << 16, "zipf"), "full_1m": (1 << 20, "full")}


def check_exact(n, lens, offs, host, src, wire, wl, crc):
    """Every output of the new call against the CPU oracle's CRCs and the source bytes."""
    full = bool((lens == MAXP).all())  # the threaded oracle for 1.5 GB of whole chunks
    want_crc = O.batch_fixed(host, MAXP, MAXP, n, threads=16) if full else O.batch_var(host, offs, lens)
    hdr = np.stack([np.full(n, 2, np.uint32), (SEQ0 + np.arange(n, dtype=np.uint64)).astype(np.uint32), lens, want_crc], axis=1)
    hdr = torch.from_numpy(hdr.astype(">u4").view(np.uint8).reshape(n, 16)).cuda()
    slots = wire.view(n, STRIDE)
    ok = torch.equal(slots[:, :16], hdr)
    ok = ok and np.array_equal(wl.cpu().numpy().view(np.uint32), lens + 16)
    ok = ok and np.array_equal(crc.cpu().numpy().view(np.uint32), want_crc)
    dl = torch.from_numpy(lens.astype(np.int64)).cuda()
    col = torch.arange(MAXP, device="cuda")[None, :]
    ends = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    for r0 in range(0, n, 1 << 15):  # packed payloads: the masked rows are one source range
        r1 = min(n, r0 + (1 << 15))
        got = slots[r0:r1, 16:][col < dl[r0:r1, None]]
        ok = ok and torch.equal(got, src[int(ends[r0]):int(ends[r1])])
    return bool(ok)


def case(name, reps, warmup):
    n, kind = BATCHES[name]
    lens = O.zipf_lengths(n) if kind == "zipf" else np.full(n, MAXP, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum())
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=0xB1D)
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    wire = torch.empty(n * STRIDE, dtype=torch.uint8, device="cuda")
    wl = torch.empty(n, dtype=torch.int32, device="cuda")
    crc = torch.empty(n, dtype=torch.int32, device="cuda")
    crc_b = torch.empty(n, dtype=torch.int32, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    n_d = (total + MAXP - 1) // MAXP  # (d): the same bytes as 1456-B chunks, n_d <= n slots
    wl_d = torch.empty(n_d, dtype=torch.int32, device="cuda")

    def a_new():
        W.build_data_packets_var(src, total, d_offs, d_lens, n, SEQ0, wire, STRIDE, wl, crc)

    def b_crc():
        W.crc32_batch_var(src, total, d_offs, d_lens, n, crc_b)

    def c_copy():
        dst.copy_(src)

    def d_fixed():
        W.build_data_packets(src, total, SEQ0, wire, STRIDE, wl_d)

    wire.fill_(0xA5)
    a_new()
    torch.cuda.synchronize()
    kernel = W.LIB.wtp_last_kernel().decode()
    exact = check_exact(n, lens, offs, src.cpu().numpy(), src, wire, wl, crc)
    b_crc()
    c_copy()
    torch.cuda.synchronize()
    exact = exact and torch.equal(crc_b, crc) and torch.equal(dst, src)
    if kind == "full":  # byte-identical to the fixed builder's ring
        ring_a = wire.clone()
        d_fixed()
        torch.cuda.synchronize()
        exact = exact and torch.equal(ring_a, wire)
        del ring_a
    if not exact:
        raise SystemExit(f"buildvar_bench: {name}: outputs are not exact")
    t = B.sample({k: (fn, None, 1) for k, fn in zip("abcd", (a_new, b_crc, c_copy, d_fixed))}, reps, warmup)
    two_pass = np.asarray(t["b"]) + np.asarray(t["c"])
    a, b, c, d = (float(np.median(t[k])) for k in "abcd")
    traffic = 2 * total + 12 * n + 16 * n + 8 * n  # reads len + 12 B, writes 16 + len + 8 B per datagram
    return {"batch": name, "n": n, "stride": STRIDE, "payload_bytes": total, "mean_len": round(total / n, 1),
            "exact": exact, "kernel": kernel,
            "a_build_var_ms": round(a, 4), "b_crc_batch_var_ms": round(b, 4), "c_copy_ms": round(c, 4),
            "d_build_fixed_ms": round(d, 4), "d_chunks": n_d,
            "a_over_b_plus_c": round(a / (b + c), 4), "a_over_d": round(a / d, 4),
            "a_stats": stats(t["a"]), "b_plus_c_stats": stats(two_pass), "d_stats": stats(t["d"]),
            "a_spread": B.spread(t["a"]), "b_plus_c_spread": B.spread(two_pass),
            "a_model_traffic_gbps": round(traffic / (a * 1e-3) / 1e9, 1)}


def main():
    ap = B.parser()
    ap.add_argument("--batches", default="zipf_1m,zipf_64k,full_1m")
    B.add_out(ap, "buildvar")
    a = ap.parse_args()
    res = B.start("buildvar_bench", a, min_reps=20)
    cases = [case(b, a.reps, a.warmup) for b in a.batches.split(",")]
    head = next((c for c in cases if c["batch"] == "zipf_1m"), None)
    res.update({"goal_ratio": GOAL, "headline_ratio": head["a_over_b_plus_c"] if head else None,
                "goal_met": bool(head["a_over_b_plus_c"] <= GOAL) if head else None, "cases": cases})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
