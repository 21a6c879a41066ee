#!/usr/bin/env python3
"""The in-order flush (wtp_rx_deliver) against what a caller could do before it existed, in
one process, in turn per repetition, timed with device events:

  (a) the new call
  (b) torch on the device: masked_select of the (n, 1456) image under col < len, the mask
      built inside the timed region (it depends on the lengths)
  (c) torch's contiguous device-to-device copy of as many bytes as are delivered (a floor:
      one contiguous range read and written, where the call reads 1456-B-strided slots)
  (v) the new call followed by wtp_crc32_verify_batch of the next datagram batch (the
      figure a cache policy of the copy kernel is chosen by)

Windows: 1 M Zipf(1.1) slots, 64 K of them, and 1 M x 1456 B.  The window state is made on
the device by wtp_build_data_packets_var -> wtp_accept_data_packets from a packed stream,
and every timed configuration is checked exact first: the delivered stream against that
source, d_offsets_out / d_lengths_out / d_counts against the lengths, (b) against the source.

Prints one JSON line and writes it to profiles/deliver/deliver_bench.json (--out).
Acceptance: a < b at every window by more than the sum of both interquartile ranges.
  python tools/deliver_bench.py [--reps 25] [--warmup 3] [--batches zipf_1m,zipf_64k,full_1m] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the oracle's directories on sys.path
import oracle as O
import wtp_crc32 as W
from bench_support import iqr, stats

STRIDE, MAXP, SEQ0 = 1472, 1456, 0xFFFFF000
BATCHES = {"zipf_1m": (1 << 20, "zipf"), "zipf_64k": (1 << 16, "zipf"), "full_1m": (1 << 20, "full")}


def case(name, reps, warmup):
    n, kind = BATCHES[name]
    lens = O.zipf_lengths(n) if kind == "zipf" else np.full(n, MAXP, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    total = int(lens.sum())
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    W.synth_fill(src, seed=0xD11)
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    # the window state, made by the sender's builder and the receiver's accept
    ring = torch.empty(n * STRIDE, dtype=torch.uint8, device="cuda")
    wl = torch.empty(n, dtype=torch.int32, device="cuda")
    W.build_data_packets_var(src, total, d_offs, d_lens, n, SEQ0, ring, STRIDE, wl, None)
    img = torch.full((n * MAXP,), 0x3C, dtype=torch.uint8, device="cuda")
    sl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    W.accept_data_packets(ring, STRIDE, wl, n, SEQ0, n, img, sl, ok)
    torch.cuda.synchronize()
    exact = bool((ok == 1).all()) and torch.equal(sl, d_lens)

    out = torch.empty(total, dtype=torch.uint8, device="cuda")
    o_out = torch.empty(n, dtype=torch.int64, device="cuda")
    l_out = torch.empty(n, dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    work = torch.empty(W.rx_deliver_work_bytes(n), dtype=torch.uint8, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    ok_v = torch.empty(n, dtype=torch.uint8, device="cuda")
    rows = img.view(n, MAXP)
    col = torch.arange(MAXP, device="cuda", dtype=torch.int32)[None, :]
    got_b = [None]

    def a_new():
        W.rx_deliver(img, sl, n, n, out, total, 0, o_out, l_out, counts, work=work)

    def b_torch():
        got_b[0] = torch.masked_select(rows, col < sl[:, None])

    def c_copy():
        dst.copy_(src)

    def v_next():
        a_new()
        W.verify_batch(ring, STRIDE, wl, n, ok_v)

    out.fill_(0xA5)
    a_new()
    torch.cuda.synchronize()
    kernel = W.LIB.wtp_last_kernel().decode()
    exact = exact and torch.equal(out, src) and torch.equal(o_out, d_offs) and torch.equal(l_out, d_lens)
    exact = exact and counts.cpu().tolist() == [n, n, total, total]
    b_torch()
    c_copy()
    v_next()
    torch.cuda.synchronize()
    exact = exact and torch.equal(got_b[0], src) and torch.equal(dst, src) and bool((ok_v == 1).all())
    if not exact:
        raise SystemExit(f"deliver_bench: {name}: outputs are not exact")
    t = B.sample({k: (fn, None, 1) for k, fn in zip("abcv", (a_new, b_torch, c_copy, v_next))}, reps, warmup)
    a, b, c, v = (float(np.median(t[k])) for k in "abcv")
    traffic = (total + 4 * n) + (total + 12 * n)  # reads len + 4 B, writes len + 12 B per record
    return {"batch": name, "n": n, "delivered_bytes": total, "mean_len": round(total / n, 1), "exact": exact,
            "kernel": kernel, "a_deliver_ms": round(a, 4), "b_masked_select_ms": round(b, 4), "c_copy_ms": round(c, 4),
            "v_deliver_then_verify_ms": round(v, 4), "a_over_b": round(a / b, 4), "a_over_c": round(a / c, 4),
            "a_stats": stats(t["a"]), "b_stats": stats(t["b"]), "c_stats": stats(t["c"]), "v_stats": stats(t["v"]),
            "a_iqr_ms": round(iqr(t["a"]), 4), "b_iqr_ms": round(iqr(t["b"]), 4),
            "a_below_b_by_more_than_both_iqr": B.below_by_more_than_both_iqr(t["a"], t["b"]),
            "a_model_traffic_gbps": round(traffic / (a * 1e-3) / 1e9, 1),
            "a_payload_read_plus_write_gbps": round(2 * total / (a * 1e-3) / 1e9, 1)}


def main():
    ap = B.parser()
    ap.add_argument("--batches", default="zipf_1m,zipf_64k,full_1m")
    B.add_out(ap, "deliver")
    a = ap.parse_args()
    res = B.start("deliver_bench", a, min_reps=20)
    cases = [case(b, a.reps, a.warmup) for b in a.batches.split(",")]
    res.update({"accepted": all(c["a_below_b_by_more_than_both_iqr"] for c in cases), "cases": cases})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
