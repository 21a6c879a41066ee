#!/usr/bin/env python3
"""Whole-buffer CRC (wtp_crc32_buffer) against what a caller could do before it existed, in
one process, alternating per repetition, timed with device events:

  (a) wtp_crc32_batch_fixed over the 1456-B chunks: the chunk CRCs only, no file digest
  (b) wtp_crc32_buffer: the same braided launch plus the device fold of its CRCs
  (c) wtp_crc32_concat alone over the chunk CRCs (recorded, not gated)

Size: the workload's 1 M x 1456-B synthetic buffer (seed 0x5EED).  Checked before any
timing: (b) equals the host fold (wtp_crc32_combine) of (a)'s CRC vector, (c) equals it
too, and that vector's sha256 equals the reference's digest in
tests/golden/bench_digests.json, which ties the full-size result to the reference.
Also reported: the buffer call at 64 KiB (the C2 size) and, at both sizes, from base offset
8 (the head and tail route), each checked against the host fold / the CPU CRC.

Prints one JSON line and writes it to profiles/buffer/buffer_bench.json (--out).
Goal (1 M chunks, aligned): buffer_ms / batch_fixed_ms <= 1.10.
  python tools/buffer_bench.py [--reps 25] [--warmup 3] [--chunks 1048576] [--out PATH]"""
import hashlib
import json
import os

import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import wtp_crc32 as W
from bench_support import stats

MAXP, GOAL, OFF = 1456, 1.10, 8


def host_fold(crcs, last_len):
    d = 0
    for c in crcs[:-1].tolist():
        d = W.LIB.wtp_crc32_combine(d, c, MAXP)
    return int(W.LIB.wtp_crc32_combine(d, int(crcs[-1]), last_len))


def u32(t):
    return int(B.u32(t)[0])


def headline(n, reps, warmup):
    total = n * MAXP
    alloc = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    W.synth_fill(alloc)
    buf = alloc[:total]
    crcs = torch.empty(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    bwork = torch.full((W.buffer_work_bytes(total),), 0xFF, dtype=torch.uint8, device="cuda")
    cwork = torch.full((W.concat_work_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")

    def fixed():
        W.crc32_batch_fixed(buf, MAXP, MAXP, n, crcs)

    def whole():
        W.crc32_buffer(buf, total, out, work=bwork)

    def concat():
        W.crc32_concat(crcs, None, n, out, length=MAXP, last_len=MAXP, work=cwork)

    # the check, before any timing
    fixed()
    torch.cuda.synchronize()
    fixed_kernel = W.LIB.wtp_last_kernel().decode()
    vec = crcs.cpu().numpy().view(np.uint32)
    want = host_fold(vec, MAXP)
    sha = hashlib.sha256(vec.astype("<u4").tobytes()).hexdigest()
    with open(os.path.join(B.ROOT, "tests", "golden", "bench_digests.json")) as f:
        ref_sha = json.load(f)["sha256_by_packets"].get(str(n))
    whole()
    got_buffer = u32(out)
    fold_kernel = W.LIB.wtp_last_kernel().decode()
    concat()
    got_concat = u32(out)
    check = {"host_fold": "%08X" % want, "buffer": "%08X" % got_buffer, "concat": "%08X" % got_concat,
             "crc_vector_sha256": sha[:16], "reference_sha256_match": (sha == ref_sha) if ref_sha else None,
             "passed": bool(got_buffer == want and got_concat == want and (ref_sha is None or sha == ref_sha))}
    if not check["passed"]:
        raise SystemExit(f"buffer_bench: check failed before timing: {json.dumps(check)}")
    # the same bytes from base offset 8: 8-B head, one chunk fewer, 1448-B tail
    mis = alloc[OFF:OFF + total - OFF]
    W.crc32_buffer(mis, total - OFF, out, work=bwork)
    rest = torch.empty(1, dtype=torch.int32, device="cuda")
    W.crc32_buffer(alloc[:OFF], OFF, rest)  # crc32(first 8 bytes), to tie the offset result to `want`
    offset_ok = W.crc32_combine(u32(rest), u32(out), total - OFF) == want
    if not offset_ok:
        raise SystemExit("buffer_bench: offset-8 result does not combine to the whole-buffer CRC")

    def whole_off():
        W.crc32_buffer(mis, total - OFF, out, work=bwork)

    t = B.sample({"fixed": (fixed, None, 1), "buffer": (whole, None, 1), "concat": (concat, None, 1),
                  "buffer_off8": (whole_off, None, 1)}, reps, warmup)
    a, b, c, o = (float(np.median(t[k])) for k in ("fixed", "buffer", "concat", "buffer_off8"))
    return {"chunks": n, "bytes": total, "check": check, "offset8_check": bool(offset_ok),
            "kernels": [fixed_kernel, fold_kernel],
            "batch_fixed_ms": round(a, 4), "buffer_ms": round(b, 4), "concat_ms": round(c, 4),
            "buffer_off8_ms": round(o, 4), "ratio": round(b / a, 4), "ratio_off8": round(o / a, 4),
            "batch_fixed_stats": stats(t["fixed"]), "buffer_stats": stats(t["buffer"]),
            "concat_stats": stats(t["concat"]), "buffer_off8_stats": stats(t["buffer_off8"]),
            "batch_fixed_spread": B.spread(t["fixed"]),
            "buffer_gbps": round(total / (b * 1e-3) / 1e9, 1)}


def small(nbytes, reps, warmup):
    """The buffer call at the C2 size, aligned and from offset 8, checked against the CPU CRC."""
    alloc = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    W.synth_fill(alloc)
    host = alloc.cpu().numpy()
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    work = torch.full((W.buffer_work_bytes(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")
    res = {"bytes": nbytes}
    for name, off in (("aligned", 0), ("off8", OFF)):
        view = alloc[off:off + nbytes]

        def call():
            W.crc32_buffer(view, nbytes, out, work=work)

        call()
        if u32(out) != W.crc32(host[off:off + nbytes].tobytes()):
            raise SystemExit(f"buffer_bench: {nbytes} B at offset {off}: wrong CRC")
        ts = B.sample({name: (call, None, 1)}, reps, warmup)[name]
        res[name + "_ms"] = round(float(np.median(ts)), 4)
        res[name + "_stats"] = stats(ts)
    return res


def main():
    ap = B.parser()
    ap.add_argument("--chunks", type=int, default=1 << 20)
    B.add_out(ap, "buffer")
    a = ap.parse_args()
    res = B.start("buffer_bench", a, min_reps=25)
    head = headline(a.chunks, a.reps, a.warmup)
    res.update({"goal_ratio": GOAL, "headline_ratio": head["ratio"], "goal_met": bool(head["ratio"] <= GOAL), "headline": head,
                "c2_64KiB": small(65536, a.reps, a.warmup)})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
