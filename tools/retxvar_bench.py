#!/usr/bin/env python3
"""The mixed-length selective retransmit (wtp_tx_build_retransmit_var) against three
yardsticks, none of them the code under test, in one process, the contenders taken in turn
per repetition, timed with device events:

  var      the new call on a window of 65 536 slots with about 1 %, 10 % and 100 % of them due
           (a seeded random set; the others ACKed), into a ring of max_sel = inflight entries
           and into one of max_sel = due entries; the timers are restored before the timed
           window.  Record sets: `full`, every record 1456 B at 16-B aligned offsets, and
           `zipf`, Zipf(1.1) lengths (oracle.zipf_lengths), packed.
  build    wtp_build_data_packets_var over as many contiguous records of the same set: what a
           first transmission of as many packets costs.  The call adds the count and select
           launches and one indirection.
  fixed    set `full` only: wtp_tx_build_retransmit on the same window and acked pattern.
  3pass    what a caller writes today for records: wtp_crc32_batch_var over the gathered
           offsets of the due records, plus a contiguous device-to-device copy of as many
           bytes (a lower bound of the ragged gather into the slots; the selection itself is
           not counted).  The row to read is 10 % of set `zipf`: a retransmit set of mixed records.

Every timed configuration is checked first: counts, sel, wire_len, crc_out and every emitted
slot must equal the builder's wire image of the same records (and the fixed call's ring on
set `full`).  No target ratio is fixed.

Prints one JSON line and writes it to profiles/retxvar/retxvar_bench.json (--out).
  python tools/retxvar_bench.py [--reps 25] [--warmup 3] [--inflight 65536] [--configs full:0.01,...] [--out PATH]
  python tools/retxvar_bench.py --trace [--trace-out profiles/retxvar/kernel_trace.txt]
--trace touches no device itself: it starts, one after the other, one child per configuration
under `rocprofv3 --kernel-trace --stats` (ring = the window) and writes the per-kernel
durations (tools/kstats.py's columns, split by grid) under one heading per configuration."""
import glob
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the oracle's directories on sys.path
from bench_support import i32, iqr, stats

STRIDE, MAXP, SEQ0, NOW, TIMEOUT = 1472, 1456, 0xFFFF8000, 10_000, 500
SETS, FRACTIONS = ("full", "zipf"), (0.01, 0.1, 1.0)


def bench(a):
    import oracle as O  # here, not at the top: --trace's parent loads no library
    import wtp_crc32 as W

    head = B.start("retxvar_bench", a, min_reps=0 if a.short else 20)
    inflight = a.inflight
    wanted = [c.split(":") for c in a.configs.split(",")] if a.configs else [(s, str(f)) for s in SETS for f in FRACTIONS]
    rows = []
    for kind in SETS:
        fracs = [float(f) for s, f in wanted if s == kind]
        if not fracs:
            continue
        lens = np.full(inflight, MAXP, np.uint32) if kind == "full" else O.zipf_lengths(inflight).astype(np.uint32)
        offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
        total = int(lens.sum())
        src = torch.empty(total, dtype=torch.uint8, device="cuda")
        W.synth_fill(src, seed=0x7E7)
        d_offs, d_lens = torch.from_numpy(offs.view(np.int64)).cuda(), i32(lens)
        image = torch.zeros((inflight, STRIDE), dtype=torch.uint8, device="cuda")
        image_wl, image_crc = (torch.zeros(inflight, dtype=torch.int32, device="cuda") for _ in range(2))
        W.build_data_packets_var(src, total, d_offs, d_lens, inflight, SEQ0, image, STRIDE, image_wl, image_crc)
        wire, ywire, fwire = (torch.empty((inflight, STRIDE), dtype=torch.uint8, device="cuda") for _ in range(3))
        wlen, ywlen, sel, crc, ycrc = (torch.empty(inflight, dtype=torch.int32, device="cuda") for _ in range(5))
        counts = torch.zeros(2, dtype=torch.int32, device="cuda")
        work = torch.empty(W.tx_work_bytes(inflight, inflight), dtype=torch.uint8, device="cuda")
        sent0 = torch.full((inflight,), NOW - TIMEOUT - 1, dtype=torch.int32, device="cuda")
        sent = sent0.clone()
        for frac in fracs:
            mask = np.random.default_rng(int(frac * 1000)).random(inflight) < frac
            due_slots = np.flatnonzero(mask)
            due = int(due_slots.size)
            acked = i32(~mask)
            idx = torch.from_numpy(due_slots).cuda()
            g_offs, g_lens = d_offs[idx].contiguous(), d_lens[idx].contiguous()
            due_bytes = int(lens[due_slots].sum())
            ybytes = int(lens[:due].sum())
            dst = torch.empty(max(due_bytes, 1), dtype=torch.uint8, device="cuda")

            def restore():
                sent.copy_(sent0)

            def build():
                W.build_data_packets_var(src, total, d_offs, d_lens, due, SEQ0, ywire, STRIDE, ywlen, ycrc)

            def three_pass():
                W.crc32_batch_var(src, total, g_offs, g_lens, due, ycrc)
                dst[:due_bytes].copy_(src[:due_bytes])

            row = {"set": kind, "inflight": inflight, "fraction": frac, "due": due, "payload_mb": round(due_bytes / 1e6, 3),
                   "mean_len": round(due_bytes / max(due, 1), 1)}
            for label, max_sel in (("ring_inflight", inflight), ("ring_due", due)):
                if a.ring and label != a.ring:
                    continue

                def var():
                    W.tx_build_retransmit_var(src, total, d_offs, d_lens, SEQ0, inflight, acked, sent, NOW, TIMEOUT, 0, wire,
                                              STRIDE, max_sel, sel, wlen, crc, counts, work=work)

                def fixed():
                    W.tx_build_retransmit(src, total, SEQ0, inflight, acked, sent, NOW, TIMEOUT, 0, fwire, STRIDE, max_sel, sel,
                                          wlen, counts, work=work)

                wire.zero_()
                restore()
                var()
                torch.cuda.synchronize()
                kernel = W.LIB.wtp_last_kernel().decode()
                exact = bool(counts.tolist() == [due, due] and torch.equal(sel[:due], idx.to(torch.int32))
                             and torch.equal(wire[:due], image[idx]) and torch.equal(wlen[:due], image_wl[idx])
                             and torch.equal(crc[:due], image_crc[idx]) and bool((sent[idx] == NOW).all()))
                if kind == "full":
                    fwire.zero_()
                    restore()
                    fixed()
                    torch.cuda.synchronize()
                    exact = exact and torch.equal(fwire[:due], wire[:due])
                if not exact:
                    raise SystemExit(f"retxvar_bench: set {kind} fraction {frac} max_sel {max_sel}: outputs are not exact")
                units = {"var": (var, restore, 1), "build": (build, None, 1), "3pass": (three_pass, None, 1)}
                if kind == "full":
                    units["fixed"] = (fixed, restore, 1)
                t = B.sample(units, a.reps, a.warmup)
                v, b, p = (float(np.median(t[k])) for k in ("var", "build", "3pass"))
                res = {"max_sel": max_sel, "exact": exact, "kernel": kernel, "var_ms": round(v, 4), "build_var_ms": round(b, 4),
                       "var_over_build": round(v / b, 4), "three_pass_ms": round(p, 4), "var_over_three_pass": round(v / p, 4),
                       "var_ms_stats": stats(t["var"]), "build_var_ms_stats": stats(t["build"]),
                       "three_pass_ms_stats": stats(t["3pass"]), "var_payload_gbps": round(due_bytes / (v * 1e-3) / 1e9, 1)}
                if kind == "full":
                    f = float(np.median(t["fixed"]))
                    res.update({"fixed_ms": round(f, 4), "fixed_ms_stats": stats(t["fixed"]), "var_over_fixed": round(v / f, 4),
                                "var_minus_fixed_ms": round(v - f, 4), "two_iqr_ms": round(iqr(t["var"]) + iqr(t["fixed"]), 4),
                                "slower_than_fixed_beyond_two_iqr": B.below_by_more_than_both_iqr(t["fixed"], t["var"])})
                row[label] = res
            rows.append(row)
        del src, image, wire, ywire, fwire
    B.write_result({**head, "rows": rows}, a.out)


def kernel_table(folder):
    """tools/kstats.py --grid over the rocpd databases under `folder`, the library's kernels only."""
    by = {}
    for db in glob.glob(os.path.join(folder, "**", "*.db"), recursive=True):
        c = sqlite3.connect(db)
        for name, dur, gx, wx in c.execute("select name, duration, grid_x, workgroup_x from kernels"):
            if "wtp::" in name:
                by.setdefault(name[:90] + f" grid {gx // max(wx, 1)}x{wx}", []).append(dur / 1e3)
    out = [f"{'count':>6} {'mean':>9} {'median':>9} {'p10':>9} {'p90':>9}  kernel (us)"]
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        x = np.array(v)
        out.append(f"{x.size:6d} {x.mean():9.2f} {np.median(x):9.2f} {np.percentile(x, 10):9.2f} {np.percentile(x, 90):9.2f}  {k}")
    return out


def trace(a):
    lines = []
    for kind in SETS:
        for frac in FRACTIONS:
            tmp = tempfile.mkdtemp(prefix="retxvar_trace_")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--configs", f"{kind}:{frac}", "--ring", "ring_inflight", "--inflight", str(a.inflight), "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--out", os.path.join(tmp, "bench.json")]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
            lines += [f"## set {kind}, {frac:g} of {a.inflight} slots due, ring = the window"] + kernel_table(tmp) + [""]
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.trace_out)), exist_ok=True)
    with open(a.trace_out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines), flush=True)


def main():
    ap = B.parser()
    ap.add_argument("--inflight", type=int, default=65536)
    ap.add_argument("--configs", default="", help="set:fraction,... (default: every set and fraction)")
    ap.add_argument("--ring", default="", help="ring_inflight or ring_due only")
    ap.add_argument("--short", action="store_true", help="allow fewer than 20 repetitions (not for committed figures)")
    B.add_out(ap, "retxvar")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-out", default=os.path.join(B.ROOT, "profiles", "retxvar", "kernel_trace.txt"))
    a = ap.parse_args()
    trace(a) if a.trace else bench(a)


if __name__ == "__main__":
    main()
