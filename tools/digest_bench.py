#!/usr/bin/env python3
"""wtp_rx_digest_flows at the size of a large receive round, timed with device events, once from
captured graphs and once back to back.  Every shape is about 95 MB of delivered records, so the
rows are comparable:

  shapes    64 flows x 1024 slots, 1024 x 64, 65 536 x 1 and 1 x 65 536 of full 1456-byte records,
            and 65 536 flows of one 64-byte record (the per-flow overhead).  The stream and
            d_flow_info of a shape are what wtp_rx_deliver_flows writes for a state whose slots are
            all filled; the digest's state is zeroed once and then runs on.
  beside    on the same bytes: "per_flow", what a caller does today, F wtp_crc32_buffer calls over
            the flows' ranges from one captured graph (F = 64 and 1024 only); "buffer", one
            wtp_crc32_buffer over the whole delivered range, the byte-rate yardstick; "deliver",
            wtp_rx_deliver_flows on the state that produced the stream, the call the digest follows.
  cold      the 64-flow shape over 12 copies of the stream at distinct addresses, 1.1 GB in all, one
            call per copy in turn: the 95 MB of a warm row sit in the 256-MiB Infinity Cache.

Every variant is first checked against tests/digest_model.py (and the buffer calls against the
oracle).  Two conditions are read from the result: the digest is faster than the per-flow calls
at 64 and at 1024 flows ("vs_per_flow", with the ratio), and one flow takes no longer than 64
flows at the same bytes beyond the larger min-to-max range of the two rows ("one_vs_64").

Prints one JSON line and writes it to profiles/digest/digest_bench.json (--out).
  python tools/digest_bench.py [--reps 25] [--warmup 3] [--inner 10] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import digest_model as M
import oracle as O
import wtp_crc32 as W
from bench_support import stats, u32, z

MAXP, SLOTS, COPIES = 1456, 1 << 16, 12
SHAPES = {"64x1024": (64, 1024, MAXP), "1024x64": (1024, 64, MAXP), "65536x1": (SLOTS, 1, MAXP), "1x65536": (1, SLOTS, MAXP),
          "65536x1_of_64B": (SLOTS, 1, 64)}


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Shape:
    """The device state of one shape: the window image with every slot filled, the stream and
    d_flow_info that deliver_flows makes of it, and the digest's state, outputs and scratch."""

    def __init__(self, nf, w, rec, img):
        self.nf, self.w, self.bytes = nf, w, nf * w * rec
        self.img, self.sl = img, z(nf * w, fill=rec)
        self.stream = torch.empty(self.bytes + 16, dtype=torch.uint8, device="cuda")[:self.bytes]
        self.adv, self.info, self.dcnt = z(nf, torch.int64), z(4 * nf, torch.int64), z(4, torch.int64)
        self.dwork = torch.empty(W.rx_deliver_flows_work_bytes(nf, w), dtype=torch.uint8, device="cuda")
        self.crc, self.nb, self.counts = z(nf), z(nf, torch.int64), z(4, torch.int64)
        self.work = torch.empty(W.rx_digest_scratch_bytes(nf), dtype=torch.uint8, device="cuda")

    def deliver(self):
        W.rx_deliver_flows(self.img, self.sl, self.nf, self.w, self.w, self.stream, self.bytes, 0, None, None, self.adv, self.info,
                           self.dcnt, work=self.dwork)

    def digest(self, stream=None):
        W.rx_digest_flows(self.stream if stream is None else stream, self.bytes, self.info, self.nf, self.crc, self.nb, None, None, 0,
                          None, None, 0, None, None, self.counts, work=self.work)

    def check(self, name):
        """One deliver and one digest from a zeroed state against the model; returns the host stream."""
        self.deliver()
        self.digest()
        torch.cuda.synchronize()
        host, info = self.stream.cpu().numpy(), u64(self.info).reshape(-1, 4)
        want = M.digest(host, self.bytes, info, np.zeros(self.nf, np.uint32), np.zeros(self.nf, np.uint64))
        if not (int(u64(self.dcnt)[2]) == self.bytes and np.array_equal(u32(self.crc), want[0]) and np.array_equal(u64(self.nb), want[1])
                and np.array_equal(u64(self.counts), want[4])):
            raise SystemExit(f"digest_bench: {name} is not exact")
        return host, info


def main():
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=10)
    B.add_out(ap, "digest")
    a = ap.parse_args()
    res = B.start("digest_bench", a, min_reps=10)
    img = torch.randint(0, 256, (SLOTS * MAXP,), dtype=torch.uint8, device="cuda")
    calls, slow, rows = {}, {}, {}
    out1 = z(1)
    for name, (nf, w, rec) in SHAPES.items():
        s = Shape(nf, w, rec, img)
        host, info = s.check(name)
        rows[name] = {"flows": nf, "slots_per_flow": w, "record_bytes": rec, "bytes": s.bytes}
        calls[name] = (s.digest, a.inner)
        calls[name + "/deliver"] = (s.deliver, a.inner)
        bwork = torch.empty(W.buffer_work_bytes(s.bytes), dtype=torch.uint8, device="cuda")
        whole = (lambda s=s, bwork=bwork: W.crc32_buffer(s.stream, s.bytes, out1, work=bwork))
        whole()
        if int(u32(out1)[0]) != O.crc32(host):
            raise SystemExit(f"digest_bench: the buffer call over {name} is not exact")
        calls[name + "/buffer"] = (whole, a.inner)
        if nf in (64, 1024):  # what a caller does today: one call per flow, the F values then folded on the host
            outs = z(nf)
            ranges = [(int(b), int(n)) for b, n in info[:, 2:]]

            def per_flow(s=s, outs=outs, ranges=ranges, bwork=bwork):
                for f, (b, n) in enumerate(ranges):
                    W.crc32_buffer(s.stream[b:], n, outs[f:], work=bwork)

            per_flow()
            if not np.array_equal(u32(outs), u32(s.crc)):  # one round from zero: the flow's CRC is its segment's
                raise SystemExit(f"digest_bench: the per-flow calls over {name} are not exact")
            slow[name + "/per_flow"] = (per_flow, 1)
        if name == "64x1024":  # the cold variant: the same call over address-distinct copies of the stream in turn
            copies = [s.stream.clone() for _ in range(COPIES)]
            calls[name + "/cold"] = ((lambda s=s, copies=copies: [s.digest(c) for c in copies]), 1)
            rows[name]["cold_bytes"] = COPIES * s.bytes
    for how in ("graph", "back_to_back"):
        t = B.sample(B.repeated(calls, how), a.reps, a.warmup, alternate=True)
        if how == "graph":
            t.update(B.sample(B.repeated(slow, how), max(a.reps // 2, 10), 2))
        t["64x1024/cold"] = [v / COPIES for v in t["64x1024/cold"]]
        rows[how] = {"unit_ms": {name: stats(v) for name, v in t.items()}}
    g = rows["graph"]["unit_ms"]
    for name in SHAPES:
        rows[name]["GBps_graph"] = round(rows[name]["bytes"] / g[name]["median"] / 1e6, 1)
        rows[name]["buffer_GBps_graph"] = round(rows[name]["bytes"] / g[name + "/buffer"]["median"] / 1e6, 1)
        rows[name]["share_of_deliver"] = round(g[name]["median"] / g[name + "/deliver"]["median"], 3)
    rows["64x1024"]["cold_GBps_graph"] = round(rows["64x1024"]["bytes"] / g["64x1024/cold"]["median"] / 1e6, 1)
    gates = {"vs_per_flow": {}}
    for name in ("64x1024", "1024x64"):
        ratio = g[name + "/per_flow"]["median"] / g[name]["median"]
        gates["vs_per_flow"][name] = {"per_flow_ms": g[name + "/per_flow"]["median"], "digest_ms": g[name]["median"],
                                      "ratio": round(ratio, 1), "faster": bool(g[name]["max"] < g[name + "/per_flow"]["min"])}
    one, many = g["1x65536"], g["64x1024"]
    gap, allowed = one["median"] - many["median"], max(one["max"] - one["min"], many["max"] - many["min"])
    gates["one_vs_64"] = {"one_flow_ms": one, "flows_64_ms": many, "gap_ms": round(gap, 4), "spread_ms": round(allowed, 4),
                          "within_spread": bool(gap <= allowed)}
    res.update({"inner": a.inner, "unit": "one call; ms per call (per_flow: F calls; cold: per call of 12 in turn)", "shapes": rows,
                "gates": gates})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
