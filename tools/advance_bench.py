#!/usr/bin/env python3
"""The receive window's slide (wtp_rx_advance) against what a caller could do before it
existed, in one process, in turn per repetition, timed with device events:

  (a)  the new call, the advance read from device memory
  (b)  torch on the device with the advance k already on the host (the favourable case for
       this route): copy_ of slot_len[k:] with a fill of the tail, and a contiguous copy_ of
       img[k * 1456:] into the second image, filled or not
  (b') route (b) with the .item() read of k inside the timed region
  (c)  torch's contiguous device-to-device copy of exactly the bytes (a) moves: the window's
       lengths and the filled bytes of the slots that stay (a floor: one contiguous range)
  (v)  the new call followed by wtp_accept_data_packets of the next round's batch into the
       window it wrote (the figure the kernel's store policy is chosen by)

Configurations: S1 = 2^20 slots moved by 300 000, S2 = 65 536 by 20 000 (the slots that leave
are the delivered run, the slot behind them is the hole, and 1 % of the slots behind the hole
hold Zipf(1.1) records, the rest are empty); Z = 2^20 Zipf(1.1) slots moved by 1; D = 2^20
slots of 1456 B moved by 1.  Every configuration is checked exact first: (a) against an
image and state computed on the device without the call, (b) against (a) where the two agree
by definition (the state; the image over each slot's stored length).

Prints one JSON line and writes it to profiles/advance/advance_bench.json (--out).
Acceptance: a < b at S1 and S2 by more than the sum of both interquartile ranges.
  python tools/advance_bench.py [--reps 25] [--warmup 3] [--configs S1,S2,Z,D] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's and the oracle's directories on sys.path
import oracle as O
import wtp_crc32 as W
from bench_support import iqr, stats

STRIDE, MAXP, EMPTY, SEQ0 = 1472, 1456, 0xFFFFFFFF, 0xFFFFF000
CONFIGS = {"S1": (1 << 20, 300000, "sparse"), "S2": (1 << 16, 20000, "sparse"), "Z": (1 << 20, 1, "zipf"),
           "D": (1 << 20, 1, "full")}
GATED = ("S1", "S2")
NEXT_BATCH = 65536  # datagrams of the next round's accept in route (v)


def lengths(w, a, kind):
    if kind == "full":
        return np.full(w, MAXP, dtype=np.uint32)
    lens = O.zipf_lengths(w).astype(np.uint32)
    if kind == "sparse":
        rng = np.random.default_rng(w + a)
        behind = np.arange(w) > a
        lens[behind & (rng.random(w) >= 0.01)] = EMPTY
        lens[a] = EMPTY  # the hole that ended the delivered run
    return lens


def expected(img, lens, a, w, fill):
    """The second image after the call, from the first one and the host's lengths, without it."""
    v = np.full(w, EMPTY, np.int64)
    v[:w - a] = lens[a:]
    vt = torch.from_numpy(np.where(v <= MAXP, v, 0)).cuda()
    want = torch.full((w, MAXP), fill, dtype=torch.uint8, device="cuda")
    want[:w - a] = img.view(w, MAXP)[a:]
    want.masked_fill_(~(torch.arange(MAXP, device="cuda")[None, :] < vt[:, None]), fill)
    return want.view(-1), v


def case(name, reps, warmup):
    w, a, kind = CONFIGS[name]
    lens = lengths(w, a, kind)
    img = torch.empty(w * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(img, seed=0xAD7)
    sl = torch.from_numpy(lens.view(np.int32)).cuda()
    adv = torch.tensor([a, 0, 0, 0], dtype=torch.int64, device="cuda")  # as rx_deliver's d_counts
    img2 = torch.empty(w * MAXP, dtype=torch.uint8, device="cuda")
    sl2 = torch.empty(w, dtype=torch.int32, device="cuda")
    img_b = torch.empty(w * MAXP, dtype=torch.uint8, device="cuda")
    sl_b = torch.empty(w, dtype=torch.int32, device="cuda")

    def a_new():
        W.rx_advance(img, sl, w, adv, img2, sl2)

    def b_torch(k=a):
        sl_b[:w - k].copy_(sl[k:])
        sl_b[w - k:].fill_(-1)
        img_b[:(w - k) * MAXP].copy_(img[k * MAXP:])

    def b_read():
        b_torch(int(adv[0].item()))

    # exactness, before anything is timed
    img2.fill_(0x3C)
    sl2.fill_(12345)
    a_new()
    torch.cuda.synchronize()
    kernel = W.LIB.wtp_last_kernel().decode()
    want, v = expected(img, lens, a, w, 0x3C)
    exact = torch.equal(img2, want) and np.array_equal(sl2.cpu().numpy().view(np.uint32), v.astype(np.uint32))
    del want
    img_b.fill_(0x3C)
    b_read()
    torch.cuda.synchronize()
    exact = exact and torch.equal(sl_b, sl2)
    keep = torch.arange(MAXP, device="cuda")[None, :] < torch.from_numpy(np.where(v <= MAXP, v, 0)).cuda()[:, None]
    exact = exact and torch.equal(img_b.view(w, MAXP).masked_fill(~keep, 0), img2.view(w, MAXP).masked_fill(~keep, 0))
    del keep
    moved = int(v[v <= MAXP].sum())

    # (c): one contiguous range of the bytes (a) moves
    c_bytes = moved + 4 * w
    c_src = torch.empty(c_bytes, dtype=torch.uint8, device="cuda")
    W.synth_fill(c_src, seed=1)
    c_dst = torch.empty(c_bytes, dtype=torch.uint8, device="cuda")

    def c_copy():
        c_dst.copy_(c_src)

    # (v): the next round's batch, full datagrams for the last NEXT_BATCH slots of the new window (empty in S1, S2;
    # filled in Z and D, where accept verifies and places nothing: the advance's stores are what differs)
    nb = min(NEXT_BATCH, w // 2)
    pay = torch.empty(nb * MAXP, dtype=torch.uint8, device="cuda")
    W.synth_fill(pay, seed=2)
    ring = torch.empty(nb * STRIDE, dtype=torch.uint8, device="cuda")
    wl = torch.empty(nb, dtype=torch.int32, device="cuda")
    W.build_data_packets(pay, nb * MAXP, (SEQ0 + w - nb) & 0xFFFFFFFF, ring, STRIDE, wl)
    ok = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def v_next():
        a_new()
        W.accept_data_packets(ring, STRIDE, wl, nb, SEQ0, w, img2, sl2, ok)

    c_copy()
    v_next()
    torch.cuda.synchronize()
    exact = exact and torch.equal(c_dst, c_src) and bool((ok == 1).all())
    if not exact:
        raise SystemExit(f"advance_bench: {name}: outputs are not exact")
    t = B.sample({k: (fn, None, 1) for k, fn in zip("abrcv", (a_new, b_torch, b_read, c_copy, v_next))}, reps, warmup)
    ma, mb, mr, mc, mv = (float(np.median(t[k])) for k in "abrcv")
    traffic = 8 * w + 2 * moved  # per slot 4 B read + 4 B written, + 2 v for a valid slot
    return {"config": name, "window": w, "advance": a, "contents": kind, "filled_slots_moved": int((v <= MAXP).sum()),
            "bytes_moved": moved, "exact": exact, "kernel": kernel, "a_advance_ms": round(ma, 4),
            "b_torch_k_on_host_ms": round(mb, 4), "b_read_k_ms": round(mr, 4), "c_copy_ms": round(mc, 4),
            "v_advance_then_accept_ms": round(mv, 4), "a_over_b": round(ma / mb, 4), "a_over_c": round(ma / mc, 4),
            "a_stats": stats(t["a"]), "b_stats": stats(t["b"]), "b_read_stats": stats(t["r"]), "c_stats": stats(t["c"]),
            "v_stats": stats(t["v"]), "a_iqr_ms": round(iqr(t["a"]), 4), "b_iqr_ms": round(iqr(t["b"]), 4),
            "a_below_b_by_more_than_both_iqr": B.below_by_more_than_both_iqr(t["a"], t["b"]), "gated": name in GATED,
            "b_bytes_copied": (w - a) * (MAXP + 4) + 4 * a, "a_model_traffic_bytes": traffic,
            "a_model_traffic_gbps": round(traffic / (ma * 1e-3) / 1e9, 1)}


def main():
    ap = B.parser()
    ap.add_argument("--configs", default="S1,S2,Z,D")
    B.add_out(ap, "advance")
    a = ap.parse_args()
    res = B.start("advance_bench", a, min_reps=20)
    cases = [case(c, a.reps, a.warmup) for c in a.configs.split(",")]
    res.update({"accepted": all(c["a_below_b_by_more_than_both_iqr"] for c in cases if c["gated"]), "cases": cases})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
