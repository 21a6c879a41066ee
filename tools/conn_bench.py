#!/usr/bin/env python3
"""The connection table's two calls (wtp_flows_classify, wtp_flows_control) at the batch size of
the receive round, timed with device events, once from captured graphs and once back to back:

  state     16 384 connections in a table of 8192 buckets (mean load 2), nflows 20 480, window 4
  classify  64 Ki datagrams whose keys are drawn from the live connections, 1 in 16 from none
  control   the same ring three times over:
            "data"    no control datagram in the batch (the common round): what the call costs
                      when there is nothing to do
            "dups"    every datagram a START of a live connection with its seqNum (START_DUP,
                      64 Ki ACKs): the ranking and the ACK ring at their fullest, no state change
            "churn"   4096 ENDs of live connections and 4096 STARTs of new keys among DATA: the
                      table, the ring and 4096 windows change
  restore   "churn" changes the state, so its unit restores the table, the ring and the per-flow
            words first (device copies); that cost is timed alone as "restore" and reported
            beside it, not subtracted

Every variant is first checked on the device against tests/conn_model.py.  The host side of the
same work (a hash-map lookup per datagram and an upload) is not timed here.

Prints one JSON line and writes it to profiles/conn/conn_bench.json (--out).
  python tools/conn_bench.py [--reps 25] [--warmup 3] [--inner 10] [--out PATH]"""
import numpy as np
import torch

import bench_support as B  # first: it puts the binding's directory on sys.path
import conn_model as M
import wtp_crc32 as W
from bench_support import i32, stats, u32, z

N, NKEYS, NB, WINDOW, CHURN = 1 << 16, 1 << 14, 1 << 13, 4, 4096
NFLOWS = NKEYS + CHURN  # the ids of the connections that "churn" opens are free while all the others are live


def dev_bytes(a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # a copy: np.frombuffer gives a read-only array


def main():
    ap = B.parser()
    ap.add_argument("--inner", type=int, default=10)
    B.add_out(ap, "conn")
    a = ap.parse_args()
    res = B.start("conn_bench", a, min_reps=10)
    rng = np.random.default_rng(0xC0BE)
    keys = [M.key_of(j & 0xFFFF, 0x0A000000 + j * 7919) for j in range(NKEYS + CHURN)]
    live, fresh = keys[:NKEYS], keys[NKEYS:]
    # open all live connections on the device: one batch of STARTs from an empty table
    table = torch.full((W.conn_table_bytes(NB),), 0xFF, dtype=torch.uint8, device="cuda")
    st = M.State(NFLOWS, WINDOW, NB)
    st.slot_len[:] = M.EMPTY
    flow_start, seq0, slot_len = i32(st.flow_start), i32(st.seq0), i32(st.slot_len)
    free, free_pos = i32(st.free), i32(st.free_pos)
    out = dict(wire=z(N * 16, torch.uint8), src=z(N), opened=z(NFLOWS), osrc=z(NFLOWS), closed=z(NFLOWS), verdict=z(N), counts=z(6))
    work = torch.empty(W.conn_scratch_bytes(N, NFLOWS), dtype=torch.uint8, device="cuda")
    rl, ok = i32(np.full(N, 16)), torch.ones(N, dtype=torch.uint8, device="cuda")

    def control(ring, dkeys, flow, n):
        W.flows_control(ring, 16, rl, dkeys, 16, flow, ok, n, table, NB, NFLOWS, WINDOW, flow_start, seq0, slot_len, free,
                        free_pos, out["wire"], 16, N, out["src"], out["opened"], out["osrc"], out["closed"], out["verdict"],
                        out["counts"], work=work)

    def batch(items_keys, types, seqs):
        flow = z(len(items_keys))
        dkeys = dev_bytes(np.frombuffer(b"".join(items_keys), np.uint8))
        W.flows_classify(dkeys, 16, len(items_keys), table, NB, flow)
        return dev_bytes(M.header_ring(types, seqs)), dkeys, flow

    ring0 = M.header_ring(np.full(NKEYS, M.START), np.arange(NKEYS))
    want = M.control(st, ring0, 16, live, M.classify(st.table, live), np.ones(NKEYS, np.uint8), W.conn_bucket)
    control(*batch(live, np.full(NKEYS, M.START), np.arange(NKEYS)), NKEYS)
    torch.cuda.synchronize()
    if not (want["exact"] and u32(out["counts"]).tolist() == want["counts"].tolist()):
        raise SystemExit("conn_bench: opening the connections is not exact")
    st = want["state"]
    saved = [t.clone() for t in (table, flow_start, seq0, slot_len, free, free_pos)]

    def restore():
        for t, s in zip((table, flow_start, seq0, slot_len, free, free_pos), saved):
            t.copy_(s)

    pick = rng.integers(0, NKEYS, N)
    bkeys = [live[k] if i % 16 else M.key_of(i & 0xFFFF, 0x7F000001) for i, k in enumerate(pick)]
    h_flow = M.classify(st.table, bkeys)
    variants, rows = {}, {}
    # classify and the three control batches, each checked against the model first
    d_keys, d_flow = dev_bytes(np.frombuffer(b"".join(bkeys), np.uint8)), z(N)
    variants["classify"] = lambda: W.flows_classify(d_keys, 16, N, table, NB, d_flow)
    variants["classify"]()
    if not np.array_equal(u32(d_flow), h_flow):
        raise SystemExit("conn_bench: classify is not exact")
    variants["restore"] = restore
    seq_of = np.where(h_flow < NFLOWS, st.flow_start[np.minimum(h_flow, NFLOWS - 1)], 0)
    types = {"data": np.full(N, M.DATA), "dups": np.where(h_flow < NFLOWS, M.START, M.DATA)}
    churn_keys, churn_types, churn_seq = list(bkeys), np.full(N, M.DATA), seq_of.copy()
    at = rng.permutation(N)[:2 * CHURN]
    for j, i in enumerate(at[:CHURN]):  # ENDs of CHURN distinct live connections
        churn_keys[i], churn_types[i], churn_seq[i] = live[j * 4], M.END, st.flow_start[st.table[live[j * 4]]]
    for j, i in enumerate(at[CHURN:]):
        churn_keys[i], churn_types[i], churn_seq[i] = fresh[j], M.START, j
    cases = {"data": (bkeys, types["data"], seq_of), "dups": (bkeys, types["dups"], seq_of),
             "churn": (churn_keys, churn_types, churn_seq)}
    for name, (ks, ty, sq) in cases.items():
        restore()
        ring, dk, fl = batch(ks, ty, sq)
        want = M.control(st, M.header_ring(ty, sq), 16, ks, M.classify(st.table, ks), np.ones(N, np.uint8), W.conn_bucket)
        control(ring, dk, fl, N)
        torch.cuda.synchronize()
        exact = bool(want["exact"] and np.array_equal(u32(out["verdict"]), want["verdict"])
                     and u32(out["counts"]).tolist() == want["counts"].tolist()
                     and np.array_equal(u32(slot_len), want["state"].slot_len) and np.array_equal(u32(free_pos), want["state"].free_pos))
        if not exact:
            raise SystemExit(f"conn_bench: control ({name}) is not exact")
        rows[name] = {"counts": want["counts"].tolist()}
        if name == "churn":
            variants[name] = lambda ring=ring, dk=dk, fl=fl: (restore(), control(ring, dk, fl, N))
        else:
            variants[name] = lambda ring=ring, dk=dk, fl=fl: control(ring, dk, fl, N)
    restore()
    calls = {name: (fn, a.inner) for name, fn in variants.items()}
    for how in ("graph", "back_to_back"):
        t = B.sample(B.repeated(calls, how), a.reps, a.warmup, alternate=True)
        rows[how] = {"unit_ms": {name: stats(v) for name, v in t.items()}}
    res.update({"inner": a.inner, "n": N, "connections": NKEYS, "nbuckets": NB, "nflows": NFLOWS, "window": WINDOW,
                "unit": "one call over 64 Ki datagrams (churn: restore + call); ms per unit", "cases": rows})
    B.write_result(res, a.out)


if __name__ == "__main__":
    main()
