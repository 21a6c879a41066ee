#!/usr/bin/env python3
"""What the protocol entry points answer before any device is touched, recorded from one
build of the library so that a change to their host code can be compared against it.

    WTP_LIB=/path/to/libwtp_crc32.so python tests/golden/make_abi_refusals.py
Output: tests/golden/abi_refusals.json (data only).  tests/test_abi_refusals.py runs the
same cases against the current library and compares.

For each of the 15 `int` calls of the protocol translation units: a baseline argument list
that would be valid (host addresses that are never dereferenced), every single violation
that include/wtp_crc32.h documents, and every ordered pair of two violations (the second's
arguments are applied after the first's; two violations that set one argument to different
values, or that are valid together, make no pair).  Recorded: the return code and
wtp_last_error().  Which message two bad arguments give is part of the C-ABI.  Also the
documented shapes that return WTP_OK without a launch.  No case here reaches a launch:
cases() refuses to produce one whose answer is neither WTP_EINVAL nor such a WTP_OK.

For the *_work_bytes functions: their value over a grid of arguments (0, 1, around the
block sizes 256 and 1024, every documented limit and one past it, both ACK modes).
"""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "a3-reliable-transport_amd"))

EINVAL, P = -1, 1456
MAXI, MAXW, MAXB, MAXF, MAXS = 1 << 20, 1 << 20, 1 << 24, 1 << 20, 1 << 24
GRID = [0, 1, 255, 256, 257, 1023, 1024, 1025]

_buf = C.create_string_buffer(1 << 20)
A = (C.addressof(_buf) + 15) & ~15  # arrays below are 64 KiB apart: no two overlap


def ptr(k):
    return A + (k << 16)


def nulls(*names):
    return {f"null {n}": {n: None} for n in names}


def calls(L):
    """{call: (baseline arguments in order, {violation: overrides}, {no-op: overrides}, pairs that are valid)}"""
    out = {}
    out["wtp_accept_data_packets"] = (
        dict(d_dgrams=ptr(0), stride=1472, d_recv_len=ptr(1), n=4, seq0=7, window=8, d_out=ptr(2), d_slot_len=ptr(3),
             d_ok=ptr(4), d_place=ptr(5), d_ack=ptr(6), stream=None),
        {"n 2^31": dict(n=1 << 31), "stride": dict(stride=15), "n 0, null d_slot_len": dict(n=0, d_slot_len=None),
         **nulls("d_dgrams", "d_recv_len", "d_ok", "d_out", "d_slot_len")},
        {"n 0, no d_ack": dict(n=0, d_ack=None), "nothing": dict(n=0, d_ack=None, d_dgrams=None, d_slot_len=None)}, ())
    out["wtp_crc32_concat"] = (
        dict(d_crc=ptr(0), d_len=None, len=P, last_len=100, n=4, d_work=ptr(1), work_bytes=L.wtp_crc32_concat_work_bytes(4),
             d_out=ptr(2), stream=None),
        {"work_bytes": dict(work_bytes=L.wtp_crc32_concat_work_bytes(4) - 1), **nulls("d_out", "d_crc", "d_work")}, {}, ())
    out["wtp_crc32_buffer"] = (
        dict(d_buf=ptr(0), nbytes=5000, d_work=ptr(1), work_bytes=L.wtp_crc32_buffer_work_bytes(5000), d_out=ptr(2),
             stream=None),
        {"work_bytes": dict(work_bytes=L.wtp_crc32_buffer_work_bytes(5000) - 1), **nulls("d_out", "d_buf", "d_work")}, {}, ())
    out["wtp_tx_ingest_acks"] = (
        dict(d_dgrams=ptr(0), stride=16, d_recv_len=ptr(1), n=4, mode=0, seq0=7, inflight=8, d_acked=ptr(2), d_ok=ptr(3),
             d_hit=ptr(4), d_counts=ptr(5), stream=None),
        {"n 2^31": dict(n=1 << 31), "inflight": dict(inflight=MAXI + 1), "mode": dict(mode=2), "stride": dict(stride=15),
         **nulls("d_counts", "d_acked", "d_dgrams", "d_recv_len", "d_ok")}, {}, ())
    need = L.wtp_tx_work_bytes(8, 4)
    sel = dict(seq0=7, inflight=8, d_acked=ptr(1), d_sent_ms=ptr(2), now_ms=1000, timeout_ms=50, flags=0, d_wire=ptr(3),
               wire_stride=1472, max_sel=4, d_sel=ptr(4), d_wire_len=ptr(5))
    tail = dict(d_counts=ptr(6), d_work=ptr(7), work_bytes=need, stream=None)
    bad = {"wire_stride": dict(wire_stride=1471), "inflight": dict(inflight=MAXI + 1), "work_bytes": dict(work_bytes=need - 1),
           **nulls("d_counts", "d_work", "d_acked", "d_sent_ms", "d_wire")}
    out["wtp_tx_build_retransmit"] = (
        dict(d_payloads=ptr(0), total_bytes=8 * P, **sel, **tail),
        {**bad, "total_bytes": dict(total_bytes=7 * P), **nulls("d_payloads")}, {}, ())
    out["wtp_tx_build_retransmit_var"] = (
        dict(d_base=ptr(0), base_bytes=8 * P, d_offsets=ptr(8), d_lengths=ptr(9), **sel, d_crc_out=ptr(10), **tail),
        {**bad, **nulls("d_base", "d_offsets", "d_lengths")}, {}, ())
    need = L.wtp_rx_ack_work_bytes(4, 8, 1)
    out["wtp_rx_build_acks"] = (
        dict(d_dgrams=ptr(0), stride=1472, d_recv_len=ptr(1), n=4, mode=1, seq0=7, window=8, d_ok=ptr(2), d_place=ptr(3),
             d_slot_len=ptr(4), d_ack_wire=ptr(5), ack_stride=16, skip=0, max_acks=4, d_src=ptr(6), d_counts=ptr(7),
             d_work=ptr(8), work_bytes=need, stream=None),
        {"n": dict(n=MAXB + 1), "mode": dict(mode=2), "window": dict(window=MAXW + 1), "stride": dict(stride=15),
         "ack_stride": dict(ack_stride=15), "work_bytes": dict(work_bytes=need - 1),
         **nulls("d_counts", "d_work", "d_dgrams", "d_recv_len", "d_ok", "d_place", "d_slot_len", "d_ack_wire")}, {}, ())
    out["wtp_build_data_packets_var"] = (
        dict(d_base=ptr(0), base_bytes=8 * P, d_offsets=ptr(1), d_lengths=ptr(2), n=4, seq0=7, d_wire=ptr(3), wire_stride=1472,
             d_wire_len=ptr(4), d_crc_out=ptr(5), stream=None),
        {"wire_stride": dict(wire_stride=1471), "n 2^31": dict(n=1 << 31), **nulls("d_base", "d_offsets", "d_lengths", "d_wire")},
        {"n 0": dict(n=0), "nothing": dict(n=0, d_base=None, d_offsets=None, d_lengths=None, d_wire=None)}, ())
    need = L.wtp_rx_deliver_work_bytes(8)
    out["wtp_rx_deliver"] = (
        dict(d_img=ptr(0), d_slot_len=ptr(1), window=8, max_slots=8, d_stream=ptr(2), stream_bytes=4096, stream_off=0,
             d_offsets_out=ptr(3), d_lengths_out=ptr(4), d_counts=ptr(5), d_work=ptr(6), work_bytes=need, stream=None),
        {"window": dict(window=MAXW + 1), "stream_off": dict(stream_off=4097), "work_bytes": dict(work_bytes=need - 1),
         **nulls("d_counts", "d_work", "d_img", "d_slot_len", "d_stream")}, {}, ())
    out["wtp_rx_advance"] = (
        dict(d_img=ptr(0), d_slot_len=ptr(1), window=8, d_adv=ptr(2), d_img_next=ptr(3), d_slot_len_next=ptr(4), stream=None),
        {"window": dict(window=MAXW + 1), "d_slot_len overlap": dict(d_slot_len_next=ptr(1) + 4),
         "d_img overlap": dict(d_img_next=ptr(0) + 1),
         **nulls("d_img", "d_img_next", "d_adv", "d_slot_len", "d_slot_len_next")},
        {"window 0": dict(window=0), "nothing": dict(window=0, d_img=None, d_slot_len=None, d_adv=None, d_img_next=None,
                                                      d_slot_len_next=None)},
        [("null d_img", "null d_img_next")])
    out["wtp_tx_advance"] = (
        dict(d_acked=ptr(0), d_sent_ms=ptr(1), slots=8, d_adv=ptr(2), fill_ms=9, d_acked_next=ptr(3), d_sent_ms_next=ptr(4),
             stream=None),
        {"slots": dict(slots=MAXI + 1), "acked_next over acked": dict(d_acked_next=ptr(0) + 4),
         "acked_next over sent_ms": dict(d_acked_next=ptr(1) + 4), "sent_ms_next over acked": dict(d_sent_ms_next=ptr(0) + 4),
         "sent_ms_next over sent_ms": dict(d_sent_ms_next=ptr(1) + 4), "sent_ms_next over acked_next": dict(d_sent_ms_next=ptr(3) + 4),
         **nulls("d_adv", "d_acked", "d_sent_ms", "d_acked_next", "d_sent_ms_next")},
        {"slots 0": dict(slots=0), "nothing": dict(slots=0, d_acked=None, d_sent_ms=None, d_adv=None, d_acked_next=None,
                                                    d_sent_ms_next=None)}, ())
    limits = {"nflows": dict(nflows=MAXF + 1), "window": dict(window=MAXW + 1), "slots": dict(nflows=(1 << 12) + 1, window=1 << 12)}
    out["wtp_accept_data_packets_flows"] = (
        dict(d_dgrams=ptr(0), stride=1472, d_recv_len=ptr(1), d_flow=ptr(2), n=4, d_seq0=ptr(3), nflows=3, window=5,
             d_out=ptr(4), d_slot_len=ptr(5), d_ok=ptr(6), d_place=ptr(7), d_ack=ptr(8), stream=None),
        {"n 2^31": dict(n=1 << 31), "stride": dict(stride=15), **limits, "n 0, null d_slot_len": dict(n=0, d_slot_len=None),
         "n 0, null d_seq0": dict(n=0, d_seq0=None),
         **nulls("d_dgrams", "d_recv_len", "d_flow", "d_ok", "d_out", "d_slot_len", "d_seq0")},
        {"n 0, no d_ack": dict(n=0, d_ack=None), "n 0, no flows": dict(n=0, nflows=0)}, ())
    need = L.wtp_rx_ack_flows_work_bytes(4)
    out["wtp_rx_build_acks_flows"] = (
        dict(d_dgrams=ptr(0), stride=1472, d_recv_len=ptr(1), d_flow=ptr(2), n=4, mode=1, d_seq0=ptr(3), nflows=3, window=5,
             d_ok=ptr(4), d_flow_ack=ptr(5), d_ack_wire=ptr(6), ack_stride=16, skip=0, max_acks=4, d_src=ptr(7),
             d_counts=ptr(8), d_work=ptr(9), work_bytes=need, stream=None),
        {"n": dict(n=MAXB + 1), "mode": dict(mode=2), "window": dict(window=MAXW + 1), "stride": dict(stride=15),
         "ack_stride": dict(ack_stride=15), "work_bytes": dict(work_bytes=need - 1),
         **nulls("d_counts", "d_work", "d_dgrams", "d_recv_len", "d_ok", "d_flow", "d_seq0", "d_flow_ack", "d_ack_wire")}, {}, ())
    need = L.wtp_rx_deliver_flows_work_bytes(3, 5)
    out["wtp_rx_deliver_flows"] = (
        dict(d_img=ptr(0), d_slot_len=ptr(1), nflows=3, window=5, max_slots=5, d_stream=ptr(2), stream_bytes=4096, stream_off=0,
             d_offsets_out=ptr(3), d_lengths_out=ptr(4), d_flow_adv=ptr(5), d_flow_info=ptr(6), d_counts=ptr(7), d_work=ptr(8),
             work_bytes=need, stream=None),
        {**limits, "slots, product past 2^32": dict(nflows=1 << 20, window=1 << 20), "stream_off": dict(stream_off=4097),
         "work_bytes": dict(work_bytes=need - 1),
         **nulls("d_counts", "d_work", "d_flow_adv", "d_img", "d_slot_len", "d_stream")}, {}, ())
    out["wtp_rx_advance_flows"] = (
        dict(d_img=ptr(0), d_slot_len=ptr(1), nflows=3, window=5, d_flow_adv=ptr(2), d_seq0=ptr(3), d_img_next=ptr(4),
             d_slot_len_next=ptr(5), d_seq0_next=ptr(6), stream=None),
        {**limits, "d_slot_len overlap": dict(d_slot_len_next=ptr(1) + 4), "d_img overlap": dict(d_img_next=ptr(0) + 1),
         "d_seq0 overlap": dict(d_seq0_next=ptr(3) + 4),
         **nulls("d_img", "d_img_next", "d_seq0", "d_seq0_next", "d_flow_adv", "d_slot_len", "d_slot_len_next")},
        {"no flows": dict(nflows=0), "window 0": dict(window=0),
         "nothing": dict(nflows=0, window=0, d_img=None, d_slot_len=None, d_flow_adv=None, d_seq0=None, d_img_next=None,
                         d_slot_len_next=None, d_seq0_next=None)},
        [("null d_img", "null d_img_next"), ("null d_seq0", "null d_seq0_next")])
    return out


def work_grids():
    g = GRID
    return {
        "wtp_tx_work_bytes": itertools.product(g + [MAXI, MAXI + 1], g + [MAXI, MAXI + 1]),
        "wtp_rx_ack_work_bytes": itertools.product(g + [MAXB, MAXB + 1], g + [MAXW, MAXW + 1], [0, 1]),
        "wtp_rx_ack_flows_work_bytes": ((n,) for n in g + [MAXB, MAXB + 1]),
        "wtp_rx_deliver_work_bytes": ((w,) for w in g + [MAXW, MAXW + 1]),
        "wtp_rx_deliver_flows_work_bytes": itertools.product(g + [1 << 12, (1 << 12) + 1, MAXF, MAXF + 1],
                                                             g + [1 << 12, (1 << 12) + 1, MAXW, MAXW + 1]),
        "wtp_crc32_concat_work_bytes": ((n,) for n in g + [MAXB, MAXB + 1]),
        "wtp_crc32_buffer_work_bytes": ((n,) for n in g + [P - 1, P, P + 1, 1 << 30, (1 << 30) + 1]),
    }


def cases(L):
    """{"refusals": {call: {case: [rc, message]}}, "work_bytes": {function: {"a,b": value}}}"""
    ref = {}
    for name, (base, bad, noop, valid_pairs) in calls(L).items():
        f = getattr(L, name)
        valid = {frozenset(p) for p in valid_pairs}

        def run(over, want):
            rc = f(*{**base, **over}.values())
            if rc != want:
                raise SystemExit(f"{name} {over}: returned {rc}, expected {want}: not a case for this file")
            return [rc, L.wtp_last_error().decode() if rc else ""]

        got = {v: run(over, EINVAL) for v, over in bad.items()}
        for a, b in itertools.permutations(bad, 2):
            if frozenset((a, b)) in valid or any(k in bad[b] and bad[b][k] != v for k, v in bad[a].items()):
                continue
            got[f"{a} + {b}"] = run({**bad[a], **bad[b]}, EINVAL)
        got.update({f"ok: {v}": run(over, 0) for v, over in noop.items()})
        ref[name] = got
    work = {name: {",".join(map(str, a)): int(getattr(L, name)(*a)) for a in grid} for name, grid in work_grids().items()}
    return {"refusals": ref, "work_bytes": work}


def render(doc) -> str:
    """One case per line, so that a difference reads as the cases that changed."""
    lines = ["{"]
    for si, (section, body) in enumerate(doc.items()):
        lines.append(f" {json.dumps(section)}: {{")
        for ci, (call, rows) in enumerate(body.items()):
            lines.append(f"  {json.dumps(call)}: {{")
            items = list(rows.items())
            lines += [f"   {json.dumps(k)}: {json.dumps(v)}" + ("," if i + 1 < len(items) else "") for i, (k, v) in enumerate(items)]
            lines.append("  }" + ("," if ci + 1 < len(body) else ""))
        lines.append(" }" + ("," if si + 1 < len(doc) else ""))
    return "\n".join(lines + ["}"]) + "\n"


if __name__ == "__main__":
    import wtp_crc32 as W  # the library that WTP_LIB names, else the tree's
    text = render(cases(W.LIB))
    assert json.loads(text)
    with open(os.path.join(HERE, "abi_refusals.json"), "w") as fh:
        fh.write(text)
    print(f"{W.LIB_PATH}: {text.count(chr(10))} lines")
