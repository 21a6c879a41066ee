#!/usr/bin/env python3
"""Generate tests/golden/wire.json from the REFERENCE's own Packet and Window code.

Run in the build container (needs the reference tree and `make -C oracle all`):
    python tests/golden/make_wire_golden.py

Every header byte, parse result and window verdict below is produced by calling the
reference's cpp/src/base/Packet.cpp, cpp/src/opt/Packet.cpp and cpp/src/opt/Window.cpp,
compiled from where they lie into oracle/_ref/libref_packet_{base,opt}.so through
oracle/ref_packet_shim.cpp.  Nothing here is computed by a restatement (oracle.build_datagram,
tests/retx_model.py, tests/ack_model.py), so those and the kernels are pinned by this file
rather than by each other.  The only project code used is oracle.synth_fill_np, for the
payload bytes, which are input and are never stored: a record keeps their start_byte.

Output (data only): wire.json
  datagrams  type words x seqNums x payload lengths as the reference serialises them
             (Packet(type, data, seq) + getNetworkOrderHeader(), base == opt asserted):
             rows [type, seqNum, start_byte, total length, 16 header bytes as hex]
  parse      Packet(buf, size) of a subset, and of headers whose length field disagrees
             with the buffer: rows [header hex, start_byte, size, type, seqNum, length,
             checksum, calculateCheckSum()]
  window     opt Window traces: (seq0, inflight, ACK seqNums) -> (acked flags, advance)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import oracle as O  # noqa: E402

M32 = 0xFFFFFFFF
TYPES = [0, 1, 2, 3, 7, 0x00000102, 0x00010002, 0x01000002, 0x02000000, 0x00000200, 0x80000002, 0xFFFFFF02, 0x02020202,
         0x00000103, 0x03000000, 0x80000003, 0x03030303]
SEQS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
LENS = [0, 1, 15, 16, 17, 1455, 1456]
PARSE_TYPES = [2, 3, 0x00000102, 0x02000000, 0x80000003]
PARSE_LENS = [0, 17, 1456]
WRONG_LENGTHS = ("0", "len+1", "1457")  # the shim hands the reference no length field above 65536


def start_byte(ti, si, li):
    return 4096 * (si * len(LENS) + li) + 64 * ti


def payload(sb, ln):
    return O.synth_fill_np(ln, start_byte=sb).tobytes()


class Mix:
    """splitmix64 as a seeded stream: the traces must not depend on a library's generator."""

    def __init__(self, seed):
        self.s = seed

    def next(self, bound):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return (z ^ (z >> 31)) % bound

    def shuffle(self, items):
        items = list(items)
        for i in range(len(items) - 1, 0, -1):
            j = self.next(i + 1)
            items[i], items[j] = items[j], items[i]
        return items


def window_acks(mix, seq0, inflight, kind):
    """The ACK seqNums of one trace: in-window ones by `kind` ("gap": never slot 0, so the
    advance is 0 for inflight > 1; "lead": a leading run and scattered slots; "full": every
    slot), two of them twice more, three below the window and three at or above its end."""
    slots = list(range(inflight))
    if kind == "gap" and inflight > 1:
        inwin = [s for s in slots[1:] if mix.next(3) != 0] or [inflight - 1]
    elif kind == "lead" and inflight > 1:
        inwin = slots[:1 + inflight // 3] + [s for s in slots[2 + inflight // 3:] if mix.next(4) == 0]
    else:
        inwin = slots
    dup = [inwin[mix.next(len(inwin))], inwin[0], inwin[-1]]
    below = [-1, -50, 0x80000000]
    above = [inflight, inflight + 1, inflight + 49]
    return [(seq0 + s) & M32 for s in mix.shuffle(inwin + dup + below + above)]


def main():
    base, opt = O.ref_packet_lib("base"), O.ref_packet_lib("opt")
    if base is None or opt is None:
        sys.exit("oracle/_ref/libref_packet_{base,opt}.so missing: run `make -C oracle all` in the build container")
    g = {"generator": "tests/golden/make_wire_golden.py",
         "source": "reference cpp/src/base/Packet.cpp, cpp/src/opt/Packet.cpp, cpp/src/opt/Window.cpp via oracle/_ref",
         "seed": O.SEED, "payload_rule": "payload = oracle.synth_fill_np(total - 16, start_byte), seed 0x5EED",
         "types": TYPES, "seqs": SEQS, "lens": LENS}

    rows, made = [], {}
    for ti, t in enumerate(TYPES):
        for si, s in enumerate(SEQS):
            for li, ln in enumerate(LENS):
                sb = start_byte(ti, si, li)
                d = O.ref_build_datagram(base, t, s, payload(sb, ln))
                assert d == O.ref_build_datagram(opt, t, s, payload(sb, ln)), "base and opt serialise differently"
                assert len(d) == 16 + ln and d[16:] == payload(sb, ln)
                rows.append([t, s, sb, len(d), d[:16].hex()])
                made[t, s, ln] = (sb, d)
    g["datagrams"] = rows

    parse = []

    def record(d, sb):
        out = O.ref_parse_datagram(base, d)
        assert out == O.ref_parse_datagram(opt, d), "base and opt parse differently"
        parse.append([d[:16].hex(), sb, len(d)] + out)

    for t in PARSE_TYPES:
        for s in SEQS:
            for ln in PARSE_LENS:
                sb, d = made[t, s, ln]
                record(d, sb)
    for k, (t, s, ln) in enumerate([(2, 0, 0), (2, 1, 17), (2, 0x80000000, 1455), (2, 0xFFFFFFFF, 1456), (3, 0x7FFFFFFF, 0),
                                    (3, 1, 16)]):
        sb, d = made[t, s, ln]
        for wrong in (0, ln + 1, 1457):
            if wrong != ln:
                record(d[:8] + wrong.to_bytes(4, "big") + d[12:], sb)
    g["parse"] = {"wrong_lengths": list(WRONG_LENGTHS),
                  "note": "calculateCheckSum() covers header.length bytes, zero-padded past the buffer's end",
                  "records": parse}

    traces = []
    for seq0 in (0, 0xFFFFFFF0):
        for inflight in (1, 10, 64):
            for kind in ("gap", "lead", "full"):
                mix = Mix(O.SEED + seq0 % 251 + 7 * inflight + len(kind))
                acks = window_acks(mix, seq0, inflight, kind)
                flags, adv = O.ref_window_run(opt, seq0, inflight, acks)
                traces.append({"kind": kind, "seq0": seq0, "inflight": inflight, "acks": acks,
                               "acked": "".join(str(int(f)) for f in flags), "advance": adv})
    g["window"] = traces

    head = {k: v for k, v in g.items() if k not in ("datagrams", "parse", "window")}
    with open(os.path.join(HERE, "wire.json"), "w") as f:  # one record per line
        f.write("{\n")
        for k, v in head.items():
            f.write(f" {json.dumps(k)}: {json.dumps(v)},\n")
        f.write(' "datagrams": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ],\n")
        f.write(f' "parse": {{"wrong_lengths": {json.dumps(g["parse"]["wrong_lengths"])}, "note": {json.dumps(g["parse"]["note"])},\n')
        f.write('  "records": [\n' + ",\n".join("   " + json.dumps(r) for r in parse) + "\n  ]},\n")
        f.write(' "window": [\n' + ",\n".join("  " + json.dumps(t) for t in traces) + "\n ]\n}\n")
    print("wrote", os.path.join(HERE, "wire.json"), len(rows), "datagrams,", len(parse), "parse records,", len(traces), "traces")


if __name__ == "__main__":
    main()
