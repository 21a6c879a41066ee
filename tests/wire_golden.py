"""tests/golden/wire.json as the wire tests use it (tests/test_wire_reference.py on the CPU,
tests/test_gpu_wire.py on the device): what the reference's own Packet and Window code
produced, recorded by tests/golden/make_wire_golden.py.  The file is only read, once, and
payload bytes are regenerated from each record's start_byte."""
import functools
import json
import os

import oracle as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wire.json")


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def payload(start_byte, length):
    return O.synth_fill_np(length, start_byte=start_byte, seed=load()["seed"]).tobytes()


@functools.lru_cache(maxsize=None)
def corpus():
    """{(type word, seqNum, payload length): (start_byte, the reference's 16 header bytes)}."""
    return {(t, s, total - 16): (sb, bytes.fromhex(hdr)) for t, s, sb, total, hdr in load()["datagrams"]}


def datagram(ptype, seq, length):
    """The reference's datagram for one corpus entry: recorded header, regenerated payload."""
    sb, hdr = corpus()[ptype, seq, length]
    return hdr + payload(sb, length)
