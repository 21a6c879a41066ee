"""Sequential model of wtp_accept_data_packets (include/wtp_crc32.h): the arrival-order
loop of the reference's receiver (cpp/src/base/Receiver.cpp:25-35, :208-237) over a
window the caller owns.  ok comes from oracle.verify_datagrams, pinned to the reference."""
import numpy as np

import oracle as O

MAXP = 1456
EMPTY = 0xFFFFFFFF
NOT_PLACED = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def accept(ring, stride, recv_len, seq0, window, out, slot_len):
    """Returns (ok, place, out, slot_len, ack); `out` / `slot_len` are the window state on
    entry (not modified: copies are returned)."""
    ring = np.ascontiguousarray(ring, dtype=np.uint8)
    recv_len = np.ascontiguousarray(recv_len, dtype=np.uint32)
    n = recv_len.size
    out, slot_len = out.copy(), slot_len.copy()
    ok = O.verify_datagrams(ring, stride, recv_len)[0] if n else np.zeros(0, np.uint8)
    place = np.full(n, NOT_PLACED, dtype=np.uint32)
    for i in range(n):
        if not ok[i]:
            continue
        d = ring[i * stride:i * stride + int(recv_len[i])]
        ln = d.size - 16
        s = (int.from_bytes(d[4:8].tobytes(), "big") - seq0) & M32
        if int.from_bytes(d[0:4].tobytes(), "big") != 2 or ln > MAXP or s >= window or slot_len[s] != EMPTY:
            continue
        out[s * MAXP:s * MAXP + ln] = d[16:]
        slot_len[s] = ln
        place[i] = s
    lead = 0
    while lead < window and slot_len[lead] != EMPTY:
        lead += 1
    return ok, place, out, slot_len, (seq0 + lead) & M32


# ---- the corpus of the randomised differential test -------------------------------------------
FUZZ_SEEDS = range(12)
FUZZ_BASE = 0xACCE02  # chosen so that test_accept_model.py's conditions on the corpus hold
FUZZ_STRIDES = (1472, 1504, 1500, 1480, 1488)
# what every batch of at least 8 datagrams contains; "long" (a payload of 1457 .. stride - 16
# bytes) only where the stride holds one
FUZZ_KINDS = ("placeable", "dup_batch", "dup_filled", "below", "at_end", "above", "far", "type0", "type1", "type3",
              "type7", "zero", "long", "runt", "over_stride", "flip_payload", "flip_crc")


def fuzz_kinds(stride):
    return [k for k in FUZZ_KINDS if k != "long" or stride - 16 > MAXP]


def fuzz_case(seed):
    """(rng, window, seq0, stride, ring_off, out_off, ns) of one seed: three successive calls
    of ns[k] datagrams on one window.  seq0 is uniform for an even seed and within 768 of the
    2^32 wrap for an odd one; seed 5 makes its middle call with n == 0, seed 2 its first with
    the smallest batch."""
    rng = np.random.default_rng(FUZZ_BASE + seed)
    window = int(rng.integers(1, 701))
    seq0 = int(rng.integers(0xFFFFFD00, 1 << 32)) if seed % 2 else int(rng.integers(0, 1 << 32))
    stride = FUZZ_STRIDES[seed % len(FUZZ_STRIDES)]  # every stride at least twice
    ring_off = (0, 0, 0, 1, 8)[int(rng.integers(5))]
    out_off = (0, 0, 4)[int(rng.integers(3))]
    ns = [int(x) for x in rng.integers(8, 601, 3)]
    if seed == 5:
        ns[1] = 0
    if seed == 2:
        ns[0] = 8
    return rng, window, seq0, stride, ring_off, out_off, ns


def fuzz_batch(rng, seq0, window, stride, state, n=None):
    """(ring, recv_len, kinds) of one random batch for a window whose slot_len on entry is
    `state`; n in [8, 600] unless given.  kinds[i] is the set of FUZZ_KINDS that datagram i
    was made for: every kind of fuzz_kinds(stride) is dealt to a datagram of its own while n
    allows it (n >= 17), else a datagram carries up to three kinds of different groups
    (sequence number, type, length, damage).  A datagram without a kind of some group gets
    that group's plain value: a DATA datagram of 0 .. min(1456, stride - 16) bytes, intact,
    for an empty slot of the window if it has a kind (then only the kind keeps it from being
    placed), else mostly for a low slot, so that a leading run fills up."""
    if n is None:
        n = int(rng.integers(8, 601))
    ring = rng.integers(0, 256, n * stride, dtype=np.uint8)  # random bytes behind every datagram
    recv_len = np.zeros(n, dtype=np.uint32)
    kinds = [set() for _ in range(n)]
    if n == 0:
        return ring, recv_len, kinds
    assert n >= 8
    order = rng.permutation(n)
    for j, kind in enumerate(fuzz_kinds(stride)):
        kinds[order[j % n]].add(kind)
    first, dup = sorted((int(order[0]), int(order[1])))  # the duplicate arrives after its original
    for i in (first, dup):
        kinds[i] -= {"placeable", "dup_batch"}
    kinds[first].add("placeable")
    kinds[dup].add("dup_batch")
    state = np.asarray(state)
    filled, empty = np.flatnonzero(state != EMPTY), np.flatnonzero(state == EMPTY)

    # About 8 slots of the window (the same ones in every call) are holes: no plain datagram
    # is sent for them, so the window does not fill up, the ACK stays inside it, and the
    # datagrams that have a kind find empty slots in every call.
    every = np.arange(window, dtype=np.uint64)
    hole = ((every + np.uint64(1)) * np.uint64(0x9E3779B1) & np.uint64(M32)) % np.uint64(window) < 8
    plain = np.flatnonzero(~hole)
    empty_holes = np.flatnonzero(hole & (state == EMPTY))
    if empty_holes.size:
        empty = empty_holes

    def pick(slots):
        return int(slots[rng.integers(slots.size)]) if slots.size else int(rng.integers(window))

    fresh, fresh_len = pick(empty), -1
    maxlen = min(MAXP, stride - 16)
    for i in range(n):
        k = kinds[i]
        if "placeable" in k or "dup_batch" in k:
            s = fresh
        elif "dup_filled" in k:
            s = pick(filled)
        elif "below" in k:
            s = -1 - int(rng.integers(4))
        elif "at_end" in k:
            s = window
        elif "above" in k:
            s = window + 1 + int(rng.integers(50))
        elif "far" in k:
            s = int(rng.integers(window + 1000, (1 << 32) - 1000))
        elif k:
            s = pick(empty)  # so that only the kind itself keeps it from being placed
        elif plain.size and rng.random() < 0.8:
            s = int(plain[int(plain.size * rng.random() ** 2)])
        else:
            s = int(rng.integers(-20, 20))
            s += window if s >= 0 else 0  # up to 20 below the window or past its end
        ptype = next((t for t in (0, 1, 3, 7) if f"type{t}" in k), 2)
        if "zero" in k:
            ln = 0
        elif "long" in k:
            ln = int(rng.integers(MAXP + 1, stride - 16 + 1))
        else:
            ln = maxlen if rng.random() < 0.05 else int(rng.integers(0, maxlen + 1))
            if "flip_payload" in k or "placeable" in k:
                ln = max(ln, 1)
            if "dup_batch" in k and ln == fresh_len:  # other bytes and another length
                ln = ln - 1 if ln > 1 else 2
        if "placeable" in k:
            fresh_len = ln
        d = bytearray(O.build_datagram((seq0 + s) & M32, rng.integers(0, 256, ln, dtype=np.uint8).tobytes(), ptype=ptype))
        if "flip_payload" in k and ln:
            d[16 + int(rng.integers(ln))] ^= 1 << int(rng.integers(8))
        if "flip_crc" in k or ("flip_payload" in k and not ln):
            d[12 + int(rng.integers(4))] ^= 1 << int(rng.integers(8))
        ring[i * stride:i * stride + len(d)] = np.frombuffer(bytes(d), dtype=np.uint8)
        recv_len[i] = len(d)
        if "runt" in k:
            recv_len[i] = (0, 15)[int(rng.integers(2))]
        if "over_stride" in k:
            recv_len[i] = stride + 1 + int(rng.integers(3000))
    return ring, recv_len, kinds


def fuzz_verdict(kind, ok, placed, recv_len, stored):
    """Whether the model's verdict on a datagram made for `kind` alone is the one the kind
    stands for (stored: slot_len of its slot after the call, for a placed one)."""
    if kind == "placeable":
        return ok and placed
    if kind == "zero":
        return ok and recv_len == 16 and placed and stored == 0
    if kind in ("runt", "over_stride", "flip_payload", "flip_crc"):
        return not ok and not placed
    if kind == "long":
        return ok and not placed and recv_len - 16 > MAXP
    return ok and not placed  # duplicates, sequence numbers outside the window, other types
