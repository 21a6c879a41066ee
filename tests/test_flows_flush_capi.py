"""C-ABI checks of the multi-connection flush and slide that need no GPU: the entry points
exist, the header and the binding declare them, and every WTP_EINVAL case of
include/wtp_crc32.h is refused with a message of its own before any device is touched (the
pointers below are host addresses that are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, MAXP = -1, 1456
MAXW, MAXF, MAXS = 1 << 20, 1 << 20, 1 << 24


@pytest.fixture(scope="module")
def L():
    import wtp_crc32 as W
    return W.LIB


@pytest.fixture(scope="module")
def mem():
    buf = C.create_string_buffer(1 << 17)
    return (C.addressof(buf) + 15) & ~15, buf  # the buffer lives as long as the fixture


def deliver_args(p, **kw):
    a = dict(d_img=p, d_slot_len=p, nflows=3, window=5, max_slots=5, d_stream=p, stream_bytes=4096, stream_off=0,
             d_offsets_out=p, d_lengths_out=p, d_flow_adv=p, d_flow_info=p, d_counts=p, d_work=p, work_bytes=1 << 16, stream=None)
    a.update(kw)
    return list(a.values())


def advance_args(p, nflows=3, window=5, **kw):
    """Two states that touch: every `next` array starts at the byte after its input's last."""
    s = nflows * window
    a = dict(d_img=p, d_slot_len=p + 65536, nflows=nflows, window=window, d_flow_adv=p + 98304, d_seq0=p + 90000,
             d_img_next=p + s * MAXP, d_slot_len_next=p + 65536 + 4 * s, d_seq0_next=p + 90000 + 4 * nflows, stream=None)
    a.update(kw)
    return list(a.values())


BIG = 1 << 40  # a work size that no limit case is refused for

DELIVER_CASES = {
    "nflows": dict(nflows=MAXF + 1, window=1, work_bytes=BIG),
    "window": dict(nflows=1, window=MAXW + 1, work_bytes=BIG),
    "slots": dict(nflows=(1 << 12) + 1, window=1 << 12, work_bytes=BIG),
    "slots, product past 2^32": dict(nflows=1 << 20, window=1 << 20, work_bytes=BIG),
    "stream_off": dict(stream_off=4097),
    "work_bytes": dict(work_bytes=39),
    "d_counts": dict(d_counts=None),
    "d_work": dict(d_work=None),
    "d_flow_adv": dict(d_flow_adv=None),
    "d_flow_adv, window == 0": dict(d_flow_adv=None, window=0),
    "d_img": dict(d_img=None),
    "d_slot_len": dict(d_slot_len=None),
    "d_stream": dict(d_stream=None),
}


def test_symbols_header_and_binding():
    import wtp_crc32 as W
    names = ("wtp_rx_deliver_flows_work_bytes", "wtp_rx_deliver_flows", "wtp_rx_advance_flows")
    for name in names:
        assert name in W.EXPORTED and getattr(W.LIB, name).argtypes is not None
    assert W.rx_deliver_flows.__doc__ and W.rx_advance_flows.__doc__ and callable(W.rx_deliver_flows_work_bytes)
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def params(ret, name):
        m = re.search(ret + r"\s+" + name + r"\s*\(([^)]*)\)", decl)
        assert m, name
        return [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]

    assert params("size_t", names[0]) == ["nflows", "window"]
    assert params("int", names[1]) == ["d_img", "d_slot_len", "nflows", "window", "max_slots", "d_stream", "stream_bytes",
                                       "stream_off", "d_offsets_out", "d_lengths_out", "d_flow_adv", "d_flow_info", "d_counts",
                                       "d_work", "work_bytes", "stream"]
    assert params("int", names[2]) == ["d_img", "d_slot_len", "nflows", "window", "d_flow_adv", "d_seq0", "d_img_next",
                                       "d_slot_len_next", "d_seq0_next", "stream"]
    assert len(W.LIB.wtp_rx_deliver_flows.argtypes) == 16 and len(W.LIB.wtp_rx_advance_flows.argtypes) == 10
    assert "k_rx_advance_flows" in src and "k_dflows_copy" in src


def test_deliver_flows_einval(L, mem):
    msgs = {}
    for name, kw in DELIVER_CASES.items():
        assert L.wtp_rx_deliver_flows(*deliver_args(mem[0], **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
        assert msgs[name], name
    # one message per case of the header; the two ways into a case share its message
    kinds = {k.split(",")[0] for k in msgs}
    assert len({msgs[k] for k in kinds}) == len(kinds) == 11, msgs
    assert msgs["d_flow_adv"] == msgs["d_flow_adv, window == 0"]
    assert msgs["slots"].split(">")[1] == msgs["slots, product past 2^32"].split(">")[1]
    for ptr in ("d_counts", "d_work", "d_flow_adv", "d_img", "d_slot_len", "d_stream"):
        assert ptr in msgs[ptr] and "null" in msgs[ptr]
    need = L.wtp_rx_deliver_flows_work_bytes(3, 5)
    assert L.wtp_rx_deliver_flows(*deliver_args(mem[0], work_bytes=need - 1)) == EINVAL
    assert f"work_bytes {need - 1} < {need}" in L.wtp_last_error().decode()
    # the checks come in the header's order: the limits, the stream, the work size, then the pointers
    a = mem[0]
    assert L.wtp_rx_deliver_flows(*deliver_args(a, nflows=MAXF + 1, stream_off=5000, d_counts=None)) == EINVAL
    assert "nflows" in L.wtp_last_error().decode()
    assert L.wtp_rx_deliver_flows(*deliver_args(a, stream_off=5000, work_bytes=0, d_counts=None)) == EINVAL
    assert "stream_off" in L.wtp_last_error().decode()
    assert L.wtp_rx_deliver_flows(*deliver_args(a, work_bytes=0, d_counts=None)) == EINVAL
    assert "work_bytes" in L.wtp_last_error().decode()
    # what a shape does not need may be NULL and is then not the reason: the refusal is the next check's
    for kw, why in ((dict(nflows=0, d_flow_adv=None, d_img=None, d_slot_len=None, d_stream=None, d_counts=None), "d_counts"),
                    (dict(window=0, d_img=None, d_slot_len=None, d_stream=None, d_work=None), "d_work"),
                    (dict(max_slots=0, d_stream=None, d_work=None), "d_work")):
        assert L.wtp_rx_deliver_flows(*deliver_args(a, **kw)) == EINVAL and why in L.wtp_last_error().decode()


def test_deliver_flows_work_bytes_is_monotone_and_bounded(L):
    sizes = [0, 1, 2, 3, 16, 64, 1023, 1024, 1025, 1 << 12, 1 << 14, 1 << 20]
    for a in sizes:
        for b in sizes:
            got = L.wtp_rx_deliver_flows_work_bytes(a, b)
            s = min(a * b, MAXS)
            assert got == 40 + 12 * s + 28 * ((s + 1023) // 1024) + 16 * a  # the header's formula
            assert got <= (64 << 10) + 16 * s + 16 * a
            for a2 in sizes:
                if a2 >= a:
                    assert L.wtp_rx_deliver_flows_work_bytes(a2, b) >= got and L.wtp_rx_deliver_flows_work_bytes(b, a2) >= \
                        L.wtp_rx_deliver_flows_work_bytes(b, a)
    top = L.wtp_rx_deliver_flows_work_bytes(MAXF, MAXW)
    assert L.wtp_rx_deliver_flows_work_bytes(MAXF + 1, MAXW + 7) == top == L.wtp_rx_deliver_flows_work_bytes(1 << 30, 1 << 30)


ADVANCE_CASES = {
    "nflows": dict(nflows=MAXF + 1, window=1),
    "window": dict(nflows=1, window=MAXW + 1),
    "slots": dict(nflows=(1 << 12) + 1, window=1 << 12),
    "no d_img": dict(d_img=None),
    "no d_img_next": dict(d_img_next=None),
    "no d_seq0": dict(d_seq0=None),
    "no d_seq0_next": dict(d_seq0_next=None),
    "d_flow_adv": dict(d_flow_adv=None),
    "d_slot_len": dict(d_slot_len=None),
    "d_slot_len_next": dict(d_slot_len_next=None),
}


def test_advance_flows_einval(L, mem):
    a = mem[0]
    msgs = {}
    for name, kw in ADVANCE_CASES.items():
        assert L.wtp_rx_advance_flows(*advance_args(a, **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
    assert len(set(msgs.values())) == len(msgs), msgs
    for ptr in ("d_flow_adv", "d_slot_len", "d_slot_len_next"):
        assert f"null pointer: {ptr} " in msgs[ptr]
    assert "d_img without d_img_next" in msgs["no d_img"] and "d_seq0_next without d_seq0" in msgs["no d_seq0_next"]
    # an output range over its input range by one element, either way round, and the same array
    base = dict(zip(("d_img", "d_slot_len", "nflows", "window", "d_flow_adv", "d_seq0", "d_img_next", "d_slot_len_next",
                     "d_seq0_next"), advance_args(a)))
    over = {}
    for arr, unit in (("d_slot_len", 4), ("d_img", 1), ("d_seq0", 4)):
        nxt = arr + "_next"
        for kw in ({nxt: base[nxt] - unit}, {arr: base[nxt], nxt: base[arr] + unit}, {nxt: base[arr]}):
            assert L.wtp_rx_advance_flows(*advance_args(a, **kw)) == EINVAL, (arr, kw)
            over[arr] = L.wtp_last_error().decode()
            assert f"{nxt} overlaps {arr}" in over[arr]
    assert len(set(over.values())) == 3
    # seq0 is checked over 4 * nflows bytes, not 4 * nflows * window: 4 * nflows apart is valid (advance_args), closer is not
    assert L.wtp_rx_advance_flows(*advance_args(a, d_seq0_next=base["d_seq0"] + 4 * 3 - 4)) == EINVAL
    # ranges that touch are accepted: with the slot_len arrays and the images of advance_args, which touch, the
    # refusal is the last check's
    assert L.wtp_rx_advance_flows(*advance_args(a, d_seq0_next=base["d_seq0"])) == EINVAL
    assert "d_seq0_next overlaps d_seq0" in L.wtp_last_error().decode()
    # the limits come first, the pairs before the pointers, the state's overlap before the image's
    assert L.wtp_rx_advance_flows(*advance_args(a, nflows=MAXF + 1, d_img=None, d_flow_adv=None)) == EINVAL
    assert "nflows" in L.wtp_last_error().decode()
    assert L.wtp_rx_advance_flows(*advance_args(a, d_img=None, d_flow_adv=None)) == EINVAL
    assert "without" in L.wtp_last_error().decode()
    assert L.wtp_rx_advance_flows(*advance_args(a, d_slot_len_next=base["d_slot_len"], d_img_next=base["d_img"])) == EINVAL
    assert "d_slot_len_next" in L.wtp_last_error().decode()
    assert L.wtp_rx_advance_flows(*advance_args(a, window=0, d_img=None)) == EINVAL  # a pair is a pair whatever the shape


def test_valid_without_device(L, mem):
    """What launches nothing returns WTP_OK without a device: a state of no slots, at the limits
    too.  (Ranges that touch are what advance_args passes; with slots they launch, so
    tests/test_gpu_flows_flush.py has them, and test_advance_flows_einval shows that they are
    not refused.)"""
    a = mem[0]
    assert L.wtp_rx_advance_flows(None, None, 0, 0, None, None, None, None, None, None) == 0
    assert L.wtp_rx_advance_flows(*advance_args(a, nflows=0)) == 0
    assert L.wtp_rx_advance_flows(*advance_args(a, window=0)) == 0
    assert L.wtp_rx_advance_flows(None, None, MAXF, 0, None, None, None, None, None, None) == 0
    assert L.wtp_rx_advance_flows(None, None, 0, MAXW, None, None, None, None, None, None) == 0
    # the limits themselves pass the limit checks: the refusal is the next check's
    for nf, w in ((MAXF, 16), (16, MAXW), (1 << 12, 1 << 12)):
        assert L.wtp_rx_advance_flows(*advance_args(a, nflows=nf, window=w, d_flow_adv=None)) == EINVAL
        assert "d_flow_adv" in L.wtp_last_error().decode()
        need = L.wtp_rx_deliver_flows_work_bytes(nf, w)
        assert L.wtp_rx_deliver_flows(*deliver_args(a, nflows=nf, window=w, work_bytes=need, d_counts=None)) == EINVAL
        assert "d_counts" in L.wtp_last_error().decode()
        assert L.wtp_rx_deliver_flows(*deliver_args(a, nflows=nf, window=w, work_bytes=need - 1)) == EINVAL
        assert "work_bytes" in L.wtp_last_error().decode()
    # stream_off == stream_bytes is valid: the refusal is the next check's
    assert L.wtp_rx_deliver_flows(*deliver_args(a, stream_off=4096, d_work=None)) == EINVAL
    assert "d_work" in L.wtp_last_error().decode()
