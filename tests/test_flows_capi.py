"""C-ABI checks of the multi-connection receive that need no GPU: the entry points exist, the
binding declares them, and every WTP_EINVAL case of include/wtp_crc32.h is refused with a
message of its own before any device is touched (the pointers below are host addresses that
are never dereferenced)."""
import ctypes as C

import pytest

EINVAL = -1
MAXW, MAXF, MAXS, MAXB = 1 << 20, 1 << 20, 1 << 24, 1 << 24


@pytest.fixture(scope="module")
def L():
    import wtp_crc32 as W
    return W.LIB


@pytest.fixture(scope="module")
def p():
    buf = C.create_string_buffer(64)
    return C.addressof(buf), buf  # the buffer lives as long as the fixture


def accept_args(p, **kw):
    a = dict(d_dgrams=p, stride=1472, d_recv_len=p, d_flow=p, n=4, d_seq0=p, nflows=3, window=5, d_out=p, d_slot_len=p,
             d_ok=p, d_place=p, d_ack=p, stream=None)
    a.update(kw)
    return list(a.values())


def acks_args(p, **kw):
    a = dict(d_dgrams=p, stride=1472, d_recv_len=p, d_flow=p, n=4, mode=1, d_seq0=p, nflows=3, window=5, d_ok=p,
             d_flow_ack=p, d_ack_wire=p, ack_stride=16, skip=0, max_acks=4, d_src=p, d_counts=p, d_work=p, work_bytes=64,
             stream=None)
    a.update(kw)
    return list(a.values())


ACCEPT_CASES = {
    "n >= 2^31": dict(n=1 << 31),
    "stride": dict(stride=15),
    "nflows": dict(nflows=MAXF + 1, window=1),
    "window": dict(nflows=1, window=MAXW + 1),
    "slots": dict(nflows=(1 << 12) + 1, window=1 << 12),
    "slots, product past 2^32": dict(nflows=1 << 20, window=1 << 20),
    "d_dgrams": dict(d_dgrams=None),
    "d_recv_len": dict(d_recv_len=None),
    "d_flow": dict(d_flow=None),
    "d_ok": dict(d_ok=None),
    "d_out": dict(d_out=None),
    "d_slot_len": dict(d_slot_len=None),
    "d_seq0": dict(d_seq0=None),
    "d_seq0, n == 0 with d_ack": dict(d_seq0=None, n=0),
}

ACKS_CASES = {
    "n > max": dict(n=MAXB + 1, work_bytes=1 << 20),
    "mode": dict(mode=2),
    "window": dict(window=MAXW + 1),
    "stride": dict(stride=15),
    "ack_stride": dict(ack_stride=15),
    "work_bytes": dict(work_bytes=7),
    "d_counts": dict(d_counts=None),
    "d_work": dict(d_work=None),
    "d_dgrams": dict(d_dgrams=None),
    "d_recv_len": dict(d_recv_len=None),
    "d_ok": dict(d_ok=None),
    "d_flow": dict(d_flow=None),
    "d_seq0": dict(d_seq0=None),
    "d_flow_ack": dict(d_flow_ack=None),
    "d_ack_wire": dict(d_ack_wire=None),
}


def test_symbols_and_binding():
    import wtp_crc32 as W
    for name in ("wtp_accept_data_packets_flows", "wtp_rx_ack_flows_work_bytes", "wtp_rx_build_acks_flows"):
        assert name in W.EXPORTED and getattr(W.LIB, name).argtypes is not None
    for f in (W.accept_data_packets_flows, W.rx_ack_flows_work_bytes, W.rx_build_acks_flows):
        assert f.__doc__ or f is W.rx_ack_flows_work_bytes
    assert (W.RX_MAX_FLOWS, W.RX_MAX_FLOW_SLOTS) == (MAXF, MAXS)


def test_accept_flows_einval(L, p):
    msgs = {}
    for name, kw in ACCEPT_CASES.items():
        assert L.wtp_accept_data_packets_flows(*accept_args(p[0], **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
        assert msgs[name], name
    # one message per case of the header; the two ways into a case share its message
    kinds = {k.split(",")[0] for k in msgs}
    assert len({msgs[k] for k in kinds}) == len(kinds) == 12, msgs
    assert msgs["d_seq0"] == msgs["d_seq0, n == 0 with d_ack"]
    assert msgs["slots"].split(">")[1] == msgs["slots, product past 2^32"].split(">")[1]
    for ptr in ("d_dgrams", "d_recv_len", "d_flow", "d_ok", "d_out", "d_slot_len", "d_seq0"):
        assert ptr in msgs[ptr] and "null" in msgs[ptr]


def test_accept_flows_valid_without_device(L, p):
    """What needs no launch returns WTP_OK without a device: n == 0 with no d_ack or no flows."""
    a = p[0]
    assert L.wtp_accept_data_packets_flows(*accept_args(a, n=0, d_ack=None)) == 0
    assert L.wtp_accept_data_packets_flows(*accept_args(a, n=0, nflows=0, d_seq0=None)) == 0
    assert L.wtp_accept_data_packets_flows(None, 1472, None, None, 0, None, 0, 0, None, None, None, None, None, None) == 0
    # a NULL d_seq0 is fine where nothing reads it; the limits themselves are valid
    assert L.wtp_accept_data_packets_flows(*accept_args(a, n=0, d_ack=None, d_seq0=None, nflows=MAXF, window=16)) == 0
    assert L.wtp_accept_data_packets_flows(*accept_args(a, n=0, d_ack=None, nflows=1, window=MAXW)) == 0
    assert L.wtp_accept_data_packets_flows(*accept_args(a, n=0, d_ack=None, nflows=1 << 12, window=1 << 12)) == 0


def test_acks_flows_einval(L, p):
    msgs = {}
    for name, kw in ACKS_CASES.items():
        assert L.wtp_rx_build_acks_flows(*acks_args(p[0], **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
    assert len(set(msgs.values())) == len(msgs), msgs
    for ptr in ("d_counts", "d_work", "d_dgrams", "d_recv_len", "d_ok", "d_flow", "d_seq0", "d_flow_ack", "d_ack_wire"):
        assert ptr in msgs[ptr] and "null" in msgs[ptr]
    # the forms of these cases that are valid (n == 0, nflows == 0, selective mode, max_acks == 0)
    # launch, so tests/test_gpu_flows.py has them


def test_ack_flows_work_bytes(L):
    sizes = [L.wtp_rx_ack_flows_work_bytes(n) for n in (0, 1, 1024, 1025, 1 << 20, MAXB, MAXB + 1, 1 << 40)]
    assert sizes == sorted(sizes) and sizes[0] >= 4 and sizes[-1] == sizes[-3]
    for n, b in zip((0, 1, 1024, 1025, 1 << 20, MAXB), sizes):
        assert b <= 4 + 4 * ((n + 1023) // 1024) and b <= (64 << 10) + 4
