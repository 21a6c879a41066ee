"""C-ABI checks of the connection table that need no GPU: the entry points exist, the header
and the binding declare them, the constants agree, and every WTP_EINVAL case of
include/wtp_crc32.h is refused with a message of its own before any device is touched (the
pointers below are host addresses that are never dereferenced)."""
import ctypes as C
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAXF = MAXW = 1 << 20
NAMES = ("wtp_conn_table_bytes", "wtp_conn_bucket", "wtp_flows_classify", "wtp_conn_scratch_bytes", "wtp_flows_control")
CONTROL_PARAMS = ["d_dgrams", "stride", "d_recv_len", "d_keys", "key_stride", "d_flow", "d_ok", "n", "d_table", "nbuckets", "nflows",
                  "window", "d_flow_start", "d_seq0", "d_slot_len", "d_free", "d_free_pos", "d_ack_wire", "ack_stride", "max_acks",
                  "d_ack_src", "d_opened", "d_opened_src", "d_closed", "d_verdict", "d_counts", "d_work", "work_bytes", "stream"]


@pytest.fixture(scope="module")
def L():
    import wtp_crc32 as W
    return W.LIB


@pytest.fixture(scope="module")
def p():
    buf = C.create_string_buffer(1 << 12)
    yield (C.addressof(buf) + 15) & ~15
    del buf


def classify_args(p, **kw):
    a = dict(d_keys=p, key_stride=16, n=4, d_table=p, nbuckets=8, d_flow=p, stream=None)
    a.update(kw)
    return list(a.values())


def control_args(p, **kw):
    a = dict(zip(CONTROL_PARAMS, [p, 16, p, p, 16, p, p, 4, p, 8, 3, 5, p, p, p, p, p, p, 16, 4, p, p, p, p, p, p, p, 1 << 16, None]))
    a.update(kw)
    return list(a.values())


def test_symbols_header_binding_and_constants():
    import wtp_crc32 as W
    for name in NAMES:
        assert name in W.EXPORTED and getattr(W.LIB, name).argtypes is not None
    for f in (W.flows_classify, W.flows_control, W.conn_table_bytes, W.conn_bucket):
        assert f.__doc__
    assert callable(W.conn_scratch_bytes)
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def params(name):
        m = re.search(r"\w+\s+" + name + r"\s*\(([^)]*)\)", decl)
        assert m, name
        return [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]

    assert params("wtp_flows_classify") == ["d_keys", "key_stride", "n", "d_table", "nbuckets", "d_flow", "stream"]
    assert params("wtp_flows_control") == CONTROL_PARAMS
    assert params("wtp_conn_scratch_bytes") == ["n", "nflows"] and params("wtp_conn_bucket") == ["key16", "nbuckets"]
    assert [len(getattr(W.LIB, n).argtypes) for n in NAMES] == [1, 2, 7, 2, 29]
    consts = dict(re.findall(r"#define (WTP_(?:NO_FLOW|CONN_\w+|CTL_\w+))\s+(\(1u << \d+\)|\w+)", src))

    def literal(v):
        m = re.fullmatch(r"\(1u << (\d+)\)", v)
        return 1 << int(m.group(1)) if m else int(v.rstrip("u"), 0)

    val = {k: literal(v) for k, v in consts.items()}
    assert val["WTP_NO_FLOW"] == W.NO_FLOW == 0xFFFFFFFF
    assert (val["WTP_CONN_KEY_BYTES"], val["WTP_CONN_WAYS"], val["WTP_CONN_MAX_BUCKETS"]) == (16, 16, 1 << 20)
    assert (W.CONN_KEY_BYTES, W.CONN_WAYS, W.CONN_MAX_BUCKETS) == (16, 16, 1 << 20)
    ctl = ["NONE", "OPENED", "START_DUP", "START_OTHER", "REFUSED_FULL", "REFUSED_BUCKET", "CLOSED", "END_STALE", "END_OTHER", "END_BUSY"]
    assert [val["WTP_CTL_" + c] for c in ctl] == [getattr(W, "CTL_" + c) for c in ctl] == list(range(10))
    import conn_model as M
    assert list(M.VERDICTS) == ctl and M.NO_FLOW == W.NO_FLOW and M.WAYS == W.CONN_WAYS
    for kernel in ("k_conn_classify", "k_conn_reset", "k_conn_emit"):
        assert kernel in src


def test_no_new_work_bytes_name():
    """The exported names ending in _work_bytes are the recorded set: the scratch function of
    wtp_flows_control is wtp_conn_scratch_bytes."""
    import wtp_crc32 as W
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_refusals.json")))
    assert {n for n in W.EXPORTED if n.endswith("_work_bytes")} == set(want["work_bytes"])
    assert "wtp_conn_scratch_bytes" in W.EXPORTED


def collect(L, fn, make, p, cases):
    msgs = {}
    for name, kw in cases.items():
        assert fn(*make(p, **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
        assert msgs[name], name
    return msgs


BUCKETS = {"nbuckets": dict(nbuckets=0), "nbuckets, not a power of two": dict(nbuckets=12),
           "nbuckets, above the limit": dict(nbuckets=1 << 21)}


def distinct(msgs):
    """One message per case; a name with a comma is another way into the case before the comma."""
    kinds = {k.split(",")[0] for k in msgs}
    assert len({msgs[k] for k in kinds}) == len(kinds), msgs
    for k in msgs:
        head = k.split(",")[0]
        assert msgs[k].split(" ")[0] == msgs[head].split(" ")[0], (k, msgs[k])


def test_classify_einval(L, p):
    cases = dict(BUCKETS, **{"n": dict(n=1 << 31), "key_stride": dict(key_stride=15), "d_keys": dict(d_keys=None),
                             "d_table": dict(d_table=None), "d_flow": dict(d_flow=None), "aligned": dict(d_table=p + 4)})
    msgs = collect(L, L.wtp_flows_classify, classify_args, p, cases)
    distinct(msgs)
    for ptr in ("d_keys", "d_table", "d_flow"):
        assert "null" in msgs[ptr] and ptr in msgs[ptr]
    assert "aligned" in msgs["aligned"] and "key_stride 15 < 16" in msgs["key_stride"] and "2^31" in msgs["n"]
    # in the header's order
    order = [("n", dict(n=1 << 31)), ("key_stride", dict(key_stride=0)), ("nbuckets", dict(nbuckets=3)), ("d_keys", dict(d_keys=None)),
             ("d_flow", dict(d_flow=None)), ("aligned", dict(d_table=p + 8))]
    for i, (why, _) in enumerate(order):
        kw = {}
        for _, more in order[i:]:
            kw.update(more)
        assert L.wtp_flows_classify(*classify_args(p, **kw)) == EINVAL and why in L.wtp_last_error().decode(), why
    # n == 0 launches nothing and needs no pointer; the limits themselves pass
    assert L.wtp_flows_classify(None, 16, 0, None, 1, None, None) == 0
    assert L.wtp_flows_classify(None, 1 << 40, 0, None, 1 << 20, None, None) == 0
    assert L.wtp_flows_classify(*classify_args(p, n=(1 << 31) - 1, nbuckets=1 << 20, d_flow=None)) == EINVAL
    assert "d_flow" in L.wtp_last_error().decode()


def test_control_einval(L, p):
    need = L.wtp_conn_scratch_bytes(4, 3)
    cases = dict(BUCKETS, **{
        "n": dict(n=1 << 31), "stride": dict(stride=15), "key_stride": dict(key_stride=15), "ack_stride": dict(ack_stride=15),
        "nflows": dict(nflows=MAXF + 1, window=0), "window": dict(nflows=0, window=MAXW + 1), "slots": dict(nflows=1 << 13, window=1 << 12),
        "work_bytes": dict(work_bytes=need - 1), "aligned": dict(d_table=p + 4)})
    ptrs = ["d_counts", "d_work", "d_table", "d_flow_start", "d_seq0", "d_free", "d_free_pos", "d_opened", "d_closed", "d_slot_len",
            "d_dgrams", "d_recv_len", "d_ok", "d_keys", "d_flow", "d_ack_wire"]
    cases.update({q: {q: None} for q in ptrs})
    cases["slots"]["work_bytes"] = cases["nflows"]["work_bytes"] = 1 << 40
    msgs = collect(L, L.wtp_flows_control, control_args, p, cases)
    distinct(msgs)
    for q in ptrs:
        assert msgs[q] == f"null pointer: {q}"
    assert f"work_bytes {need - 1} < {need}" in msgs["work_bytes"] and "aligned" in msgs["aligned"]
    assert "stride 15 < 16" == msgs["stride"] and "key_stride 15 < 16" == msgs["key_stride"] and "ack_stride 15 < 16" == msgs["ack_stride"]
    assert L.wtp_flows_control(*control_args(p, work_bytes=need, d_counts=None)) == EINVAL
    assert "d_counts" in L.wtp_last_error().decode()  # exactly wtp_conn_scratch_bytes(n, nflows) is enough
    # in the header's order
    order = [("n ", dict(n=1 << 31)), ("stride ", dict(stride=3)), ("key_stride ", dict(key_stride=3)),
             ("ack_stride ", dict(ack_stride=3)), ("nbuckets ", dict(nbuckets=5)), ("window ", dict(window=MAXW + 1)),
             ("work_bytes ", dict(work_bytes=0)), ("null pointer: d_counts", dict(d_counts=None)),
             ("null pointer: d_work", dict(d_work=None)), ("null pointer: d_seq0", dict(d_seq0=None)),
             ("null pointer: d_slot_len", dict(d_slot_len=None)), ("null pointer: d_keys", dict(d_keys=None)),
             ("null pointer: d_ack_wire", dict(d_ack_wire=None)), ("d_table ", dict(d_table=p + 1))]
    for i, (why, _) in enumerate(order):
        kw = {}
        for _, more in order[i:]:
            kw.update(more)
        assert L.wtp_flows_control(*control_args(p, **kw)) == EINVAL
        assert L.wtp_last_error().decode().startswith(why), (why, L.wtp_last_error())
    # what a shape does not need may be NULL and is then not the reason
    none = dict(d_table=None, d_flow_start=None, d_seq0=None, d_free=None, d_free_pos=None, d_opened=None, d_closed=None, d_slot_len=None)
    batch = dict(d_dgrams=None, d_recv_len=None, d_ok=None, d_keys=None, d_flow=None, d_ack_wire=None)
    for kw, why in ((dict(none, nflows=0, d_counts=None), "d_counts"),
                    (dict(window=0, d_slot_len=None, d_work=None), "d_work"),
                    (dict(batch, n=0, d_work=None), "d_work"),
                    (dict(max_acks=0, d_ack_wire=None, d_ack_src=None, d_opened_src=None, d_verdict=None, d_work=None), "d_work")):
        assert L.wtp_flows_control(*control_args(p, **kw)) == EINVAL and why in L.wtp_last_error().decode(), kw


def test_scratch_and_table_sizes(L):
    grid_n = [0, 1, 1023, 1024, 1025, 65536, (1 << 24) + 1, (1 << 31) - 1]
    grid_f = [0, 1, 7, 1 << 10, MAXF]
    for a, n in enumerate(grid_n):
        for b, f in enumerate(grid_f):
            v = L.wtp_conn_scratch_bytes(n, f)
            assert v == 20 + 4 * n + 12 * ((n + 1023) // 1024) + 8 * f  # the header's formula
            assert v <= (64 << 10) + 8 * n + 8 * f
            assert a == 0 or v >= L.wtp_conn_scratch_bytes(grid_n[a - 1], f)
            assert b == 0 or v >= L.wtp_conn_scratch_bytes(n, grid_f[b - 1])
    # the arguments are clamped to the limits
    assert L.wtp_conn_scratch_bytes(1 << 40, MAXF + 5) == L.wtp_conn_scratch_bytes((1 << 31) - 1, MAXF)
    assert [L.wtp_conn_table_bytes(b) for b in (1, 2, 1 << 20)] == [320, 640, 320 << 20]
    assert [L.wtp_conn_table_bytes(b) for b in (0, 3, 1 << 21)] == [0, 0, 0]


def test_bucket_is_below_nbuckets_and_stable(L):
    import wtp_crc32 as W
    import conn_model as M
    keys = M.fuzz_keys() + [bytes(16), b"\xff" * 16, bytes(range(16))]
    for nb in (1, 2, 4, 1024, 1 << 20):
        got = [W.conn_bucket(k, nb) for k in keys]
        assert all(0 <= g < nb for g in got) and got == [W.conn_bucket(k, nb) for k in keys]
        assert got == [W.conn_bucket(k, 1 << 20) & (nb - 1) for k in keys]  # one hash, masked
    # every byte of the key counts, and the 2048 keys of two /22s spread over 64 buckets as a hash should
    base = bytes(range(16))
    assert len({W.conn_bucket(base[:j] + bytes([base[j] ^ 1]) + base[j + 1:], 1 << 20) for j in range(16)} | {W.conn_bucket(base, 1 << 20)}) == 17
    loads = [0] * 64
    for j in range(2048):
        loads[W.conn_bucket(M.key_of(40000 + j % 7, 0x0A000000 + j), 64)] += 1
    assert max(loads) <= 64 and min(loads) >= 12  # mean 32; a Poisson tail beyond these has probability < 1e-5
    assert L.wtp_conn_bucket(None, 4) == W.NO_FLOW and L.wtp_conn_bucket(bytes(16), 3) == W.NO_FLOW
    with pytest.raises(W.WtpError):
        W.conn_bucket(b"short", 4)


def test_valid_without_device(L, p):
    """n == 0 without flows still has d_counts to write, so it launches; what can be checked here
    is that the limits themselves pass the limit checks: their refusal is the next check's."""
    for nf, w in ((MAXF, 1), (1, MAXW), (1 << 12, 1 << 12)):
        need = L.wtp_conn_scratch_bytes(4, nf)
        assert L.wtp_flows_control(*control_args(p, nflows=nf, window=w, work_bytes=need, d_counts=None)) == EINVAL
        assert "d_counts" in L.wtp_last_error().decode()
        assert L.wtp_flows_control(*control_args(p, nflows=nf, window=w, work_bytes=need - 1)) == EINVAL
        assert "work_bytes" in L.wtp_last_error().decode()
    assert L.wtp_flows_control(*control_args(p, n=(1 << 31) - 1, nbuckets=1 << 20, work_bytes=1 << 40, d_counts=None)) == EINVAL
    assert "d_counts" in L.wtp_last_error().decode()
