"""C-ABI checks of wtp_rx_digest_flows that need no GPU: the entry points exist, the header and
the binding declare them in the same order, the set of *_work_bytes names is unchanged, every
WTP_EINVAL case of include/wtp_crc32.h is refused with a message of its own before any device is
touched (the pointers below are host addresses that are never dereferenced), and the scratch
size is the header's formula."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

import digest_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAXF = 1 << 20
NAMES = ("wtp_rx_digest_scratch_bytes", "wtp_rx_digest_flows")
PARAMS = ["d_stream", "stream_bytes", "d_flow_info", "nflows", "d_flow_crc", "d_flow_bytes", "d_reset", "d_reset_count", "max_reset",
          "d_report", "d_report_count", "max_report", "d_report_crc", "d_report_bytes", "d_counts", "d_work", "work_bytes", "stream"]


@pytest.fixture(scope="module")
def L():
    import wtp_crc32 as W
    return W.LIB


@pytest.fixture(scope="module")
def p():
    buf = C.create_string_buffer(1 << 12)
    yield (C.addressof(buf) + 15) & ~15
    del buf


def args(p, **kw):
    a = dict(zip(PARAMS, [p, 4096, p, 3, p, p, p, p, 4, p, p, 4, p, p, p, p, 1 << 16, None]))
    a.update(kw)
    return list(a.values())


def test_symbols_header_and_binding():
    import wtp_crc32 as W
    for name in NAMES:
        assert name in W.EXPORTED and getattr(W.LIB, name).argtypes is not None
    assert W.rx_digest_flows.__doc__ and W.rx_digest_scratch_bytes.__doc__
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def params(name):
        m = re.search(r"\w+\s+" + name + r"\s*\(([^)]*)\)", decl)
        assert m, name
        return [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]

    assert params("wtp_rx_digest_flows") == PARAMS and params("wtp_rx_digest_scratch_bytes") == ["nflows"]
    assert [len(getattr(W.LIB, n).argtypes) for n in NAMES] == [1, len(PARAMS)]
    # the binding takes the header's parameters in the header's order (d_ dropped, the stream buffer renamed)
    names = list(inspect.signature(W.rx_digest_flows).parameters)
    want = [q[2:] if q.startswith("d_") else q for q in PARAMS if q != "work_bytes"]
    want[want.index("stream")] = "stream_buf"
    assert names == want[:-2] + ["work", "stream"]
    for kernel in ("k_dig_reset", "k_dig_report"):
        assert kernel in src
    assert "16432 + 12*nflows" in src


def test_no_new_work_bytes_name():
    """The exported names ending in _work_bytes are the recorded set: the scratch function of
    wtp_rx_digest_flows is wtp_rx_digest_scratch_bytes."""
    import wtp_crc32 as W
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_refusals.json")))
    assert {n for n in W.EXPORTED if n.endswith("_work_bytes")} == set(want["work_bytes"])
    assert "wtp_rx_digest_scratch_bytes" in W.EXPORTED


def refused(L, p, **kw):
    assert L.wtp_rx_digest_flows(*args(p, **kw)) == EINVAL, kw
    msg = L.wtp_last_error().decode()
    assert msg, kw
    return msg


def test_einval(L, p):
    need = L.wtp_rx_digest_scratch_bytes(3)
    cases = {"nflows": dict(nflows=MAXF + 1, work_bytes=1 << 40), "work_bytes": dict(work_bytes=need - 1),
             "reset list": dict(d_reset=None), "reset count": dict(d_reset_count=None),
             "report list": dict(d_report=None), "report count": dict(d_report_count=None)}
    ptrs = ["d_counts", "d_work", "d_flow_info", "d_flow_crc", "d_flow_bytes", "d_stream", "d_report_crc", "d_report_bytes"]
    cases.update({q: {q: None} for q in ptrs})
    msgs = {k: refused(L, p, **kw) for k, kw in cases.items()}
    for q in ptrs:
        assert msgs[q] == f"null pointer: {q}"
    assert msgs["nflows"] == f"nflows {MAXF + 1} > {MAXF}" and msgs["work_bytes"] == f"work_bytes {need - 1} < {need}"
    assert msgs["reset list"] == msgs["reset count"] and "d_reset" in msgs["reset list"]
    assert msgs["report list"] == msgs["report count"] and "d_report" in msgs["report list"]
    assert len(set(msgs.values())) == len(msgs) - 2  # one message per case
    # in the header's order
    order = [("nflows ", dict(nflows=MAXF + 1)), ("work_bytes ", dict(work_bytes=0)), ("null pointer: d_counts", dict(d_counts=None)),
             ("null pointer: d_work", dict(d_work=None)), ("null pointer: d_flow_info", dict(d_flow_info=None)),
             ("null pointer: d_flow_crc", dict(d_flow_crc=None)), ("null pointer: d_flow_bytes", dict(d_flow_bytes=None)),
             ("null pointer: d_stream", dict(d_stream=None)), ("exactly one of d_reset", dict(d_reset=None)),
             ("exactly one of d_report", dict(d_report_count=None))]
    for i, (why, _) in enumerate(order):
        kw = {}
        for _, more in order[i:]:
            kw.update(more)
        assert refused(L, p, **kw).startswith(why), why
    # exactly the scratch size is enough; what a shape does not need may be NULL and is then not the reason
    assert refused(L, p, work_bytes=need, d_counts=None) == "null pointer: d_counts"
    none = dict(d_flow_info=None, d_flow_crc=None, d_flow_bytes=None, d_stream=None)
    for kw in (dict(none, nflows=0), dict(d_stream=None, stream_bytes=0), dict(d_reset=None, d_reset_count=None),
               dict(d_report=None, d_report_count=None, d_report_crc=None, d_report_bytes=None),
               dict(max_report=0, d_report_crc=None, d_report_bytes=None)):
        assert refused(L, p, d_work=None, **kw) == "null pointer: d_work", kw


def test_valid_without_device(L, p):
    """nflows == 0 still has d_counts to write, so it launches; what can be checked here is that
    the no-op shapes and the limits themselves pass every check up to the last one."""
    need0 = L.wtp_rx_digest_scratch_bytes(0)
    none = dict(d_flow_info=None, d_flow_crc=None, d_flow_bytes=None, d_stream=None, d_reset=None, d_reset_count=None, d_report=None,
                d_report_count=None, d_report_crc=None, d_report_bytes=None)
    assert refused(L, p, nflows=0, stream_bytes=1 << 40, work_bytes=need0, d_work=None, **none) == "null pointer: d_work"
    assert refused(L, p, nflows=0, work_bytes=need0 - 1, **none).startswith("work_bytes")
    need = L.wtp_rx_digest_scratch_bytes(MAXF)
    assert refused(L, p, nflows=MAXF, work_bytes=need, max_reset=0xFFFFFFFF, max_report=0xFFFFFFFF, d_work=None) == "null pointer: d_work"
    assert refused(L, p, nflows=MAXF, work_bytes=need - 1).startswith("work_bytes")


def test_scratch_size(L):
    grid = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 65536, MAXF - 1, MAXF]
    for a, f in enumerate(grid):
        v = L.wtp_rx_digest_scratch_bytes(f)
        assert v == 16432 + 12 * f == M.scratch_bytes(f)  # the header's formula
        assert v <= (64 << 10) + 16 * f
        assert a == 0 or v >= L.wtp_rx_digest_scratch_bytes(grid[a - 1])
    assert L.wtp_rx_digest_scratch_bytes(MAXF + 5) == L.wtp_rx_digest_scratch_bytes(0xFFFFFFFF) == L.wtp_rx_digest_scratch_bytes(MAXF)
