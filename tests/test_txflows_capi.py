"""C-ABI checks of the multi-connection sender that need no GPU: the three entry points exist,
the header and the binding declare them, the limits agree, and every WTP_EINVAL case of
include/wtp_crc32.h is refused with a message of its own before any device is touched (the
pointers below are host addresses that are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MAXF = MAXW = MAXS = 1 << 20
NAMES = ("wtp_tx_ingest_acks_flows", "wtp_tx_advance_flows", "wtp_tx_build_retransmit_var_flows")


@pytest.fixture(scope="module")
def L():
    import wtp_crc32 as W
    return W.LIB


@pytest.fixture(scope="module")
def p():
    buf = C.create_string_buffer(1 << 17)
    yield (C.addressof(buf) + 15) & ~15
    del buf


def ingest_args(p, **kw):
    a = dict(d_dgrams=p, stride=16, d_recv_len=p, d_flow=p, n=4, mode=0, d_seq0=p, d_rec0=p, d_rec_end=p, nflows=3, window=5,
             d_acked=p, d_ok=p, d_hit=p, d_flow_adv=p, d_flow_fresh=p, stream=None)
    a.update(kw)
    return list(a.values())


def advance_args(p, nflows=3, window=5, **kw):
    """Two states that touch: every `next` array starts at the byte after its input's last."""
    s = nflows * window
    a = dict(d_acked=p, d_sent_ms=p + 8 * s, nflows=nflows, window=window, d_flow_adv=p + 65536, fill_ms=7, d_seq0=p + 70000,
             d_rec0=p + 70000 + 8 * nflows, d_acked_next=p + 4 * s, d_sent_ms_next=p + 12 * s, d_seq0_next=p + 70000 + 4 * nflows,
             d_rec0_next=p + 70000 + 12 * nflows, stream=None)
    a.update(kw)
    return list(a.values())


def build_args(p, **kw):
    a = dict(d_base=p, base_bytes=4096, d_offsets=p, d_lengths=p, nrec=9, d_seq0=p, d_rec0=p, d_rec_end=p, nflows=3, window=5,
             d_acked=p, d_sent_ms=p, now_ms=1, timeout_ms=1, flags=0, d_wire=p, wire_stride=1472, max_sel=15, d_sel=p,
             d_wire_len=p, d_crc_out=p, d_counts=p, d_work=p, work_bytes=1 << 16, stream=None)
    a.update(kw)
    return list(a.values())


def test_symbols_header_binding_and_constants():
    import wtp_crc32 as W
    for name in NAMES:
        assert name in W.EXPORTED and getattr(W.LIB, name).argtypes is not None
    assert W.tx_ingest_acks_flows.__doc__ and W.tx_advance_flows.__doc__ and W.tx_build_retransmit_var_flows.__doc__
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)

    def params(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", decl)
        assert m, name
        return [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]

    assert params(NAMES[0]) == ["d_dgrams", "stride", "d_recv_len", "d_flow", "n", "mode", "d_seq0", "d_rec0", "d_rec_end",
                                "nflows", "window", "d_acked", "d_ok", "d_hit", "d_flow_adv", "d_flow_fresh", "stream"]
    assert params(NAMES[1]) == ["d_acked", "d_sent_ms", "nflows", "window", "d_flow_adv", "fill_ms", "d_seq0", "d_rec0",
                                "d_acked_next", "d_sent_ms_next", "d_seq0_next", "d_rec0_next", "stream"]
    assert params(NAMES[2]) == ["d_base", "base_bytes", "d_offsets", "d_lengths", "nrec", "d_seq0", "d_rec0", "d_rec_end",
                                "nflows", "window", "d_acked", "d_sent_ms", "now_ms", "timeout_ms", "flags", "d_wire",
                                "wire_stride", "max_sel", "d_sel", "d_wire_len", "d_crc_out", "d_counts", "d_work", "work_bytes",
                                "stream"]
    assert [len(getattr(W.LIB, n).argtypes) for n in NAMES] == [17, 13, 25]
    limits = dict(re.findall(r"#define (WTP_TX_MAX_\w+)\s+\(1u << (\d+)\)", src))
    assert {k: 1 << int(v) for k, v in limits.items()} == {"WTP_TX_MAX_INFLIGHT": W.TX_MAX_INFLIGHT, "WTP_TX_MAX_FLOWS": W.TX_MAX_FLOWS,
                                                           "WTP_TX_MAX_FLOW_SLOTS": W.TX_MAX_FLOW_SLOTS}
    assert W.TX_MAX_FLOWS == MAXF and W.TX_MAX_FLOW_SLOTS == MAXS == W.TX_MAX_INFLIGHT
    assert "k_txf_emit" in src and "k_txf_select" in src and "k_txf_advance" in src
    # no new *_work_bytes export: the build's scratch is wtp_tx_work_bytes(nflows * window, max_sel)
    assert not [n for n in W.EXPORTED if "flows" in n and n.startswith("wtp_tx") and n.endswith("_work_bytes")]


LIMITS = {
    "nflows": dict(nflows=MAXF + 1, window=0),
    "window": dict(nflows=0, window=MAXW + 1),
    "slots": dict(nflows=1025, window=1024),
    "slots, product past 2^32": dict(nflows=1 << 20, window=1 << 20),
}


def collect(L, fn, make, p, cases):
    msgs = {}
    for name, kw in cases.items():
        assert fn(*make(p, **kw)) == EINVAL, name
        msgs[name] = L.wtp_last_error().decode()
        assert msgs[name], name
    return msgs


def distinct(msgs, shared=()):
    """One message per case; the cases named in `shared` are two ways into the case before the comma."""
    kinds = {k.split(",")[0] for k in msgs}
    assert len({msgs[k] for k in kinds}) == len(kinds), msgs
    for k in shared:
        assert msgs[k].split(">")[1] == msgs[k.split(",")[0]].split(">")[1]


def test_ingest_flows_einval(L, p):
    cases = dict(LIMITS, **{
        "n": dict(n=1 << 31), "mode": dict(mode=2), "stride": dict(stride=15),
        "d_flow_adv": dict(d_flow_adv=None), "d_flow_fresh": dict(d_flow_fresh=None),
        "d_seq0": dict(d_seq0=None), "d_rec0": dict(d_rec0=None), "d_rec_end": dict(d_rec_end=None),
        "d_acked": dict(d_acked=None),
        "d_dgrams": dict(d_dgrams=None), "d_recv_len": dict(d_recv_len=None), "d_flow": dict(d_flow=None), "d_ok": dict(d_ok=None)})
    msgs = collect(L, L.wtp_tx_ingest_acks_flows, ingest_args, p, cases)
    distinct(msgs, ["slots, product past 2^32"])
    for ptr in [k for k in cases if k.startswith("d_")]:
        assert "null" in msgs[ptr] and ptr in msgs[ptr]
    # in the header's order: the batch, the mode, the stride, the limits, the per-flow arrays, the state, the ring
    order = [("n", dict(n=1 << 31)), ("mode", dict(mode=9)), ("stride", dict(stride=0)), ("nflows", dict(nflows=MAXF + 1)),
             ("d_flow_adv", dict(d_flow_adv=None)), ("d_seq0", dict(d_seq0=None)), ("d_acked", dict(d_acked=None)),
             ("d_ok", dict(d_ok=None))]
    for i, (why, _) in enumerate(order):
        kw = {}
        for _, more in order[i:]:
            kw.update(more)
        assert L.wtp_tx_ingest_acks_flows(*ingest_args(p, **kw)) == EINVAL and why in L.wtp_last_error().decode(), why
    # what a shape does not need may be NULL
    assert L.wtp_tx_ingest_acks_flows(*ingest_args(p, n=0, nflows=0, d_dgrams=None, d_recv_len=None, d_flow=None, d_ok=None,
                                                   d_seq0=None, d_rec0=None, d_rec_end=None, d_acked=None, d_flow_adv=None,
                                                   d_flow_fresh=None)) == 0
    assert L.wtp_tx_ingest_acks_flows(*ingest_args(p, nflows=0, window=MAXW, d_acked=None, d_ok=None)) == EINVAL
    assert "d_ok" in L.wtp_last_error().decode()  # no flows: d_acked is not needed, the ring still is
    assert L.wtp_tx_ingest_acks_flows(*ingest_args(p, window=0, d_acked=None, d_flow_fresh=None)) == EINVAL
    assert "d_flow_fresh" in L.wtp_last_error().decode()  # no slots: the per-flow results are still written


def test_advance_flows_einval(L, p):
    cases = dict(LIMITS, **{
        "seq0 pair": dict(d_seq0=None), "seq0_next pair": dict(d_seq0_next=None), "rec0 pair": dict(d_rec0=None),
        "rec0_next pair": dict(d_rec0_next=None), "one pair": dict(d_seq0=None, d_seq0_next=None),
        "d_flow_adv": dict(d_flow_adv=None), "d_acked": dict(d_acked=None), "d_sent_ms": dict(d_sent_ms=None),
        "d_acked_next": dict(d_acked_next=None), "d_sent_ms_next": dict(d_sent_ms_next=None)})
    msgs = collect(L, L.wtp_tx_advance_flows, advance_args, p, cases)
    distinct(msgs, ["slots, product past 2^32"])
    for ptr in [k for k in cases if k.startswith("d_")]:
        assert f"null pointer: {ptr} " in msgs[ptr]
    assert "d_seq0_next without d_seq0" in msgs["seq0 pair"] and "d_rec0 without d_rec0_next" in msgs["rec0_next pair"]
    base = dict(zip(("d_acked", "d_sent_ms", "nflows", "window", "d_flow_adv", "fill_ms", "d_seq0", "d_rec0", "d_acked_next",
                     "d_sent_ms_next", "d_seq0_next", "d_rec0_next"), advance_args(p)))
    # an output range over an input range or the other output by one element, either way round, and the same array;
    # the arrays lie 4 KiB apart here, so that the moved one meets one other array only
    apart = {k: p + 4096 * (i + 1) for i, k in enumerate(k for k in base if k.startswith("d_"))}
    base.update(apart)
    over = set()
    pairs = [("d_acked_next", "d_acked"), ("d_acked_next", "d_sent_ms"), ("d_sent_ms_next", "d_acked"),
             ("d_sent_ms_next", "d_sent_ms"), ("d_sent_ms_next", "d_acked_next"), ("d_seq0_next", "d_seq0"),
             ("d_seq0_next", "d_rec0"), ("d_seq0_next", "d_flow_adv"), ("d_rec0_next", "d_seq0"), ("d_rec0_next", "d_rec0"),
             ("d_rec0_next", "d_flow_adv"), ("d_rec0_next", "d_seq0_next")]
    for out, other in pairs:
        size = 4 * (3 if "0" in out else 15)
        for at in (base[other] + size - 4, base[other] - size + 4, base[other]):
            assert L.wtp_tx_advance_flows(*advance_args(p, **dict(apart, **{out: at}))) == EINVAL, (out, other, at)
            assert f"{out} overlaps {other}" in L.wtp_last_error().decode(), (out, other, L.wtp_last_error())
            over.add(L.wtp_last_error().decode())
    assert len(over) == len(pairs)
    # the limits come first, then the pairs, then the pointers, then the overlaps
    assert L.wtp_tx_advance_flows(*advance_args(p, nflows=MAXF + 1, d_seq0=None, d_flow_adv=None)) == EINVAL
    assert "nflows" in L.wtp_last_error().decode()
    assert L.wtp_tx_advance_flows(*advance_args(p, d_seq0=None, d_flow_adv=None)) == EINVAL
    assert "without" in L.wtp_last_error().decode()
    assert L.wtp_tx_advance_flows(*advance_args(p, d_flow_adv=None, d_acked_next=base["d_acked"])) == EINVAL
    assert "d_flow_adv" in L.wtp_last_error().decode()
    assert L.wtp_tx_advance_flows(*advance_args(p, window=0, d_rec0=None)) == EINVAL  # a pair is a pair whatever the shape


def test_build_flows_einval(L, p):
    need = L.wtp_tx_work_bytes(15, 15)
    cases = dict(LIMITS, **{
        "wire_stride": dict(wire_stride=1471), "work_bytes": dict(work_bytes=need - 1),
        "d_counts": dict(d_counts=None), "d_counts, d_work": dict(d_work=None),
        "d_base": dict(d_base=None), "d_base, d_offsets": dict(d_offsets=None), "d_base, d_lengths": dict(d_lengths=None),
        "d_acked": dict(d_acked=None), "d_acked, d_sent_ms": dict(d_sent_ms=None),
        "d_seq0": dict(d_seq0=None), "d_seq0, d_rec0": dict(d_rec0=None), "d_seq0, d_rec_end": dict(d_rec_end=None),
        "d_wire": dict(d_wire=None)})
    for k in LIMITS:
        cases[k] = dict(cases[k], work_bytes=1 << 40)
    msgs = collect(L, L.wtp_tx_build_retransmit_var_flows, build_args, p, cases)
    kinds = {k.split(",")[0] for k in msgs}
    assert len({msgs[k] for k in kinds}) == len(kinds) == 10, msgs
    for k in msgs:
        if k.startswith("d_"):
            assert "null" in msgs[k] and k.split(", ")[-1] in msgs[k] and msgs[k] == msgs[k.split(",")[0]]
    assert f"work_bytes {need - 1} < {need}" in msgs["work_bytes"]
    assert L.wtp_tx_build_retransmit_var_flows(*build_args(p, work_bytes=need, d_counts=None)) == EINVAL
    assert "d_counts" in L.wtp_last_error().decode()  # exactly wtp_tx_work_bytes(nflows * window, max_sel) is enough
    # in the header's order
    order = [("wire_stride", dict(wire_stride=16)), ("window", dict(window=MAXW + 1)), ("work_bytes", dict(work_bytes=0)),
             ("d_counts", dict(d_counts=None)), ("d_base", dict(d_lengths=None)), ("d_acked", dict(d_acked=None)),
             ("d_seq0", dict(d_rec_end=None)), ("d_wire", dict(d_wire=None))]
    for i, (why, _) in enumerate(order):
        kw = {}
        for _, more in reversed(order[i:]):
            kw.update(more)
        if i > 1:
            kw.pop("window", None)
        assert L.wtp_tx_build_retransmit_var_flows(*build_args(p, **kw)) == EINVAL and why in L.wtp_last_error().decode(), why
    # what a shape does not need may be NULL and is then not the reason
    for kw, why in ((dict(nflows=0, d_base=None, d_offsets=None, d_lengths=None, d_acked=None, d_sent_ms=None, d_seq0=None,
                          d_rec0=None, d_rec_end=None, d_wire=None, d_counts=None), "d_counts"),
                    (dict(window=0, d_base=None, d_acked=None, d_seq0=None, d_wire=None, d_work=None), "d_work"),
                    (dict(max_sel=0, d_wire=None, d_work=None), "d_work")):
        assert L.wtp_tx_build_retransmit_var_flows(*build_args(p, **kw)) == EINVAL and why in L.wtp_last_error().decode()


def test_valid_without_device(L, p):
    """What launches nothing returns WTP_OK without a device, at the limits too; the limits
    themselves pass the limit checks, so their refusal is the next check's."""
    assert L.wtp_tx_advance_flows(None, None, 0, 0, None, 0, None, None, None, None, None, None, None) == 0
    assert L.wtp_tx_advance_flows(*advance_args(p, nflows=0)) == 0
    assert L.wtp_tx_advance_flows(*advance_args(p, window=0)) == 0
    assert L.wtp_tx_advance_flows(None, None, MAXF, 0, None, 0, None, None, None, None, None, None, None) == 0
    assert L.wtp_tx_advance_flows(None, None, 0, MAXW, None, 0, None, None, None, None, None, None, None) == 0
    assert L.wtp_tx_ingest_acks_flows(None, 16, None, None, 0, 1, None, None, None, 0, MAXW, None, None, None, None, None, None) == 0
    for nf, w in ((MAXF, 1), (1, MAXW), (1024, 1024)):
        assert L.wtp_tx_advance_flows(*advance_args(p, nflows=nf, window=w, d_flow_adv=None)) == EINVAL
        assert "d_flow_adv" in L.wtp_last_error().decode()
        assert L.wtp_tx_ingest_acks_flows(*ingest_args(p, nflows=nf, window=w, d_acked=None)) == EINVAL
        assert "d_acked" in L.wtp_last_error().decode()
        need = L.wtp_tx_work_bytes(nf * w, 7)
        assert L.wtp_tx_build_retransmit_var_flows(*build_args(p, nflows=nf, window=w, max_sel=7, work_bytes=need,
                                                               d_counts=None)) == EINVAL
        assert "d_counts" in L.wtp_last_error().decode()
        assert L.wtp_tx_build_retransmit_var_flows(*build_args(p, nflows=nf, window=w, max_sel=7, work_bytes=need - 1)) == EINVAL
        assert "work_bytes" in L.wtp_last_error().decode()
