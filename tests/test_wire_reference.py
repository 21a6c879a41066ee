"""The restatements of the wire format and of the selective sender window against what the
reference's own code produced: tests/golden/wire.json, recorded from cpp/src/base/Packet.cpp,
cpp/src/opt/Packet.cpp and cpp/src/opt/Window.cpp by tests/golden/make_wire_golden.py.  No
test here reads the reference; the last one replays the fixture through the compiled shim
where oracle/_ref was built."""
import numpy as np
import pytest

import ack_model as A
import oracle as O
import retx_model as R
import wire_golden as G

M32 = 0xFFFFFFFF
TYPES = [0, 1, 2, 3, 7, 0x00000102, 0x00010002, 0x01000002, 0x02000000, 0x00000200, 0x80000002, 0xFFFFFF02, 0x02020202,
         0x00000103, 0x03000000, 0x80000003, 0x03030303]
SEQS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
LENS = [0, 1, 15, 16, 17, 1455, 1456]


def _records():
    """(header, start_byte, size, [type, seqNum, length, checksum, calculateCheckSum()])."""
    return [(bytes.fromhex(r[0]), r[1], r[2], r[3:]) for r in G.load()["parse"]["records"]]


def _distance(trace, seq):
    return (seq - trace["seq0"]) & M32


# ---- non-vacuity ----------------------------------------------------------------------------
def test_corpus_covers_every_type_word_sequence_number_and_length():
    g = G.load()
    assert g["types"] == TYPES and g["seqs"] == SEQS and g["lens"] == LENS
    assert sorted(G.corpus()) == sorted((t, s, ln) for t in TYPES for s in SEQS for ln in LENS)
    assert len(g["datagrams"]) == len(TYPES) * len(SEQS) * len(LENS)  # no entry twice
    for (t, s, ln), (sb, hdr) in G.corpus().items():
        assert len(hdr) == 16 and len(G.payload(sb, ln)) == ln
    # the adversarial words: a right low byte under wrong upper bytes, and the byte-swapped constants
    assert {t & 0xFF for t in TYPES if t > 255} == {0, 2, 3} and 0x02000000 in TYPES and 0x03000000 in TYPES


def test_parse_records_hold_agreeing_and_disagreeing_length_fields():
    recs = _records()
    agree = [r for r in recs if r[3][2] == r[2] - 16]
    wrong = [r for r in recs if r[3][2] != r[2] - 16]
    assert len(agree) >= 5 * 5 * 3 and len(wrong) >= 12
    assert {r[3][2] for r in wrong} >= {0, 1457} and any(r[3][2] == r[2] - 16 + 1 for r in wrong)
    assert {r[3][0] for r in agree} >= {2, 3, 0x00000102, 0x02000000} and {r[3][1] for r in agree} == set(SEQS)


def test_window_traces_cover_the_cases():
    traces = G.load()["window"]
    assert len(traces) >= 12
    assert {(t["seq0"], t["inflight"]) for t in traces} == {(s, i) for s in (0, 0xFFFFFFF0) for i in (1, 10, 64)}
    for t in traces:
        d = [_distance(t, a) for a in t["acks"]]
        inwin = [x for x in d if x < t["inflight"]]
        assert inwin and len(inwin) > len(set(inwin))                      # in-window, one of them again
        assert any(x >= 0x80000000 for x in d)                             # below the window
        assert any(t["inflight"] <= x < 0x80000000 for x in d)             # at or above its end
        assert len(t["acked"]) == t["inflight"]
    assert any(t["advance"] == 0 for t in traces)
    assert any(t["advance"] == t["inflight"] for t in traces if t["inflight"] > 1)
    assert any(0 < t["advance"] < t["inflight"] for t in traces)
    assert any(t["seq0"] + t["inflight"] > M32 for t in traces)            # a window across the wrap


# ---- header writers -------------------------------------------------------------------------
def test_build_datagram_reproduces_every_recorded_datagram():
    for (t, s, ln), (sb, hdr) in G.corpus().items():
        assert O.build_datagram(s, G.payload(sb, ln), ptype=t) == hdr + G.payload(sb, ln), (hex(t), hex(s), ln)


def test_ack_builders_reproduce_the_type_3_entries():
    for (t, s, ln), (sb, hdr) in G.corpus().items():
        if t != 3:
            continue
        pay = G.payload(sb, ln)
        assert R.ack_datagram(s, checksum=int.from_bytes(hdr[12:], "big"), payload=pay) == hdr + pay
        if ln == 0:  # what a receiver sends: an empty payload, whose CRC is 0
            assert R.ack_datagram(s) == hdr
    empty = [G.corpus()[3, s, 0][1] for s in SEQS]
    assert A.ack_bytes(np.array(SEQS, dtype=np.uint32)).tobytes() == b"".join(empty)


# ---- header readers -------------------------------------------------------------------------
def test_header_readers_agree_with_the_parse_records():
    recs = _records()
    stride = 16 + 1456
    dgrams = [hdr + G.payload(sb, size - 16) for hdr, sb, size, _ in recs]
    ring, rl = R.make_ring(dgrams, stride)
    want = np.array([out for _, _, _, out in recs], dtype=np.uint32)
    for headers in (A.headers, R.headers):
        types, seqs = headers(ring, stride, len(recs))
        assert np.array_equal(types, want[:, 0]) and np.array_equal(seqs, want[:, 1])
    ok, crc = O.verify_datagrams(ring, stride, rl)
    agree = want[:, 2] == rl - 16
    assert agree.sum() >= 75 and (~agree).sum() >= 12
    # where the length field is the buffer's: the reference's own verdict, field by field
    assert np.array_equal(crc[agree], want[agree, 4])
    assert np.array_equal(ok[agree], (want[agree, 3] == want[agree, 4]).astype(np.uint8)) and ok[agree].all()
    # where it is not, the field is ignored: the CRC still covers bytes [16, recv_len) and the verdict stands
    # (Packet::calculateCheckSum() would cover header.length bytes; the reference's receivers do not call it)
    assert ok[~agree].all()
    assert np.array_equal(crc[~agree], want[~agree, 3])
    assert (want[~agree, 4] != want[~agree, 3]).any()


# ---- the selective sender window ------------------------------------------------------------
@pytest.mark.parametrize("vectorised", [False, True])
def test_selective_ingest_reproduces_every_window_trace(vectorised):
    for t in G.load()["window"]:
        ring, rl = R.make_ring([R.ack_datagram(a) for a in t["acks"]], 16)
        ok, hit, acked, (advance, newly) = R.ingest(ring, 16, rl, R.SELECTIVE, t["seq0"], t["inflight"],
                                                    np.zeros(t["inflight"], np.uint32), vectorised=vectorised)
        assert ok.all()
        assert "".join(str(int(a)) for a in acked) == t["acked"], t
        assert advance == t["advance"] and newly == t["acked"].count("1")
        # an ACK the reference does not find in its window is one the model does not count
        assert [h != R.NOT_PLACED for h in hit] == [_distance(t, a) < t["inflight"] for a in t["acks"]]


# ---- the fixture against the live reference -------------------------------------------------
def test_compiled_reference_reproduces_the_fixture():
    libs = [O.ref_packet_lib(v) for v in ("base", "opt")]
    if None in libs:
        pytest.skip("oracle/_ref not built (reference tree absent)")
    for (t, s, ln), (sb, hdr) in G.corpus().items():
        for r in libs:
            assert O.ref_build_datagram(r, t, s, G.payload(sb, ln)) == hdr + G.payload(sb, ln)
    for hdr, sb, size, out in _records():
        for r in libs:
            assert O.ref_parse_datagram(r, hdr + G.payload(sb, size - 16)) == out
    for t in G.load()["window"]:
        flags, adv = O.ref_window_run(libs[1], t["seq0"], t["inflight"], t["acks"])
        assert "".join(str(int(f)) for f in flags) == t["acked"] and adv == t["advance"]
