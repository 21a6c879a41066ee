"""CPU checks of the mixed-length DATA builder (wtp_build_data_packets_var): the sequential
model against the oracle's datagrams, and the C-ABI's argument validation, which needs no
device."""
import ctypes as C
import os
import re

import numpy as np

import buildvar_model as M
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5


def _file(golden_dir):
    return np.frombuffer(open(os.path.join(golden_dir, "input3.txt"), "rb").read(), dtype=np.uint8)


def test_model_on_irregular_records_matches_the_oracle_per_record(golden_dir):
    """input3.txt cut at irregular lengths (0 and 1456 among them): every slot is the
    oracle's datagram, the slot's tail and the lengths / CRCs are as the header says."""
    data = _file(golden_dir)
    rng = np.random.default_rng(0xB1D)
    lens = [0, 1, 1456, 3, 0, 17]
    while sum(lens) + 1456 < data.size:
        lens.append(int(rng.integers(0, 1457)))
    lens.append(data.size - sum(lens))
    lens = np.array(lens, dtype=np.uint32)
    assert lens.max() <= 1456 and int(lens.sum()) == data.size and lens.size > 8
    offs = M.packed_offsets(lens)
    stride, seq0 = 1480, 0xFFFFFFFA  # the sequence numbers wrap inside the batch
    prior = np.full(lens.size * stride + 7, SENT, dtype=np.uint8)
    wire, wl, crc = M.build(data, data.size, offs, lens, seq0, prior, stride)
    assert (prior == SENT).all()  # the model does not touch the caller's image
    for i, (o, ln) in enumerate(zip(offs.tolist(), lens.tolist())):
        payload = data[o:o + ln].tobytes()
        d = O.build_datagram((seq0 + i) & 0xFFFFFFFF, payload)
        slot = wire[i * stride:(i + 1) * stride]
        assert slot[:16 + ln].tobytes() == d and (slot[16 + ln:] == SENT).all()
        assert d[:16] == np.array([2, (seq0 + i) & 0xFFFFFFFF, ln, O.crc32(payload)], dtype=">u4").tobytes()
        assert wl[i] == 16 + ln and crc[i] == O.crc32(payload)
    assert (wire[lens.size * stride:] == SENT).all()


def test_model_of_1456_chunks_matches_the_fixed_builders_datagrams(golden_dir):
    """Offsets i * 1456 and the fixed builder's lengths give what wtp_build_data_packets is
    specified to write: the oracle's datagram of every chunk, the last one short."""
    data = _file(golden_dir)
    total = data.size - (data.size % 1456 == 0)  # a short last chunk
    n = (total + 1455) // 1456
    offs = np.arange(n, dtype=np.uint64) * 1456
    lens = np.minimum(1456, total - offs.astype(np.int64)).astype(np.uint32)
    assert n > 2 and 0 < lens[-1] < 1456
    wire, wl, crc = M.build(data, total, offs, lens, 7, np.zeros(n * 1472, np.uint8), 1472)
    want = b"".join(O.build_datagram(7 + i, data[i * 1456:min((i + 1) * 1456, total)].tobytes()).ljust(1472, b"\0")
                    for i in range(n))
    assert wire.tobytes() == want
    assert np.array_equal(wl, lens + 16) and np.array_equal(crc, O.batch_var(data, offs, lens))


def test_model_leaves_invalid_entries_alone():
    base = O.synth_fill_np(5000)
    nb = 4000  # base_bytes below the array's size: the rule is about base_bytes
    offs = np.array([0, 10, nb, nb, nb + 1, nb - 5, nb - 5, 2 ** 40, 100, 100], dtype=np.uint64)
    lens = np.array([1457, 0xFFFFFFFF, 1, 0, 0, 6, 5, 1, 4097, 1456], dtype=np.uint32)
    valid = [False, False, False, True, False, False, True, False, False, True]
    assert [M.is_valid(int(o), int(ln), nb) for o, ln in zip(offs, lens)] == valid
    prior = np.full(10 * 1472, SENT, dtype=np.uint8)
    wire, wl, crc = M.build(base, nb, offs, lens, 0, prior, 1472)
    for i, v in enumerate(valid):
        slot = wire[i * 1472:(i + 1) * 1472]
        if v:
            assert slot[:16 + lens[i]].tobytes() == O.build_datagram(i, base[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes())
            assert wl[i] == 16 + lens[i]
        else:
            assert (slot == SENT).all() and wl[i] == 0 and crc[i] == 0
    assert wl[3] == 16 and crc[3] == 0  # the empty payload at offset == base_bytes


def test_build_var_argument_validation_without_device():
    import wtp_crc32 as W
    L = W.LIB
    assert "wtp_build_data_packets_var" in W.EXPORTED and hasattr(L, "wtp_build_data_packets_var")
    buf = (C.c_uint32 * 64)()
    a = C.addressof(buf)

    def call(**kw):
        args = dict(base=a, base_bytes=256, offsets=a, lengths=a, n=1, seq0=0, wire=a, wire_stride=1472, wire_len=a,
                    crc_out=a)
        args.update(kw)
        return L.wtp_build_data_packets_var(*args.values(), None)

    assert call(wire_stride=1471) == -1 and b"wire_stride 1471 < 1472" in L.wtp_last_error()
    assert call(n=1 << 31) == -1 and b"n 2147483648 >= 2^31" in L.wtp_last_error()
    assert call(n=(1 << 40) + 5) == -1 and b"2^31" in L.wtp_last_error()
    for hole in ("base", "offsets", "lengths", "wire"):
        assert call(**{hole: None}) == -1 and b"null" in L.wtp_last_error(), hole
    # n == 0: nothing to do, no pointer is needed, no device is touched
    assert call(n=0) == 0
    assert L.wtp_build_data_packets_var(None, 0, None, None, 0, 0, None, 1472, None, None, None) == 0


def test_build_var_is_declared_in_the_header():
    src = open(os.path.join(ROOT, "include", "wtp_crc32.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+wtp_build_data_packets_var\s*\(([^)]*)\)", decl)
    assert m, "wtp_build_data_packets_var is not declared"
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["d_base", "base_bytes", "d_offsets", "d_lengths", "n", "seq0", "d_wire", "wire_stride",
                      "d_wire_len", "d_crc_out", "stream"]
    assert "k_build_var" in src
