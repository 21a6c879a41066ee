"""CPU tests of the CRC fold: the model (tests/concat_model.py) against the reference's
crc32 on real bytes, the host entry point wtp_crc32_combine against the model, the new
symbols of the C-ABI, and wSender / wReceiver --digest over loopback with --crc cpu."""
import os
import socket
import subprocess
import time

import numpy as np
import pytest

import concat_model as M
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "a3-reliable-transport_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("wtp_crc32_combine", "wtp_crc32_concat_work_bytes", "wtp_crc32_concat",
               "wtp_crc32_buffer_work_bytes", "wtp_crc32_buffer", "wtp_crc32_host_buffer")
LENS = (0, 1, 15, 16, 17, 1455, 1456, 4096)


@pytest.fixture(scope="module")
def W():
    import wtp_crc32 as W
    return W


@pytest.fixture(scope="module")
def parts():
    """One byte string per length in LENS (distinct contents) with its reference CRC."""
    return {n: (b, O.crc32(b)) for n in LENS for b in [O.synth_fill_np(n, start_byte=7 * n + 1).tobytes()]}


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbols_exported(W, name):
    assert name in W.EXPORTED
    assert getattr(W.LIB, name) is not None


def test_work_sizes(W):
    for n in (0, 1, 4097, 1 << 20, 1 << 40):
        assert 0 < W.concat_work_bytes(n) <= 65536
    for nbytes in (0, 1, 1456, 1457, 1 << 30):
        assert W.buffer_work_bytes(nbytes) == W.concat_work_bytes(0) + 4 * ((nbytes + 1455) // 1456)


def test_order_of_x():
    """x^(8 (2^32 - 1)) = 1: what lets byte counts be carried mod 2^32 - 1."""
    assert M.xpow8(M.ORDER) == M.ONE
    assert M.xpow8(1) == M.ONE >> 8 and M.mulmod(0x12345678, M.ONE) == 0x12345678


def test_model_combine_matches_reference(parts):
    for la, (a, ca) in parts.items():
        for lb, (b, cb) in parts.items():
            want = O.crc32(a + b)
            assert M.combine(ca, cb, lb) == want, (la, lb)
            assert O.combine(ca, cb, lb) == want, (la, lb)


def _forty_parts():
    rng = np.random.default_rng(40)
    lens = [int(x) for x in rng.integers(1, 3000, 40)]
    for i in (0, 7, 8, 39):
        lens[i] = 0
    lens[3], lens[20] = 1456, 4096
    return [O.synth_fill_np(n, start_byte=5000 * i).tobytes() for i, n in enumerate(lens)]


def test_model_concat_matches_reference():
    chunks = _forty_parts()
    want = O.crc32(b"".join(chunks))
    crcs, lens = [O.crc32(c) for c in chunks], [len(c) for c in chunks]
    assert M.concat_fold(crcs, lens) == want
    assert M.concat_var(crcs, lens) == want
    fixed = [O.synth_fill_np(1456, start_byte=9 * i).tobytes() for i in range(9)] + [b"tail"]
    assert M.concat_fixed([O.crc32(c) for c in fixed], 1456, 4) == O.crc32(b"".join(fixed))
    assert M.concat_fixed([], 1456, 4) == 0 and M.concat_var([], []) == 0


def test_model_forms_agree_on_long_lengths():
    """The tree (fixed), the suffix-sum form (var) and the left fold agree where the
    reference cannot go: lengths of 2^31, 2^32 - 1 and 2^32 + 5."""
    rng = np.random.default_rng(3)
    crcs = rng.integers(0, 1 << 32, 37, dtype=np.uint64).astype(np.uint32)
    for length, last in ((2**32 + 5, 1), (0xFFFFFFFF, 0), (0x80000000, 0x80000000), (0, 0)):
        lens = [length] * 36 + [last]
        want = M.concat_fold(crcs, lens)
        assert M.concat_fixed(crcs, length, last) == want
        assert M.concat_var(crcs, np.array([x % M.ORDER for x in lens], dtype=np.uint64)) == want


def test_host_combine_matches_model(W, parts):
    for la, (a, ca) in parts.items():
        for lb, (b, cb) in parts.items():
            assert W.crc32_combine(ca, cb, lb) == M.combine(ca, cb, lb) == O.crc32(a + b)
    chunks = _forty_parts()
    d = 0
    for c in chunks:
        d = W.crc32_combine(d, O.crc32(c), len(c))
    assert d == O.crc32(b"".join(chunks))


def test_host_combine_identities(W):
    a, b, c = 0xDEADBEEF, 0x0BADF00D, 0xCBF43926
    assert W.crc32_combine(c, 0, 0) == c
    for ln in (0, 1, 1456, 2**32 + 5, 2**64 - 1):
        assert W.crc32_combine(0, c, ln) == c
        assert W.crc32_combine(a, b, ln) == M.combine(a, b, ln)
    assert W.crc32_combine(a, b, 2**32 - 1) == a ^ b  # the order of x
    assert W.crc32_combine(a, b, 5 * 2**32 + 7) == W.crc32_combine(a, b, 12)


# ---- wSender / wReceiver --digest --------------------------------------------------
def _free_port():
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wait_bound(proc, port, limit=10.0):
    """Until the receiver's UDP port shows in /proc/net/udp (no fixed sleep)."""
    needle = ":%04X " % port
    end = time.monotonic() + limit
    while time.monotonic() < end and proc.poll() is None:
        with open("/proc/net/udp") as f:
            if any(needle in line.split(None, 2)[1] + " " for line in list(f)[1:]):
                return
        time.sleep(0.005)
    raise AssertionError("wReceiver did not bind its port")


@pytest.fixture(scope="module")
def binaries():
    if not (os.path.exists(os.path.join(BIN, "wSender")) and os.path.exists(os.path.join(BIN, "wReceiver"))):
        subprocess.run(["make", "-C", os.path.join(ROOT, "a3-reliable-transport_amd"), "apps"], check=True)
    return BIN


def digest_transfer(bindir, src, tmp, crc="cpu", digest=True, window=10, env=None):
    """One loopback transfer; returns (received bytes, sender stdout, receiver stdout)."""
    env = dict(os.environ, **(env or {}))
    rport = _free_port()
    outdir = os.path.join(tmp, "out")
    os.makedirs(outdir, exist_ok=True)
    flag = ["--digest"] if digest else []
    recv = subprocess.Popen([os.path.join(bindir, "wReceiver"), "-p", str(rport), "-w", str(window), "-d", outdir,
                             "-o", os.path.join(tmp, "receiver.log"), "--crc", crc, "--once"] + flag,
                            stdout=subprocess.PIPE, text=True, env=env)
    try:
        _wait_bound(recv, rport)
        s = subprocess.run([os.path.join(bindir, "wSender"), "-h", "127.0.0.1", "-p", str(rport), "-w", str(window),
                            "-i", src, "-o", os.path.join(tmp, "sender.log"), "--crc", crc] + flag,
                           timeout=60, capture_output=True, text=True, env=env)
        assert s.returncode == 0, s.stderr
        rout, _ = recv.communicate(timeout=10)
        assert recv.returncode == 0
    finally:
        if recv.poll() is None:
            recv.kill()
    with open(os.path.join(outdir, "FILE-0.out"), "rb") as f:
        return f.read(), s.stdout, rout


def check_digest(data, got, sout, rout, crc):
    """Both endpoints print the same digest line, equal to the reference's CRC of the file."""
    assert got == data
    want = "digest %d %08X" % (len(data), O.crc32(data))
    nchunks = (len(data) + 1455) // 1456
    assert sout.splitlines() == ["sent %d bytes in %d DATA packets (crc %s)" % (len(data), nchunks, crc), want]
    assert rout.splitlines() == [want]


def _blob(tmp_path, nbytes):
    src = os.path.join(str(tmp_path), "blob%d.bin" % nbytes)
    with open(src, "wb") as f:
        f.write(O.synth_fill_np(nbytes, start_byte=321).tobytes())
    return src


@pytest.mark.parametrize("what", ["input.txt", 60_000, 2 * 1456, 0])
def test_digest_loopback_cpu(binaries, tmp_path, what):
    """A sample file, a 60 000-byte blob (short last chunk), exactly two full chunks, and
    the empty file (digest 0 00000000)."""
    src = os.path.join(GOLD, what) if isinstance(what, str) else _blob(tmp_path, what)
    data = open(src, "rb").read()
    check_digest(data, *digest_transfer(binaries, src, str(tmp_path)), "cpu")


def test_no_digest_flag_stdout_unchanged(binaries, tmp_path):
    src = _blob(tmp_path, 60_000)
    got, sout, rout = digest_transfer(binaries, src, str(tmp_path), digest=False)
    assert got == open(src, "rb").read()
    assert sout == "sent 60000 bytes in 42 DATA packets (crc cpu)\n"
    assert rout == ""
