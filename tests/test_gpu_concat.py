"""GPU tests of the whole-buffer CRC: wtp_crc32_concat against the square-and-multiply
model (tests/concat_model.py) on random uint32 words (the fold is linear, so arbitrary
words exercise it fully), wtp_crc32_buffer / wtp_crc32_host_buffer against the reference's
crc32 over the bytes.  Before every device call d_work is filled (0xFF unless said) and
d_out sits between two sentinel words."""
import os

import numpy as np
import pytest

import concat_model as M
import oracle as O
from gpu_support import capture, dev_s32, u32
from test_concat_model import GOLD, binaries, check_digest, digest_transfer  # noqa: F401 (binaries: fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
SENT = (0x5A5A5A5A, 0x3C3C3C3C)

# The first launch hands 256 threads x 16 CRCs = 4096 elements to one workgroup: fixed
# lengths fold the n - 1 payloads of the common length (one launch up to n = 4097, two
# from 4098), variable lengths all n (one launch up to 4096, two from 4097).  From
# 1024 workgroups x 4096 elements on, a thread's run grows beyond 16: 4 194 305 fixed
# elements (n = 4 194 306), 4 194 305 variable ones.
ONE_GROUP = 256 * 16
NS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, ONE_GROUP - 1, ONE_GROUP, ONE_GROUP + 1, ONE_GROUP + 2,
      65_537]
ALL_GROUPS = 1024 * ONE_GROUP
FIXED_LENS = [0, 1, 16, 1456, 4096, 2**32 + 5]


@pytest.fixture(scope="module")
def W():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import wtp_crc32 as W
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    return W


def _words(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


class Out:
    """One result word between two sentinels."""

    def __init__(self):
        self.t = dev_s32([SENT[0], 0x77777777, SENT[1]])
        self.ptr = self.t[1:2]

    def value(self):
        h = u32(self.t)
        assert (int(h[0]), int(h[2])) == SENT, "a word beside d_out was written"
        return int(h[1])


def concat(W, d_crc, d_len, n, length=0, last_len=0, fill=0xFF):
    work = torch.full((W.concat_work_bytes(n),), fill, dtype=torch.uint8, device="cuda")
    out = Out()
    W.crc32_concat(d_crc, d_len, n, out.ptr, length=length, last_len=last_len, work=work)
    torch.cuda.synchronize()
    return out.value()


def buffer(W, view, nbytes, fill=0xFF):
    work = torch.full((W.buffer_work_bytes(nbytes),), fill, dtype=torch.uint8, device="cuda")
    out = Out()
    W.crc32_buffer(view, nbytes, out.ptr, work=work)
    torch.cuda.synchronize()
    return out.value()


# ---- concat, fixed lengths -----------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_concat_fixed(W, n):
    crc = _words(n, 1000 + n)
    d = dev_s32(crc) if n else None
    for length in FIXED_LENS:
        for last in sorted({0, 1, length}):
            got = concat(W, d, None, n, length, last)
            assert got == M.concat_fixed(crc, length, last), (n, length, last)
            if n:
                assert W.LIB.wtp_last_kernel().decode() == "k_concat_fold"
    if n:
        assert np.array_equal(u32(d), crc)  # d_crc is only read


@pytest.mark.parametrize("n", [ALL_GROUPS + 1, ALL_GROUPS + 2, ALL_GROUPS + 12_345])
def test_concat_fixed_all_groups(W, n):
    """The last n of 16-element runs over 1024 workgroups, the first of 17, and a larger one."""
    crc = _words(n, n)
    assert concat(W, dev_s32(crc), None, n, 1456, 777) == M.concat_fixed(crc, 1456, 777)


# ---- concat, variable lengths ----------------------------------------------------------
def _var_lens(n, seed):
    lens = np.random.default_rng(seed).integers(0, 4097, n, dtype=np.uint64).astype(np.uint32)
    for k, v in ((n // 3, 0), (n // 2, 0x80000000), (n - 1, 0xFFFFFFFF), (n // 5, 0xFFFFFFFF), (2 * n // 3, 0)):
        if n > 4:
            lens[k] = v
    return lens


@pytest.mark.parametrize("n", NS)
def test_concat_var(W, n):
    crc, lens = _words(n, 2000 + n), _var_lens(n, 3000 + n)
    if n == 0:
        assert concat(W, None, dev_s32([0]), 0) == 0
        return
    d_crc, d_len = dev_s32(crc), dev_s32(lens)
    want = M.concat_var(crc, lens)
    assert concat(W, d_crc, d_len, n) == want
    assert W.LIB.wtp_last_kernel().decode() == "k_concat_var"
    assert concat(W, d_crc, d_len, n, fill=0x00) == want  # independent of d_work's contents
    # order matters: the reversed input gives the model's value for the reversed input
    rc, rl = crc[::-1].copy(), lens[::-1].copy()
    rwant = M.concat_var(rc, rl)
    assert concat(W, dev_s32(rc), dev_s32(rl), n) == rwant
    if n >= 63:
        assert rwant != want
    # all lengths zero: the XOR of the CRCs
    assert concat(W, d_crc, dev_s32(np.zeros(n, np.uint32)), n) == int(np.bitwise_xor.reduce(crc))
    assert np.array_equal(u32(d_crc), crc) and np.array_equal(u32(d_len), lens)


def test_concat_var_all_groups(W):
    """A thread run of 17 (more than 1024 workgroups' worth of 16-element runs).  Lengths
    1456 but for five entries, so the expected value is a fold of uniform segments."""
    n = ALL_GROUPS + 1
    crc = _words(n, 77)
    lens = np.full(n, 1456, dtype=np.uint32)
    special = {5: 0, n // 3: 0x80000000, n // 2: 0xFFFFFFFF, n - 4099: 3, n - 1: 0}
    for k, v in special.items():
        lens[k] = v
    want, a = 0, 0
    for k in sorted(special):
        want = M.combine(want, M.concat_fixed(crc[a:k], 1456, 1456), 1456 * (k - a))
        want = M.combine(want, int(crc[k]), special[k])
        a = k + 1
    assert a == n
    assert concat(W, dev_s32(crc), dev_s32(lens), n) == want


def test_concat_fixed_work_independent(W):
    n = 20_000
    crc = _words(n, 5)
    d = dev_s32(crc)
    want = M.concat_fixed(crc, 1456, 99)
    assert concat(W, d, None, n, 1456, 99, fill=0xFF) == want
    assert concat(W, d, None, n, 1456, 99, fill=0x00) == want


def test_bad_arguments(W):
    n = 100
    d = dev_s32(_words(n, 9))
    out = Out()
    need = W.concat_work_bytes(n)
    work = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def rejected(rc):
        return rc == -1 and W.LIB.wtp_last_error().decode() != ""

    L = W.LIB
    assert rejected(L.wtp_crc32_concat(d.data_ptr(), None, 1456, 1, n, work.data_ptr(), need - 1, out.ptr.data_ptr(), st))
    assert rejected(L.wtp_crc32_concat(d.data_ptr(), None, 1456, 1, n, None, need, out.ptr.data_ptr(), st))
    assert rejected(L.wtp_crc32_concat(d.data_ptr(), None, 1456, 1, n, work.data_ptr(), need, None, st))
    assert rejected(L.wtp_crc32_concat(None, None, 1456, 1, n, work.data_ptr(), need, out.ptr.data_ptr(), st))
    nbytes = 5000
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    bneed = W.buffer_work_bytes(nbytes)
    bwork = torch.zeros(bneed, dtype=torch.uint8, device="cuda")
    assert rejected(L.wtp_crc32_buffer(buf.data_ptr(), nbytes, bwork.data_ptr(), bneed - 1, out.ptr.data_ptr(), st))
    assert rejected(L.wtp_crc32_buffer(buf.data_ptr(), nbytes, bwork.data_ptr(), bneed, None, st))
    assert rejected(L.wtp_crc32_buffer(None, nbytes, bwork.data_ptr(), bneed, out.ptr.data_ptr(), st))
    torch.cuda.synchronize()
    assert out.value() == 0x77777777  # no rejected call wrote the result
    # the process goes on
    assert buffer(W, buf, nbytes) == O.crc32(bytes(nbytes))


# ---- buffer ------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, 1455, 1456, 1457, 1472, 2911, 2912, 4096, 4097, 65_536,
                                    1_000_003])
def test_buffer_sizes_and_alignments(W, nbytes):
    data = O.synth_fill_np(nbytes, start_byte=nbytes)
    want = O.crc32(data)
    for off in (0, 1, 8, 15):
        got = []
        for salt in (1, 2):  # two different surroundings of the same bytes
            host = np.random.default_rng(100 * off + salt).integers(0, 256, nbytes + off + 64, dtype=np.uint8)
            host[off:off + nbytes] = data
            alloc = torch.from_numpy(host).cuda()
            assert alloc.data_ptr() % 16 == 0
            got.append(buffer(W, alloc[off:off + max(nbytes, 1)], nbytes))
            assert np.array_equal(alloc.cpu().numpy(), host)  # d_buf is only read
        assert got == [want, want], (nbytes, off)
    assert buffer(W, alloc[off:off + max(nbytes, 1)], nbytes, fill=0x00) == want  # any d_work contents


def test_buffer_large(W):
    nbytes, off = (64 << 20) + 3, 8
    alloc = torch.empty(nbytes + off + 64, dtype=torch.uint8, device="cuda")
    W.synth_fill(alloc, seed=0xB0FF)
    view = alloc[off:off + nbytes]
    got = buffer(W, view, nbytes)
    assert got == O.crc32(view.cpu().numpy())


def test_graph_replay(W):
    """A concat call and a buffer call captured on a side stream (one chain), replayed,
    then replayed again over inputs changed in place."""
    n, nbytes, off = 70_000, 300_007, 8
    d_crc = torch.zeros(n, dtype=torch.int32, device="cuda")
    alloc = torch.zeros(nbytes + off + 16, dtype=torch.uint8, device="cuda")
    view = alloc[off:off + nbytes]
    cwork = torch.full((W.concat_work_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")
    bwork = torch.full((W.buffer_work_bytes(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")
    o1, o2 = Out(), Out()

    def call():
        W.crc32_concat(d_crc, None, n, o1.ptr, length=1456, last_len=1000, work=cwork)
        W.crc32_buffer(view, nbytes, o2.ptr, work=bwork)

    g, _ = capture(call)
    for salt in (1, 2):
        crc = _words(n, salt)
        data = O.synth_fill_np(nbytes, start_byte=1000 * salt)
        d_crc.copy_(dev_s32(crc))
        view.copy_(torch.from_numpy(data).cuda())
        o1.t[1] = 0
        o2.t[1] = 0
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert o1.value() == M.concat_fixed(crc, 1456, 1000)
        assert o2.value() == O.crc32(data)


# ---- host buffer, endpoints --------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [0, 1, 1456, 1457, 1_000_003])
def test_host_buffer(W, nbytes):
    data = O.synth_fill_np(nbytes, start_byte=17)
    want = O.crc32(data)
    assert W.host_buffer(data if nbytes else np.zeros(1, np.uint8), nbytes) == want
    pin = W.PinnedBuffer(max(nbytes, 1))
    try:
        pin.array[:nbytes] = data
        assert W.host_buffer(pin.array, nbytes) == want
    finally:
        pin.free()


def test_digest_loopback_gpu(W, binaries, tmp_path):
    src = os.path.join(GOLD, "input.txt")
    with open(src, "rb") as f:
        data = f.read()
    check_digest(data, *digest_transfer(binaries, src, str(tmp_path), crc="gpu"), "gpu")
