"""Model of the CRC fold (wtp_crc32_combine, wtp_crc32_concat): zlib crc32_combine
semantics by square and multiply in GF(2)[x]/P, so lengths of 2^32 and beyond cost
O(log len) (oracle.combine shifts byte by byte).  Generated from the polynomial.

A 32-bit word is a polynomial in the CRC register's reflected order: bit 31 is x^0.
  crc32(A || B) = crc32(A) * x^(8|B|) mod P  ^  crc32(B)
The concat functions use the suffix-sum form  XOR_i crc_i * x^(8 S_i)  (S_i = bytes after
payload i), vectorised with numpy; `concat_fold` is the plain left-to-right fold.
"""
import numpy as np

POLY = 0xEDB88320
ONE = 0x80000000          # x^0
ORDER = 0xFFFFFFFF        # x^(8 * ORDER) == 1 (test_concat_model checks it)


def mulmod(a, b):
    """a * b mod P; python ints, or numpy uint32 arrays / scalars broadcast together."""
    if isinstance(a, int) and isinstance(b, int):
        p = 0
        for i in range(32):
            if (a >> (31 - i)) & 1:
                p ^= b
            b = (b >> 1) ^ (POLY if b & 1 else 0)
        return p
    a = np.asarray(a, dtype=np.uint32)
    b = np.broadcast_to(np.asarray(b, dtype=np.uint32), a.shape).copy()
    p = np.zeros(a.shape, dtype=np.uint32)
    for i in range(32):
        p ^= np.where((a >> np.uint32(31 - i)) & np.uint32(1), b, np.uint32(0))
        b = (b >> np.uint32(1)) ^ np.where(b & np.uint32(1), np.uint32(POLY), np.uint32(0))
    return p


def _pow8_table():
    g, out = ONE >> 8, []
    for _ in range(64):
        out.append(g)
        g = mulmod(g, g)
    return out


POW8 = _pow8_table()      # POW8[k] = x^(8 * 2^k)


def xpow8(nbytes: int) -> int:
    """x^(8 * nbytes) for any non-negative int below 2^64, without reducing the exponent."""
    r, k = ONE, 0
    while nbytes:
        if nbytes & 1:
            r = mulmod(r, POW8[k])
        nbytes >>= 1
        k += 1
    return r


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    return mulmod(crc_a, xpow8(len_b)) ^ crc_b


def concat_fold(crcs, lens) -> int:
    d = 0
    for c, l in zip(crcs, lens):
        d = combine(d, int(c), int(l))
    return d


def xpow8_vec(nbytes) -> np.ndarray:
    """x^(8 * nbytes[i]) for a uint64 array."""
    e = np.asarray(nbytes, dtype=np.uint64)
    r = np.full(e.shape, ONE, dtype=np.uint32)
    for k in range(64):
        bit = ((e >> np.uint64(k)) & np.uint64(1)).astype(bool)
        if bit.any():
            r = np.where(bit, mulmod(r, np.uint32(POW8[k])), r)
    return r


def concat_var(crcs, lens) -> int:
    """CRC of the concatenation from per-payload CRCs and lengths (uint32 each).  The
    suffix sums are carried mod 2^32 - 1, so they fit uint64 for any n."""
    c = np.asarray(crcs, dtype=np.uint32)
    if c.size == 0:
        return 0
    l = np.asarray(lens, dtype=np.uint64) % np.uint64(ORDER)
    after = np.concatenate([l[1:], np.zeros(1, np.uint64)])
    sfx = np.cumsum(after[::-1], dtype=np.uint64)[::-1] % np.uint64(ORDER)  # n * 2^32 < 2^64
    return int(np.bitwise_xor.reduce(mulmod(c, xpow8_vec(sfx))))


def concat_fixed(crcs, length: int, last_len: int) -> int:
    """Payloads 0 .. n-2 of `length` bytes, payload n-1 of `last_len`; any ints < 2^64.
    A pairwise tree over the body: level j multiplies the left halves by x^(8 length 2^j)."""
    c = np.asarray(crcs, dtype=np.uint32)
    n = c.size
    if n == 0:
        return 0
    body = c[:n - 1]
    m = xpow8(length)
    while body.size > 1:
        if body.size & 1:  # a leading zero contributes nothing
            body = np.concatenate([np.zeros(1, np.uint32), body])
        body = mulmod(body[0::2], np.uint32(m)) ^ body[1::2]
        m = mulmod(m, m)
    b = int(body[0]) if body.size else 0
    return combine(b, int(c[n - 1]), last_len)
