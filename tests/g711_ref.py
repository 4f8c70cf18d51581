"""G.711 in numpy, as a reference for the format stage (tests/format_ref.py): mu-law and A-law of 16-bit samples with
the semantics of the common C implementation -- what CPython's audioop.lin2ulaw / lin2alaw give at width 2 -- and the
two decoders.  The segment is found by a compare ladder over the powers of two; nothing here shares code with the
library."""
import numpy as np


def _top_bit(m, lo, hi):
    """Index of the highest set bit of each m, for m in [2^lo, 2^(hi + 1))."""
    t = np.full(m.shape, lo, dtype=np.int64)
    for b in range(lo + 1, hi + 1):
        t += m >= (1 << b)
    return t


def lin2ulaw(s):
    """uint8 mu-law codes of int16 samples: 14-bit magnitude clipped at 8159, bias 33."""
    p = np.asarray(s, dtype=np.int64) >> 2  # arithmetic
    neg = p < 0
    m = np.minimum(np.abs(p), 8159) + 33  # 33 .. 8192
    seg = _top_bit(m, 5, 13) - 5
    code = (seg << 4) | ((m >> (seg + 1)) & 15)
    # the clip plus the bias is 2^13, one past the last segment's end (0x1FFF): that implementation then returns the
    # largest code, 0x7F, before the inversion
    code = np.where(seg >= 8, 0x7F, code)
    return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def lin2alaw(s):
    """uint8 A-law codes of int16 samples: 13-bit magnitude."""
    p = np.asarray(s, dtype=np.int64) >> 3
    neg = p < 0
    m = np.where(neg, -p - 1, p)
    seg = np.maximum(_top_bit(np.maximum(m, 1), 0, 12) - 4, 0)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def ulaw2lin(c):
    u = ~np.asarray(c, dtype=np.int64) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(c):
    a = np.asarray(c, dtype=np.int64) ^ 0x55
    t = (a & 0x0F) << 4
    seg = (a & 0x70) >> 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)
