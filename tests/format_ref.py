"""The output sample formats in numpy (include/jbonsai_amd.h "Output sample formats"): float32, 16- and 24-bit PCM with
or without TPDF dither, and G.711 (tests/g711_ref.py), from the f64 samples in 16-bit scale that the PCM read entries
hand out.  encode() returns the bytes the library must produce, bit for bit.  VALUES is the value set the host and the
device tests share."""
import numpy as np

from tests.g711_ref import lin2alaw, lin2ulaw

FORMATS = ("f32", "s16", "s24", "ulaw", "alaw")
BYTES = {"f32": 4, "s16": 2, "s24": 3, "ulaw": 1, "alaw": 1}
M64 = np.uint64(0xFFFFFFFF)


def mix(z):
    """The splitmix64 finaliser on uint64 arrays (mod 2^64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dither(seed, n):
    """d[k], k = 0..n-1: triangular in (-1, 1) LSB, exact in f64."""
    r = mix(mix(np.array([seed], dtype=np.uint64)) ^ np.arange(n, dtype=np.uint64))
    return ((r >> np.uint64(32)).astype(np.float64) - (r & M64).astype(np.float64)) * 2.0 ** -32


def quant(x, lo, hi, d=None):
    """q(x): clamp and truncate toward zero; with dither d, floor((x + d) + 0.5) and then the clamp."""
    x = np.asarray(x, dtype=np.float64)
    if d is not None:
        x = np.floor((x + d) + 0.5)
    return np.clip(x, lo, hi).astype(np.int64)  # numpy truncates toward zero


def encode(v, fmt, dither_on=False, seed=0) -> bytes:
    v = np.ascontiguousarray(v, dtype=np.float64)
    d = dither(seed, v.size) if dither_on else None
    if fmt == "f32":
        return (v * 2.0 ** -15).astype("<f4").tobytes()
    if fmt == "s24":
        q = quant(256.0 * v, -8388608.0, 8388607.0, d)
        return (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    s = quant(v, -32768.0, 32767.0, d).astype(np.int16)
    if fmt == "s16":
        return s.astype("<i2").tobytes()
    return {"ulaw": lin2ulaw, "alaw": lin2alaw}[fmt](s).tobytes()


def decode_s24(data: bytes):
    b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    q = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return np.where(q >= 1 << 23, q - (1 << 24), q)


def value_set():
    """Every integer -32768..32767 with the offsets 0, +-0.25, +-0.5 and +-0.999; beyond the range on both sides; both
    zeros; a subnormal; and multiples of 2^-15 that are ties between two float32 values."""
    ints = np.arange(-32768, 32768, dtype=np.float64)
    parts = [ints + o for o in (0.0, 0.25, -0.25, 0.5, -0.5, 0.999, -0.999)]
    ties = [32768.0 * (1 + 2.0 ** -24), 32768.0 * (1 + 3 * 2.0 ** -24), -32768.0 * (1 + 2.0 ** -24),
            (1 + 2.0 ** -24), 16384.0 * (1 + 5 * 2.0 ** -24), 2.0 ** -15 * (1 + 2.0 ** -24)]
    parts.append(np.array([32767.5, -32767.5, 32768.5, -32768.5, 40000.0, -40000.0, 0.0, -0.0, 1e-310] + ties))
    return np.concatenate(parts)


VALUES = value_set()
