"""References of the noise stage (include/jbonsai_amd.h "Noise"), independent of the library:

- mix, white, vary: the splitmix64 finaliser, the white generator and JB_NOISE_VARY's rule in Python integers;
- power_sum, host_rule: the rule restated in f64 -- tiles of 1,024 samples, 256 partials of up to four terms (the first a
  product, every later one fused on), the tree h = 128 .. 1, the tile sums added in ascending order; the active test,
  the gain's operation order and y = fma(g, w, x) -- with math.fma where Python has it and an exact emulation
  (fractions) where it has not;
- ratio: 10^(db / 10) in numpy.longdouble, rounded once;
- achieved_snr_db: 10 log10((A / C) / (g^2 Bs / N)) in numpy.longdouble from the inputs themselves.
"""
import math
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
TILE, LANES = 1024, 256


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def white(seed, first, count):
    ms = mix(seed & M64)
    out = np.empty(count, dtype=np.float64)
    for i in range(count):
        r = mix(ms ^ (first + i))
        out[i] = float((r & 0xffff) + ((r >> 16) & 0xffff) + ((r >> 32) & 0xffff) + (r >> 48) - 131070)
    return out


def vary(seed, k, bed_len):
    z = mix(mix(seed & M64) ^ k)
    return z, (mix(z) % bed_len if bed_len else 0)


def sequence(n, bed=None, offset=0, seed=0):
    """w[0..n): the looped bed from `offset`, or the white sequence of `seed`."""
    if bed is None:
        return white(seed, 0, n)
    bed = np.asarray(bed, dtype=np.float64)
    return bed[(offset + np.arange(n)) % bed.size]


def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s == 0:
        return a * b + c if p == 0 else 0.0
    return float(s)


def tile_sums(z):
    z = [float(v) for v in np.asarray(z, dtype=np.float64)]
    n = len(z)
    out = []
    for i in range((n + TILE - 1) // TILE):
        p = [0.0] * LANES
        for l in range(LANES):
            first = True
            for j in range(TILE // LANES):
                k = i * TILE + l + LANES * j
                if k >= n:
                    break
                p[l] = z[k] * z[k] if first else _fma(z[k], z[k], p[l])
                first = False
        h = LANES // 2
        while h:
            for l in range(h):
                p[l] = p[l] + p[l + h]
            h //= 2
        out.append(p[0])
    return out


def total(t):
    if not t:
        return 0.0
    s = t[0]
    for v in t[1:]:
        s = s + v
    return s


def ratio(db):
    """10^(db / 10) in long double, rounded once."""
    if math.isinf(db):
        return db
    return float(np.power(np.longdouble(10), np.longdouble(db) / np.longdouble(10)))


def host_rule(x, w, snr_db, active=False, gate_db=0.0, gain=None):
    """(A, C, Bs, g, y) of x under the noise sequence w, by the rule."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    tx, tw = tile_sums(x), tile_sums(w)
    sx, bs = total(tx), total(tw)
    a, c = sx, n
    if active:
        sq = sx * ratio(-gate_db)
        a, c, first = 0.0, 0, True
        for i, t in enumerate(tx):
            ci = min(TILE, n - i * TILE)
            if t * float(n) >= sq * float(ci):
                a = t if first else a + t
                c += ci
                first = False
    if gain is not None:
        g = float(gain)
    elif a == 0.0 or bs == 0.0 or c == 0 or math.isinf(snr_db):
        g = 0.0
    else:
        g = math.sqrt(((a * float(n)) / (bs * float(c))) / ratio(snr_db))
    if g == 0.0:
        y = x.copy()
    else:
        y = np.array([_fma(g, float(wv), float(xv)) for wv, xv in zip(w, x)], dtype=np.float64).reshape(n)
    return a, c, bs, g, y


def sink_i16(y):
    """The 16-bit sink's rule: fmin to 32767, fmax to -32768, truncate."""
    return np.trunc(np.clip(np.asarray(y, dtype=np.float64), -32768.0, 32767.0)).astype(np.int16)


def achieved_snr_db(x, w, g, tiles=None):
    """10 log10((A / C) / (g^2 Bs / N)) in long double; tiles: the indices of the active tiles (None: the whole)."""
    x = np.asarray(x, dtype=np.longdouble)
    w = np.asarray(w, dtype=np.longdouble)
    n = x.size
    if tiles is None:
        a, c = np.sum(x * x), n
    else:
        sel = np.concatenate([np.arange(i * TILE, min((i + 1) * TILE, n)) for i in tiles])
        a, c = np.sum(x[sel] * x[sel]), sel.size
    bs = np.sum(w * w)
    gl = np.longdouble(g)
    return float(10 * np.log10((a / c) / (gl * gl * bs / n)))


LENGTHS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 17)
BEDS = (1, 7, 1000, 1024, 5000)


def signal(n, seed=1):
    """Speech-like test input: silence (with signed zeros), then noise at 6,000 RMS, then silence."""
    rng = np.random.default_rng(seed + n)
    x = np.round(rng.standard_normal(n) * 6000.0, 3)
    if n >= 8:
        x[: n // 5] = 0.0
        x[n - n // 7:] = -0.0
    x[::11] = -0.0
    if n <= 2:
        x[:] = 1234.5
    return x


def bed_of(lb, seed=3):
    return np.round(np.random.default_rng(seed + lb).standard_normal(lb) * 900.0, 2) + (5.0 if lb == 1 else 0.0)


def cases():
    """The shapes of the host and the device tests: every length under every bed length at the offsets 0, Lb - 1 and
    Lb // 2 and under white noise, the reference and the SNR changing from case to case.  Each: (x, bed or None,
    keywords of J.noise)."""
    out = []
    k = 0
    for n in LENGTHS:
        x = signal(n)
        for lb in BEDS:
            for off in sorted({0, lb - 1, lb // 2}):
                ref = ("whole", "active")[k % 2]
                out.append((x, bed_of(lb), dict(offset=off, snr_db=(-5.0, 10.0, 37.5)[k % 3], reference=ref,
                                                gate_db=(20.0, 3.0)[(k // 2) % 2] if ref == "active" else 0.0)))
                k += 1
        for ref in ("whole", "active"):
            out.append((x, None, dict(seed=0x1234 + n, snr_db=15.0, reference=ref,
                                      gate_db=20.0 if ref == "active" else 0.0)))
    return out
