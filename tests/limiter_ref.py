"""The limiter's rule (include/jbonsai_amd.h "Limiter") restated in numpy, independent in shape of the library's
statement: the true-peak taps from their formula, the sliding minimum as sliding_window_view(...).min, the smoothing as
one long-double dot product per sample.  And the shapes both test files run: every case is (name, x, hz, gain,
ceiling_db, opts)."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TILE = 1024  # samples per workgroup of the device (kLimTile)
LD = np.longdouble


def samples(ms, hz):
    return int(math.floor(ms * hz / 1000.0 + 0.5))


def geometry(hz, lookahead_ms=2.0, hold_ms=8.0):
    return max(1, samples(lookahead_ms, hz)), samples(hold_ms, hz)


def window(L):
    """The interior of a Hann window of L + 3 points, normalised to sum 1 (long double)."""
    i = np.arange(1, L + 2, dtype=LD)
    pi = LD(np.pi) + LD(1.2246467991473532e-16)  # (the double nearest pi, and what it leaves out)
    h = LD(0.5) - LD(0.5) * np.cos(LD(2.0) * pi * i / LD(L + 2))
    return h / h.sum()


def true_peak_taps(hz):
    """[F - 1, 12]: phase p = 1..F-1, tap j: sinc(t) kaiser_8(t / 6), t = p / F + 5 - j."""
    F = min(64, -(-192000 // hz))
    p = np.arange(1, F, dtype=np.float64)[:, None]
    j = np.arange(12, dtype=np.float64)[None, :]
    t = p / F + 5.0 - j
    return F, np.sinc(t) * np.i0(8.0 * np.sqrt(1.0 - (t / 6.0) ** 2)) / np.i0(8.0)


def between(u, hz):
    """b[-1 .. N-1] (index i: b[i - 1]): the largest interpolated magnitude between samples i - 1 and i."""
    F, h = true_peak_taps(hz)
    n = u.size
    if F < 2:
        return np.zeros(n + 1)
    pad = np.concatenate([np.zeros(6), u, np.zeros(6)]).astype(LD)  # pad[k] = u[k - 6]
    win = sliding_window_view(pad, 12)  # win[i] = u[i - 6 .. i + 5] = the window of b[i - 1]
    return np.abs(win[: n + 1] @ h.T.astype(LD)).max(axis=1).astype(np.float64)


def detector(u, hz, true_peak):
    d = np.abs(u)
    if true_peak:
        b = between(u, hz)
        d = np.maximum(d, np.maximum(b[:-1], b[1:]))
    return d


def limit(x, hz, gain, ceiling_db, true_peak=False, lookahead_ms=2.0, hold_ms=8.0):
    """(y, a, d, c, L, H) of the rule, a and y in long double before y's rounding to f64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    L, H = geometry(hz, lookahead_ms, hold_ms)
    c = np.float64(32768.0) * np.power(np.float64(10.0), np.float64(ceiling_db) / 20.0)
    u = x * np.float64(gain)
    d = detector(u, hz, true_peak)
    with np.errstate(divide="ignore"):
        r = np.where(d > c, c / np.where(d > c, d, 1.0), 1.0)
    # m[k], k = -L .. n - 1: min r[k - H .. k + L] of r padded with ones: index k + L of the windows over
    # r[-L - H .. n - 1 + L]
    rp = np.concatenate([np.ones(L + H), r, np.ones(L)])
    m = sliding_window_view(rp, H + L + 1).min(axis=1)  # n + L entries
    w = window(L)
    # a[i] = sum_j w[j] m[i - j] = sum_j w[j] mm[i + L - j]: the windows of m of L + 1 entries, reversed
    a = (sliding_window_view(m.astype(LD), L + 1)[:, ::-1] @ w)
    a = np.minimum(a, r.astype(LD))
    y = np.clip(u.astype(LD) * a, -LD(c), LD(c))
    return y, a, d, c, L, H


def reach(d, c, L, H):
    """mask[n]: some d[i] > c lies in i = n - L - H .. n + L."""
    n = d.size
    mask = np.zeros(n, dtype=bool)
    for i in np.nonzero(d > c)[0]:
        mask[max(0, i - L): min(n, i + L + H + 1)] = True
    return mask


def true_peak_of(y, hz):
    """The largest magnitude of y and of its interpolated phases (every gap, the two at the ends included)."""
    y = np.asarray(y, dtype=np.float64)
    return max(np.abs(y).max(), between(y, hz).max())


CEILING = -1.0


def _noise(rng, n, amp=3000.0):
    return rng.standard_normal(n) * amp


def cases():
    """The edge shapes: N = 1, N < L, N = tile - 1, tile, tile + 1; a peak at sample 0, at N - 1 and on either side of
    a tile boundary; a run of over-ceiling samples longer than the tile; 8, 16 and 48 kHz; 2 L + H = 2048."""
    rng = np.random.default_rng(20261019)
    big = 60000.0
    out = []
    out.append(("n1", np.array([big]), 16000, 1.0, None))
    x = _noise(rng, 10)
    x[4] = -big
    out.append(("n_below_L", x, 16000, 1.0, None))
    for n in (TILE - 1, TILE, TILE + 1):
        x = _noise(rng, n)
        x[0] = big
        x[n - 1] = -big
        x[n // 2] = 0.7 * big
        out.append(("n%d_ends" % n, x, 16000, 1.7, None))
    x = _noise(rng, 3 * TILE + 77)
    x[TILE - 1] = big
    x[2 * TILE] = -big
    out.append(("tile_boundary", x, 16000, 1.3, None))
    # every sample of [2 tile - 200, 3 tile + 100) over the ceiling, either sign: the third tile and its halo
    # (L + H = 160 in front, L = 32 behind) hold no r = 1
    x = _noise(rng, 5 * TILE - 100)
    run = _noise(rng, TILE + 300, 8000.0)
    c = 32768.0 * 10.0 ** (CEILING / 20.0)
    x[2 * TILE - 200: 3 * TILE + 100] = np.where(run < 0.0, -1.0, 1.0) * (1.05 * c / 1.5 + np.abs(run))
    out.append(("long_run", x, 16000, 1.5, None))
    for hz in (8000, 48000):
        x = _noise(rng, 2 * TILE + 313, 6000.0)
        x[17] = big
        x[TILE + 5] = -0.9 * big
        out.append(("hz%d" % hz, x, hz, 1.9, None))
    # 48 kHz, 10 ms and 1088 samples of hold: 2 L + H = 2048
    x = _noise(rng, 3 * TILE + 11, 8000.0)
    x[5] = big
    x[TILE + TILE // 2] = big
    x[3 * TILE] = -big
    out.append(("span2048", x, 48000, 1.4, (10.0, 1088 / 48.0)))
    return out


def longest_run(mask):
    """The longest stretch of consecutive true entries."""
    best = cur = 0
    for v in mask:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best
