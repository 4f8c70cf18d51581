"""numpy evaluation of the true-peak definition (include/jbonsai_amd.h "loudness", step 5; ITU-R BS.1770-4 Annex 2):
the oversampling factor, the Kaiser-windowed sinc interpolator, the phases and the peak.  Independent of the library:
the table comes from the formula here, not from jb_true_peak_filter."""
import math

import numpy as np

FULL_SCALE = 32768.0
TAPS = 12


def factor(hz):
    """F = min(64, ceil(192000 / hz))."""
    return min(64, -(-192000 // int(hz)))


def _i0(x):
    """I0 by its power series sum_k ((x/2)^k / k!)^2 (all terms positive)."""
    s = term = 1.0
    h = 0.25 * x * x
    for k in range(1, 80):
        term *= h / (k * k)
        s += term
    return s


def h_of(t):
    """h(t) = sinc(t) I0(8 sqrt(1 - (t/6)^2)) / I0(8) for |t| < 6, else 0."""
    if abs(t) >= 6.0:
        return 0.0
    sinc = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
    return sinc * _i0(8.0 * math.sqrt(1.0 - (t / 6.0) ** 2)) / _i0(8.0)


def table(hz):
    """(F, taps): taps [F - 1][12], row p - 1 = phase p, h[p][j] = h(p/F + 5 - j)."""
    F = factor(hz)
    taps = np.zeros((F - 1, TAPS))
    for p in range(1, F):
        for j in range(TAPS):
            taps[p - 1, j] = h_of(p / F + 5 - j)
    return F, taps


_tables = {}


def true_peak_lin(x, hz):
    """TPlin = max(max |x[n]|, max_{p,n} |y_p[n]|), y_p[n] = sum_j h[p][j] x[n - 5 + j], x = 0 outside [0, N)."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return 0.0
    if hz not in _tables:
        _tables[hz] = table(hz)
    F, taps = _tables[hz]
    best = float(np.max(np.abs(x)))
    if F > 1:
        xp = np.concatenate([np.zeros(5), x, np.zeros(6)])
        win = np.lib.stride_tricks.sliding_window_view(xp, TAPS)  # win[n][j] = x[n - 5 + j]
        best = max(best, float(np.max(np.abs(win @ taps.T))))
    return best


def true_peak(x, hz):
    """TP (dBTP) of x at hz; -inf for silence."""
    lin = true_peak_lin(x, hz)
    return 20.0 * math.log10(lin / FULL_SCALE) if lin > 0 else -math.inf


def gain_db(L, TP, target, ceiling):
    terms = [v for v in (target - L, ceiling - TP) if math.isfinite(v)]
    return min(terms) if terms else 0.0
