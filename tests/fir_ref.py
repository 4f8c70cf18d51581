"""References of the convolution stage (include/jbonsai_amd.h "Convolution"), independent of the library:

- direct_ld: the rule's sum in numpy.longdouble (the order of the terms does not matter at that precision for the gates
  that use it);
- host_rule: the host rule restated in f64 -- the in-range terms in ascending k, the first a product, every later one
  fused onto the sum -- with math.fma where Python has it and an exact emulation (fractions) where it has not;
- model_partitioned: a float64 numpy model of the uniform partitioned overlap-save the device runs, from the output of
  fir_geometry (block, partitions): numpy's FFT in the place of the device's;
- fft_whole: float64 numpy.fft.irfft(rfft(x, n) rfft(h, n)) on the whole signal, the yardstick of the error gate;
- rel_err: max|y - y_ld| / (||h||_1 max|x|), the gate's metric.
"""
import math
from fractions import Fraction

import numpy as np


def direct_ld(x, h, d):
    """y[n] = sum_k h[k] x[n + d - k] over the in-range terms, n in [0, N), in long double."""
    x = np.asarray(x, dtype=np.longdouble)
    h = np.asarray(h, dtype=np.longdouble)
    n = x.size
    if n == 0:
        return np.zeros(0, dtype=np.longdouble)
    full = np.convolve(x, h)  # full[m] = sum_k h[k] x[m - k], m in [0, N + K - 1)
    return full[d:d + n]


def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s == 0:
        # an exact zero: the sign rules of a sum of (the exact product) and c
        return a * b + c if p == 0 else 0.0
    return float(s)  # (Fraction -> float rounds to nearest even, once)


def host_rule(x, h, d):
    """The host rule in f64, term for term."""
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    h = [float(v) for v in np.asarray(h, dtype=np.float64)]
    n, k_taps = len(x), len(h)
    y = np.zeros(n, dtype=np.float64)
    for i in range(n):
        top = i + d
        klo, khi = max(0, top - (n - 1)), min(k_taps - 1, top)
        if klo > khi:
            continue
        acc = h[klo] * x[top - klo]
        for k in range(klo + 1, khi + 1):
            acc = _fma(h[k], x[top - k], acc)
        y[i] = acc
    return y


def model_partitioned(x, h, d, block, partitions):
    """Uniform partitioned overlap-save in float64: blocks of `block` samples counted from the utterance's first
    sample, n_fft = 2 block, block j's spectrum from the n_fft samples that end at its end (shifted by d, zeros outside
    the utterance); the d samples in front of block 0 are lead = ceil(d / block) blocks -lead .. -1 of their own;
    Y_j = sum_p X[j - p] H[p] with p ascending from 0 to min(partitions - 1, j + lead), the last `block` samples of the
    inverse kept."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, bk, n_fft = x.size, block, 2 * block
    nb = (n + bk - 1) // bk
    lead = (d + bk - 1) // bk
    hp = np.zeros(partitions * bk)
    hp[:h.size] = h
    H = [np.fft.rfft(hp[p * bk:(p + 1) * bk], n_fft) for p in range(partitions)]
    # x'[m] = x[m + d] at xs[(lead + 1) bk + m]: block f's window is xs[(f + lead) bk : (f + lead + 2) bk]
    xs = np.zeros((nb + lead + 1) * bk)
    xs[(lead + 1) * bk - d:(lead + 1) * bk - d + n] = x
    X = [np.fft.rfft(xs[f * bk:f * bk + n_fft]) for f in range(nb + lead)]  # X[f + lead]
    y = np.zeros(nb * bk)
    for j in range(nb):
        acc = np.zeros(bk + 1, dtype=np.complex128)
        for p in range(min(partitions - 1, j + lead) + 1):
            acc = acc + X[j + lead - p] * H[p]
        y[j * bk:(j + 1) * bk] = np.fft.irfft(acc, n_fft)[bk:]
    return y[:n]


def fft_whole(x, h, d):
    """float64 FFT convolution of the whole signal: the yardstick."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if x.size == 0:
        return np.zeros(0)
    n = 1
    while n < x.size + h.size - 1:
        n *= 2
    full = np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)
    return full[d:d + x.size]


def rel_err(y, y_ld, x, h):
    """max|y - y_ld| / (||h||_1 max|x|)."""
    scale = float(np.sum(np.abs(np.asarray(h, dtype=np.float64))) * np.max(np.abs(np.asarray(x, dtype=np.float64))))
    e = np.max(np.abs(np.asarray(y, dtype=np.longdouble) - np.asarray(y_ld, dtype=np.longdouble)))
    return float(e) / scale


def delays(k_taps):
    """The four delays of the tests: 0, 1, (K - 1) / 2 and K - 1, without repeats."""
    return sorted({0, min(1, k_taps - 1), (k_taps - 1) // 2, k_taps - 1})
