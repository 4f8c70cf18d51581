"""The reference of the filter stage's tests: the serial cascade in numpy.longdouble over the library's own coefficients
(jb_filter_design), the table of filters and lengths, the input, the error measure and the gate.

The error of a result is max|y - y_ld| / max|y_ld| over the utterance.

The gate is a measurement, made when the tests run: floor() is that error for scipy.signal.sosfilt in f64 (a serial
direct-form II transposed cascade: the floor any f64 recursion has), the largest over the whole table below, and the
device and the host seam are gated at gate() = 8 x floor().  The device's scan re-associates each start state as a sum
over up to 8 + 6 + chunk carried terms, and nothing else separates it from the serial order.  With scipy 1.15 the floor
is 1.426e-12 (the high-pass at 20 Hz / 96 kHz over 130 tiles: its poles are the nearest to the unit circle), the gate
1.141e-11, and the host seam's largest error 1.323e-12.  Run this file to print every case.
"""
from __future__ import annotations

import functools

import numpy as np

import jbonsai_amd as J

TILE = 4096
LENGTHS = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 2 * TILE + 3, 65 * TILE + 5, 130 * TILE + 7]
MAX_LEN = max(LENGTHS)

def _butter8():
    from scipy import signal

    return J.raw_filter(signal.butter(8, 0.2, output="sos"))


@functools.lru_cache(maxsize=None)
def filters():
    """[(name, Filter, hz)]: the eight filters, then the 4-section cascades every one of them is a member of."""
    hp20, hp70 = J.highpass(20.0, 0.7071), J.highpass(70.0)
    peak, lsh, hsh = J.peaking(3000.0, 6.0, 2.0), J.lowshelf(200.0, -6.0), J.highshelf(8000.0, 4.0)
    notch = J.notch(50.0, 30.0)
    return [
        ("hp20@96k", hp20, 96000),
        ("hp70@48k", hp70, 48000),
        ("telephone@8k", J.telephone_band(), 8000),
        ("peaking@48k", peak, 48000),
        ("lowshelf@48k", lsh, 48000),
        ("highshelf@48k", hsh, 48000),
        ("notch@48k", notch, 48000),
        ("butter8", _butter8(), 48000),  # (RAW: itself a 4-section cascade)
        ("hp70+peaking+lowshelf+highshelf@48k", hp70 + peak + lsh + hsh, 48000),
        ("hp20+notch+telephone@96k", hp20 + notch + J.telephone_band(), 96000),
    ]


@functools.lru_cache(maxsize=None)
def signal_at(hz: int) -> np.ndarray:
    """MAX_LEN samples at hz: noise, a 220 Hz tone and a DC offset of 1000, inside +-32767.  An utterance of n samples
    is its first n."""
    rng = np.random.default_rng(20251019 + hz)
    t = np.arange(MAX_LEN, dtype=np.float64)
    x = 3000.0 * rng.standard_normal(MAX_LEN) + 8000.0 * np.sin(2.0 * np.pi * 220.0 * t / hz) + 1000.0
    return np.clip(x, -32767.0, 32767.0)


def cascade_longdouble(coefs: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The serial cascade (transposed direct form II) of coefs [ns, 5] = b0 b1 b2 a1 a2 over x, in numpy.longdouble."""
    ld = np.longdouble
    y = np.asarray(x, dtype=ld)
    for c in coefs:
        b0, b1, b2, a1, a2 = (ld(v) for v in c)
        s0 = s1 = ld(0)
        out = np.empty(y.size, dtype=ld)
        for i, xi in enumerate(y):
            yi = b0 * xi + s0
            s0 = b1 * xi - a1 * yi + s1
            s1 = b2 * xi - a2 * yi
            out[i] = yi
        y = out
    return y


@functools.lru_cache(maxsize=None)
def reference(index: int) -> np.ndarray:
    """The long-double output of filters()[index] over its rate's MAX_LEN samples (its first n: the reference of the
    utterance of n samples).  Computed once."""
    _, f, hz = filters()[index]
    return cascade_longdouble(J.filter_design(f, hz), signal_at(hz))


def error(y: np.ndarray, index: int) -> float:
    """max|y - y_ld| / max|y_ld| of an n-sample result of filters()[index]; 0 for n = 0."""
    n = len(y)
    if n == 0:
        return 0.0
    ref = reference(index)[:n]
    return float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - ref)) / np.max(np.abs(ref)))


def cases():
    """[(filter index, n)] over the whole table."""
    return [(i, n) for i in range(len(filters())) for n in LENGTHS]


def sosfilt_errors():
    """{(filter index, n): error of scipy.signal.sosfilt in f64}."""
    from scipy import signal

    out = {}
    for i, (_, f, hz) in enumerate(filters()):
        sos = J.filter_sos(f, hz)
        for n in LENGTHS:
            out[(i, n)] = error(signal.sosfilt(sos, signal_at(hz)[:n]), i) if n else 0.0
    return out


@functools.lru_cache(maxsize=None)
def floor() -> float:
    return max(sosfilt_errors().values())


def gate() -> float:
    return 8.0 * floor()


def host_errors():
    """{(filter index, n): error of jb_filter_pcm_host}."""
    return {(i, n): error(J.filter_pcm_host(signal_at(hz)[:n], f, hz), i)
            for i, (_, f, hz) in enumerate(filters()) for n in LENGTHS}


if __name__ == "__main__":
    sos, host = sosfilt_errors(), host_errors()
    for (i, n) in cases():
        print(f"{filters()[i][0]:40s} n={n:7d}  sosfilt {sos[(i, n)]:.3e}  host seam {host[(i, n)]:.3e}")
    print(f"largest: sosfilt {max(sos.values()):.3e}  host seam {max(host.values()):.3e}  "
          f"floor {floor():.3e}  gate {gate():.3e}")
