"""The converter's rule of include/jbonsai_amd.h ("output rate") restated away from the library, the cases that reach
every path of k_resample, and the host probe with real FMAs (tests/plan/resample_probe.cpp).

prototype_ld evaluates the header's formula in numpy.longdouble (a 64-bit mantissa on x86-64) with its own sinc and I0
series -- it takes nothing from jb_resample_filter -- and polyphase_ld sums in long double.  polyphase_seq64 is the
float64 comparator: the float64 prototype of tests/test_resample_abi.py, accumulated one term after the other in
ascending j (no einsum: its pairwise sums are another order).  The per-sample measure is

    e(Y) = max_k |Y[k] - Y_ld[k]| / max_k |Y_ld[k]|

and the tests hold the FMA chain to e(probe) <= GATE * e(polyphase_seq64), GATE the project's one factor
(tests/fbank_ref.py), and the device to the probe bit for bit.
"""
import subprocess
from collections import namedtuple
from math import gcd
from pathlib import Path

import numpy as np

from tests import fbank_ref

LD = np.longdouble
GATE = fbank_ref.GATE
SIGMA = 3000.0  # of the Gaussian signals, as tests/test_gpu_resample.py's
have_long_double = fbank_ref.have_long_double

ROOT = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"

# The paths of k_resample (jb_resample_geometry): the window in LDS with 4, 2 or 1 waves per row block, or no LDS
LDS4, LDS2, LDS1, GLOBAL = "lds-4-waves", "lds-2-waves", "lds-1-wave", "global"
Case = namedtuple("Case", "in_hz out_hz L M ntaps path rows pad what")
# rows and pad as jb_resample_geometry reports them (asserted by check_class: a change of the LDS budget or of the
# thresholds that moves a case to another path fails there instead of quietly testing one path twice)
CASES = (
    Case(48000, 16000, 1, 3, 214, LDS4, 256, 0, "the baseline of tests/test_gpu_resample.py"),
    Case(48000, 32000, 2, 3, 108, LDS4, 256, 0, "L = 2"),
    Case(16000, 48000, 3, 1, 72, LDS4, 256, 0, "M = 1, L = 3 below the wave count"),
    Case(48000, 25000, 25, 48, 138, LDS2, 128, 4, "2 waves, pad 4"),
    Case(48000, 1500, 1, 32, 2276, LDS2, 128, 5, "2 waves, pad 5, L = 1"),
    Case(48000, 11025, 147, 640, 310, LDS1, 12, 7, "12 rows, pad 7"),
    Case(48000, 22050, 147, 320, 156, LDS1, 24, 6, "24 rows, pad 6"),
    Case(44100, 48000, 160, 147, 72, LDS1, 55, 0, "55 rows, unpadded, odd M, L > M"),
    Case(8000, 44100, 441, 80, 72, LDS1, 64, 4, "rows capped at 64 (95 fit), pad 4"),
    Case(48000, 1000, 1, 48, 3414, LDS1, 64, 4, "64 rows (89 fit), L = 1: three waves idle"),
    Case(48000, 400, 1, 120, 8534, GLOBAL, 256, 0, "the window does not fit: global memory"),
    Case(2048, 1, 1, 2048, 145636, GLOBAL, 256, 0, "global memory, the largest M and ntaps"),
    Case(1, 2048, 2048, 1, 72, LDS4, 256, 0, "the largest L"),
    Case(2048, 2047, 2047, 2048, 72, LDS1, 3, 7, "3 rows per tile, the largest L with the largest M"),
)
IDS = [f"{c.in_hz}-{c.out_hz}" for c in CASES]
WAVES = {LDS4: 4, LDS2: 2, LDS1: 1, GLOBAL: 4}


def check_class(g, c):
    """The geometry jb_resample_geometry reports for case c is the path the table names."""
    assert (g.L, g.M, g.ntaps, g.identity) == (c.L, c.M, c.ntaps, 0), c
    assert (g.L, g.M) == (c.out_hz // gcd(c.in_hz, c.out_hz), c.in_hz // gcd(c.in_hz, c.out_hz))
    assert g.lds == (c.path != GLOBAL) and g.row_waves == WAVES[c.path], (c, g.lds, g.row_waves)
    assert (g.rows, g.pad) == (c.rows, c.pad), (c, g.rows, g.pad)
    if c.path == LDS4:
        assert g.fit >= 256
    elif c.path == LDS2:
        assert 128 <= g.fit < 256
    elif c.path == LDS1:
        assert 1 <= g.fit < 128 and g.rows == min(g.fit, 64)
    else:
        assert g.fit == 0 and g.lds_bytes == 0 and g.ntaps + g.M > g.cap


def out_len(n, L, M):
    return -(-n * L // M)


def lengths(L, M, ntaps, rows):
    """Input lengths of a case: 0, 1, 2 and ntaps - 1 (every window hangs over both ends), and for each row count R
    in 1, rows - 1, rows, rows + 1 and 2 rows + 1 the lengths whose n_out has ceil(n_out / L) = R and n_out mod L of
    0, 1 and L - 1 (last_rows: the nearest that a length gives): a tile of one row, a tile one row short, the full
    tile, one row in a second tile, a third tile; last rows whole, of one output and one output short."""
    ns = [0, 1, 2, ntaps - 1]
    for R in sorted({1, rows - 1, rows, rows + 1, 2 * rows + 1} - {0}):
        by_rest = {}
        # n_out in ((R - 1) L, R L]  <=>  n L / M in ((R - 1) L, R L]: n within M + 1 of (R - 1) M
        for n in range(max(1, (R - 1) * M - 1), R * M + 2):
            n_out = out_len(n, L, M)
            if -(-n_out // L) == R:
                by_rest.setdefault(n_out % L, n)
        assert by_rest, (L, M, R)
        ns += [by_rest[r] for r in last_rows(L, M)]
    return ns


def last_rows(L, M):
    """The n_out mod L a case is run at: 0, the smallest above 0 and the largest that any length gives.  n = m M + i
    with i in 1..M has n_out = m L + ceil(i L / M), so the row count does not matter; with L <= M these are 0, 1 and
    L - 1, with L > M the nearest there are (none but 0 with M = 1)."""
    reach = sorted({-(-i * L // M) % L for i in range(1, M + 1)})
    return sorted({0, min(reach[1:], default=0), reach[-1]})


def rests(ns, L, M):
    return {out_len(n, L, M) % L for n in ns if n}


def signals(c, ns):
    rng = np.random.default_rng(c.in_hz * 4099 + c.out_hz)
    return [SIGMA * rng.standard_normal(n) for n in ns]


# ---- the rule in long double, and the float64 comparator -------------------------------------------------------------
def _i0_ld(x):
    """sum_k ((x / 2)^k / k!)^2 in long double: for x <= 10 the terms fall below 1e-40 of the sum before k = 50."""
    h = x * x / LD(4)
    s, term = np.ones_like(x), np.ones_like(x)
    for k in range(1, 50):
        term = term * h / LD(k * k)
        s = s + term
    return s


def prototype_ld(in_hz, out_hz):
    """(L, M, C, h[L][2 C]) in long double, from the header's formula alone."""
    g = gcd(in_hz, out_hz)
    L, M = out_hz // g, in_hz // g
    r = min(LD(1), LD(L) / LD(M))
    fc = LD(45) / LD(100) * r
    H = LD(32) / (LD(2) * fc)
    C = int(np.ceil(H))
    pi = np.arccos(LD(-1))
    p = np.arange(L, dtype=LD)[:, None]
    j = np.arange(2 * C, dtype=LD)[None, :]
    t = p / LD(L) + LD(C - 1) - j
    inside = np.abs(t) < H
    x = LD(2) * fc * t
    # sinc(x) = (-1)^n sin(pi (x - n)) / (pi x) with n the nearest integer: the sine of a small argument
    n = np.rint(x)
    sign = LD(1) - LD(2) * np.mod(n, LD(2))
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(x == 0, LD(1), sign * np.sin(pi * (x - n)) / (pi * x))
    u = np.clip(LD(1) - (t / H) ** 2, LD(0), None)
    w = _i0_ld(LD(10) * np.sqrt(u)) / _i0_ld(np.array(LD(10)))
    return L, M, C, np.where(inside, LD(2) * fc * sinc * w, LD(0))


def _polyphase(x, L, M, h):
    """y[k] = sum_j h[p][j] x[q - C + 1 + j] in h's type, one term after the other in ascending j."""
    x = np.asarray(x)
    ntaps = h.shape[1]
    C = ntaps // 2
    k = np.arange(out_len(x.size, L, M), dtype=np.int64)
    q, p = (k * M) // L, (k * M) % L
    xp = np.concatenate([np.zeros(C - 1), x, np.zeros(C + 1)]).astype(h.dtype)  # xp[a + C - 1] = x[a]
    hT = np.ascontiguousarray(h.T)
    acc = hT[0][p] * xp[q]
    for j in range(1, ntaps):
        acc = acc + hT[j][p] * xp[q + j]
    return acc


def polyphase_ld(x, in_hz, out_hz):
    L, M, _, h = prototype_ld(in_hz, out_hz)
    return _polyphase(x, L, M, h)


def polyphase_seq64(x, in_hz, out_hz):
    from tests.test_resample_abi import prototype

    L, M, _, h = prototype(in_hz, out_hz)
    y = _polyphase(np.asarray(x, dtype=np.float64), L, M, h.astype(np.float64))
    assert y.dtype == np.float64
    return y


def err(Y, Y_ld):
    Y_ld = np.asarray(Y_ld, dtype=LD)
    return float(np.max(np.abs(np.asarray(Y, dtype=np.float64).astype(LD) - Y_ld)) / np.max(np.abs(Y_ld)))


# ---- the probe -------------------------------------------------------------------------------------------------------
def build_probe(folder):
    """tests/plan/resample_probe.cpp by the host pass of hipcc, contraction off, against the built library."""
    libdir = ROOT / "jbonsai_amd"
    exe = Path(folder) / "resample_probe"
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall",
           "-Werror", "-Wno-unused-result", "-I", str(ROOT / "include"), "-x", "hip",
           str(ROOT / "tests" / "plan" / "resample_probe.cpp"), "-L", str(libdir), "-ljbonsai_amd",
           "-Wl,-rpath," + str(libdir), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_probe(exe, in_hz, out_hz, xs, folder):
    """The probe's outputs of the utterances xs (binary files under `folder`), one array each."""
    src, dst = Path(folder) / f"x_{in_hz}_{out_hz}.f64", Path(folder) / f"y_{in_hz}_{out_hz}.f64"
    np.concatenate([np.asarray(x, dtype="<f8") for x in xs] + [np.zeros(0, dtype="<f8")]).tofile(src)
    r = subprocess.run([str(exe), str(in_hz), str(out_hz), str(src), str(dst), *[str(len(x)) for x in xs]],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    y = np.fromfile(dst, dtype="<f8")
    g = gcd(in_hz, out_hz)
    n_out = [out_len(len(x), out_hz // g, in_hz // g) for x in xs]
    assert y.size == sum(n_out)
    return [a.astype(np.float64) for a in np.split(y, np.cumsum(n_out)[:-1])]
