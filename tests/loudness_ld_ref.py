"""The loudness definition (include/jbonsai_amd.h "loudness", steps 1 to 3, 7 and 8) in numpy.longdouble (a 64-bit
mantissa on x86-64): the coefficients from the formula, the serial cascade from zero state, the hop sums z_j, the
four-hop blocks, both gates, L, the momentary maximum, the short-term windows with their maximum, and the loudness
range with the nearest-rank rule.  Independent of the library and of tests/loudness_ref.py: nothing is taken from
jb_loudness_filter, and every sum is a plain ascending sum in long double.

The constants of step 1 are the doubles the header's decimals round to (what the library and the f64 comparator read);
everything computed from them -- pi, tan, the powers, the divisions -- is long double.

Every comparison with a gate records its margin (Measure.margin: the smallest distance in LU of a block from -70 and
from Gamma, of a short-term window from -70 and from Gamma_r, and of the two order statistics of LRA from their
neighbours in the sorted list).  A margin under MARGIN is an error of the table that made the case, never a skip: there
the last bits of a sum could decide membership and no comparison of values would mean anything."""
import math

import numpy as np

LD = np.longdouble
FULL_SCALE = 32768.0
MARGIN = 1e-6  # LU, the rule of tests/loudness_groups_ref.py
BLOCK_HOPS, WINDOW_HOPS = 4, 30

SHELF_FC, SHELF_Q = 1681.974450955533, 0.7071752369554196
SHELF_DB, SHELF_VB_EXP = 3.999843853973347, 0.4996667741545416
HP_FC, HP_Q = 38.13547087602444, 0.5003270373238773


def pi_ld():
    return LD(4) * np.arctan(LD(1))


def hop_of(hz):
    return (int(hz) + 5) // 10


def k_filter_ld(hz):
    """(b, a) as [2][3] long-double arrays (shelf, then high-pass) and the hop H at hz."""
    fs = LD(int(hz))

    def stage(fc, Q, shelf):
        K = np.tan(pi_ld() * LD(fc) / fs)
        Q = LD(Q)
        a0 = LD(1) + K / Q + K * K
        if shelf:
            Vh = np.power(LD(10), LD(SHELF_DB) / LD(20))
            Vb = np.power(Vh, LD(SHELF_VB_EXP))
            b = [(Vh + Vb * K / Q + K * K) / a0, LD(2) * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
        else:
            b = [LD(1), LD(-2), LD(1)]
        return b, [LD(1), LD(2) * (K * K - LD(1)) / a0, (LD(1) - K / Q + K * K) / a0]

    b1, a1 = stage(SHELF_FC, SHELF_Q, True)
    b2, a2 = stage(HP_FC, HP_Q, False)
    return np.array([b1, b2], dtype=LD), np.array([a1, a2], dtype=LD), hop_of(hz)


def pole_radius(hz):
    """The largest pole modulus of the two stages (long double)."""
    _, a, _ = k_filter_ld(hz)
    r = LD(0)
    for a1, a2 in ((a[0][1], a[0][2]), (a[1][1], a[1][2])):
        disc = a1 * a1 - LD(4) * a2
        if disc < 0:
            r = max(r, np.sqrt(a2))
        else:
            r = max(r, (abs(a1) + np.sqrt(disc)) / LD(2))
    return r


def response_sq(hz, f):
    """|H(e^{j 2 pi f / hz})|^2 of the cascade, from the long-double coefficients."""
    b, a, _ = k_filter_ld(hz)
    w = LD(2) * pi_ld() * LD(f) / LD(int(hz))
    # in powers of u = 1 - z^-1 = 2 sin(w/2) (sin(w/2) + j cos(w/2)): c0 + c1 z^-1 + c2 z^-2 =
    # (c0 + c1 + c2) - (c1 + 2 c2) u + c2 u^2.  At 40 Hz the direct form 1 - 2 cos w + cos 2w loses 1 / w^2 = 1e5 of its
    # digits; here the two sums of coefficients are exact (neighbours within a factor of 2) and the three terms are of
    # the size of the result
    sh, ch = np.sin(w / LD(2)), np.cos(w / LD(2))
    ure, uim = LD(2) * sh * sh, LD(2) * sh * ch
    u2re, u2im = ure * ure - uim * uim, LD(2) * ure * uim

    def mag_sq(c):
        k0, k1 = (c[0] + c[1]) + c[2], c[1] + LD(2) * c[2]
        re = k0 - k1 * ure + c[2] * u2re
        im = -k1 * uim + c[2] * u2im
        return re * re + im * im

    out = LD(1)
    for k in range(2):
        out *= mag_sq(b[k]) / mag_sq(a[k])
    return out


def hop_energies_ld(x, hz):
    """z_j of x at hz over its full hops (long double [nh]) and H: both stages sample by sample (transposed direct
    form II, as step 1 states it) from zero state, y^2 added in ascending order inside each hop."""
    b, a, H = k_filter_ld(hz)
    nh = len(x) // H
    z = np.zeros(nh, dtype=LD)
    if nh == 0:
        return z, H
    xs = (np.asarray(x[: nh * H], dtype=LD) / LD(FULL_SCALE)).tolist()  # (a list of long-double scalars)
    b10, b11, b12, a11, a12 = b[0][0], b[0][1], b[0][2], a[0][1], a[0][2]
    b20, b21, b22, a21, a22 = b[1][0], b[1][1], b[1][2], a[1][1], a[1][2]
    s0 = s1 = t0 = t1 = LD(0)
    i = 0
    for j in range(nh):
        acc = LD(0)
        for xn in xs[i:i + H]:
            w = b10 * xn + s0
            s0 = b11 * xn - a11 * w + s1
            s1 = b12 * xn - a12 * w
            y = b20 * w + t0
            t0 = b21 * w - a21 * y + t1
            t1 = b22 * w - a22 * y
            acc += y * y
        z[j] = acc
        i += H
    return z, H


def loud_ld(ms):
    """-0.691 + 10 log10(ms) in long double; -inf for 0."""
    ms = np.asarray(ms, dtype=LD)
    with np.errstate(divide="ignore"):
        return LD(-0.691) + LD(10) * np.log10(ms)


def _sliding(z, k, H):
    z = np.asarray(z, dtype=LD)
    if z.size < k:
        return np.zeros(0, dtype=LD)
    out = np.zeros(z.size - k + 1, dtype=LD)
    for i in range(k):
        out += z[i:z.size - k + 1 + i]
    return out / (LD(k) * LD(H))


def _margin(l, gate):
    l = np.asarray(l, dtype=LD)
    return float(np.min(np.abs(l - LD(gate)))) if l.size else math.inf


def _gated(ms, rel):
    """(the values above both gates, the smallest margin of the two comparisons)"""
    l = loud_ld(ms)
    margin = _margin(l, -70.0)
    keep = l > LD(-70)
    if not keep.any():
        return ms[:0], margin
    gamma = loud_ld(np.sum(ms[keep]) / LD(int(keep.sum()))) + LD(rel)
    margin = min(margin, _margin(l[keep], gamma))
    return ms[keep & (l > gamma)], margin


class Measure:
    """What the definition gives for one utterance, every loudness as a long double (or -inf / nan)."""

    def __init__(self, z, H):
        z = np.asarray(z, dtype=LD)
        self.nh = int(z.size)
        bl = _sliding(z, BLOCK_HOPS, H)
        kept, self.margin = _gated(bl, -10.0)
        self.lufs = loud_ld(np.sum(kept) / LD(kept.size)) if kept.size else LD(-math.inf)
        self.max_momentary = loud_ld(bl.max()) if bl.size else LD(-math.inf)
        w = _sliding(z, WINDOW_HOPS, H)
        self.max_short_term = loud_ld(w.max()) if w.size else LD(-math.inf)
        kept, m = _gated(w, -20.0)
        self.margin = min(self.margin, m)
        kept = np.sort(kept)
        self.n_windows = n = int(kept.size)
        self.lra, self.lra_low, self.lra_high = LD(0), LD(math.nan), LD(math.nan)
        if n:
            ranks = [int(math.floor((n - 1) * p + 0.5)) for p in (0.10, 0.95)]
            lk = loud_ld(kept)
            for r in ranks:  # a neighbour at the same loudness would make the selected element a matter of rounding
                for q in (r - 1, r + 1):
                    if 0 <= q < n:
                        self.margin = min(self.margin, float(abs(lk[r] - lk[q])))
            lo, hi = kept[ranks[0]], kept[ranks[1]]
            self.lra, self.lra_low, self.lra_high = LD(10) * np.log10(hi / lo), lk[ranks[0]], lk[ranks[1]]

    def check_margin(self, what):
        if self.margin < MARGIN:
            raise AssertionError("%s: a value within %.3g LU of a gate (or of its neighbour in rank): the table, not "
                                 "the library, is at fault" % (what, self.margin))


def measure(x, hz):
    z, H = hop_energies_ld(x, hz)
    return Measure(z, H)


def peak_db_ld(x):
    """20 log10(max |x| / 32768) in long double; -inf for silence or no sample."""
    x = np.asarray(x, dtype=np.float64)
    m = float(np.max(np.abs(x))) if x.size else 0.0
    return LD(20) * np.log10(LD(m) / LD(FULL_SCALE)) if m > 0 else LD(-math.inf)
