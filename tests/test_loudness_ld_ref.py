"""The long-double loudness reference (tests/loudness_ld_ref.py) and its table (tests/loudness_ld_cases.py) checked on
their own, without a GPU: the coefficients against the BS.1770 table, the cascade against the transfer function it
implements, the whole evaluation against the f64 one on the existing tests' signals, and the table's classes against
the tiling rule."""
import math

import numpy as np
import pytest

from tests import loudness_ld_cases as T
from tests import loudness_ld_ref as R
from tests.fbank_ref import have_long_double
from tests.loudness_ref import integrated, k_filter

pytestmark = pytest.mark.skipif(not have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")
LD = R.LD
EPS = float(np.finfo(LD).eps)


def test_coefficients_at_48k_round_to_the_bs1770_table():
    b, a, H = R.k_filter_ld(48000)
    assert H == 4800
    table_b = [[1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -2.0, 1.0]]
    table_a = [[1.0, -1.69065929318241, 0.73248077421585], [1.0, -1.99004745483398, 0.99007225036621]]
    # the table has 14 decimals (tests/test_loudness_abi.py holds the library to 1e-14 of it)
    for got, want, tol in ((b[0], table_b[0], 5e-15), (a[0], table_a[0], 5e-15), (b[1], table_b[1], 0.0),
                           (a[1], table_a[1], 5e-15)):
        for g, w in zip(got, want):
            assert abs(float(g - LD(w))) <= tol, (float(g), w)
            assert round(float(g), 14) == w


@pytest.mark.parametrize("hz", [3400, 8000, 48000, 192000, 614390])
def test_coefficients_are_the_f64_formula_to_its_rounding(hz):
    b, a, H = R.k_filter_ld(hz)
    rb, ra, rh = k_filter(hz)
    assert H == rh
    # f64: tan, three or four operations and a division on values of order 1, K^2 - 1 and 1 - K/Q + K^2 exact to an ulp
    # of their terms: 8 ulp of the largest coefficient (2.7) bounds the difference
    assert float(np.max(np.abs(b - rb.astype(LD)))) <= 8 * 2.0 ** -52 * 2.0
    assert float(np.max(np.abs(a - ra.astype(LD)))) <= 8 * 2.0 ** -52 * 2.0


@pytest.mark.parametrize("hz", [8000, 48000, 96000])
@pytest.mark.parametrize("f", [997, 40])
def test_steady_state_energy_of_a_sine_is_the_transfer_function(hz, f):
    """x = A sin(2 pi f n / hz): after the transient y = A |H| sin(. + phase), and over one second -- ten hops, a whole
    number f of periods, so the cosine term of sin^2 sums to zero -- the hop energies add up to |H|^2 A^2 (10 H) / 2.

    Level.  The transient decays as r^n, r the largest pole modulus (the high-pass: -ln r = 239 per second at any
    rate); the sum starts after one second, where r^(hz) < e^-230 is below any rounding.  What is left is the
    recursion's rounding: an error of eps per operation reaches y through the state's impulse response, whose l1 norm
    is at most 2 / (1 - r) per stage, so |dy| <= 16 eps / (1 - r) of the largest internal signal, A itself, and the
    energy is off by twice that relative to |H| A.  At 96 kHz and 40 Hz (|H|^2 = 0.28, 1 - r = 1.2e-3) that is
    2.7e-15, the largest of the six; the differences seen are 3e-19 to 7e-17."""
    H = R.hop_of(hz)
    assert 10 * H == hz
    A = 0.5
    n = np.arange(20 * H)
    # (made in long double: samples rounded to f64 would be a sine plus 1e-16 of noise)
    x = (LD(A) * LD(32768.0)) * np.sin(LD(2) * R.pi_ld() * LD(f) * n.astype(LD) / LD(hz))
    z, _ = R.hop_energies_ld(x, hz)
    r = float(R.pole_radius(hz))
    assert r ** hz < 1e-99
    h2 = R.response_sq(hz, f)
    want = h2 * LD(A) * LD(A) * LD(10 * H) / LD(2)
    got = np.sum(z[10:20])
    level = 2.0 * 16.0 * EPS / (1.0 - r) / math.sqrt(float(h2))
    rel = float(abs(got - want) / want)
    print("%d Hz, %d Hz: |H|^2 %.6f, relative error %.3e, level %.3e" % (hz, f, float(h2), rel, level))
    assert rel <= level
    assert level < 1e-13  # three orders under anything an f64 evaluation resolves in a sum of hz terms


def _existing_signals():
    """The signals of tests/test_gpu_loudness.py::test_seam_against_numpy (the synthesized sentence apart) and of
    ::test_seam_at_other_rates at two rates."""
    IN, H = 48000, 4800
    rng = np.random.default_rng(7)
    out = [(IN, 32768.0 * np.sin(2 * np.pi * 997 * np.arange(2 * IN) / IN))]
    for N in (4 * H - 1, 4 * H, 4 * H + 1, 7 * H - 1, 7 * H + 1, 23 * H + 1):
        out.append((IN, rng.standard_normal(N) * 3000.0))
    out.append((IN, np.zeros(9 * H)))
    out.append((IN, rng.standard_normal(9 * H) * 0.02))
    loud = rng.standard_normal(12 * H) * 8000.0
    out.append((IN, np.concatenate([loud, loud[: 30 * H // 3] * 0.01, loud[:6 * H] * 0.01])))
    for hz in (8000, 96000):
        rng = np.random.default_rng(hz)
        h = (hz + 5) // 10
        out += [(hz, rng.standard_normal(N) * 2000.0) for N in (4 * h - 1, 4 * h + 1, 9 * h + 17)]
    return out


def test_agrees_with_the_f64_evaluation_to_its_floor():
    """tests/loudness_ref.integrated on zero-mean signals: each y carries the f64 recursion's rounding, relative
    2^-53 / (1 - r) at worst (the high-pass at 96 kHz: 1 - r = 1.2e-3, so 1e-13), the sums average it down; 1e-13 of
    the mean square is 4.4e-13 LU.  (On a carried state the f64 evaluation is up to 5e-10 LU off: the table's e64.)"""
    worst = 0.0
    for hz, x in _existing_signals():
        m = R.measure(x, hz)
        m.check_margin("%d Hz, %d samples" % (hz, x.size))
        L, P = integrated(x, hz)
        e = T.err(L, m.lufs)
        worst = max(worst, e)
        assert e <= 4.4e-13, (hz, x.size, e)
        if math.isfinite(P):
            assert T.err(P, R.peak_db_ld(x)) <= 2 * np.spacing(abs(P))
        else:
            assert R.peak_db_ld(x) == -math.inf
    print("largest |L_f64 - L_ld|: %.3e LU" % worst)


def test_table_classes_follow_the_tiling_rule():
    T.check_table()
    for hz in T.RATES:
        H = T.RATES[hz][0]
        ns = [n for _, n in T.cases(hz)]
        assert max(ns) <= 430000
        assert 4 * H in ns and 5 * H + min(T.RATES[hz][3], H) + 1 in ns
    assert [n // T.RATES[T.EDGE_HZ][0] for _, n in T.edge_cases()] == list(T.EDGE_HOPS)
    assert max(n for _, n in T.edge_cases()) <= 430000


def test_gate_margins_and_dropped_blocks():
    """The lowest rate's cases (the cheapest) through the reference: every margin is clear, the carried-state and
    white cases have a finite L from 4 H samples on and -inf below, LRA of the edge cases is not 0."""
    hz = T.EDGE_HZ
    H = T.RATES[hz][0]
    for kind, n in T.cases(hz):
        m = T.reference(hz, kind, n)
        assert m.margin >= R.MARGIN
        if kind in ("quiet", "silence") or n < 4 * H:
            assert m.lufs == -math.inf
        else:
            assert math.isfinite(float(m.lufs)) and m.max_momentary >= m.lufs
        assert m.n_windows == 0 and m.max_short_term == -math.inf
    for kind, n in T.edge_cases():
        m = T.reference(hz, kind, n)
        assert m.n_windows > 0 and float(m.lra) > 3.0 and m.lra_high > m.lra_low
        assert float(m.max_short_term) <= float(m.max_momentary)
    assert T.reference(hz, "edge", 300 * H + T.EDGE_TAIL).nh == 300


def test_step_signal_drops_blocks_at_the_relative_gate():
    hz = 48000
    H = T.RATES[hz][0]
    (kind, n), = [c for c in T.cases(hz) if c[0] == "step"]
    m = T.reference(hz, kind, n)
    loud = R.measure(T.pcm(hz, kind, 8 * H), hz)
    # near the loud part's loudness (the blocks across the step stay); the absolute gate alone would read lower
    assert float(loud.lufs) - 1.5 < float(m.lufs) < float(loud.lufs)
    bl = R._sliding(T._z_ld(hz, kind), 4, H)
    assert float(R.loud_ld(np.sum(bl) / LD(bl.size))) < float(m.lufs) - 1.0
