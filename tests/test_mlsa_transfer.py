"""The CPU oracle's synthesis filters against their transfer functions (tests/mlsa_ref.py) on the whole case table
(tests/mlsa_cases.py): this pins oracle/jbo_hot.c where no golden of the reference does -- the goldens reach one shape
(order 34, alpha 0.55, frame period 240) -- and with it every PCM test of the suite that compares a kernel with the
oracle.  No GPU.  The MGLSA cases run the oracle's filter loop on given coefficients (O.vocoder(coef=, cfirst=)).

Gates, all 8 x the worst value measured over the table (profiles/r20_mlsa_transfer.txt, written by
tests/tools/mlsa_transfer_study.py), u = 2^-53:
  * max |oracle - reference| <= 8 x 31.3 u x peak for Stage::Zero (worst: order 63, alpha 0.77, noise) and
    8 x 475.3 u x peak for the MGLSA cascade (worst: twelve stages; these filters, converted from line spectral pairs,
    ring for up to 20,000 samples and their rounding errors with them);
  * the reference alone: the impulse response on N and on 2N points agrees to 1e-16 of its peak and what lies
    behind N is under 1e-16 of the peak (the slow case, order 49 at alpha 0.77, needs N = 8192);
  * the pulse positions of the reference excitation stay 1e-6 clear of the rounding of k p (asserted where they are
    computed);
  * post-filter energy (X1, unpinned by the reference's goldens): O.b2en within 8 x 8.5 u of the energy integral of
    the REVERSED coefficient sequence (tests/mlsa_ref.py reversed_energy), and the b_0 shift of O.postfilter_mcp
    within 8 x 4.1 u of ln(e1 / e2) / 2.  Shapes gated are those where b2en's truncation to 576 terms is below its
    rounding; NOT gated, because the truncation shows: nmcp 25 at alpha 0.55 (4.6e-13), nmcp 35 at alpha 0.55 (6.9e-7),
    nmcp 50 at alpha 0.77 (5.7e-5) -- the test asserts that these are off by more than the gate, so that the
    distinction is kept honest.  The unreversed integral is off by a factor of 1.5 to 2.5.

What the gates catch, measured on scratch copies of the oracle with one change each (same profile): the cases of the
68 that end over their gate, and the smallest error among those, in gates:
  * PPADE[3] 0.01369984 -> 0.01369985                 the 50 Stage::Zero cases, the least by 1.9e3 x
  * the (i & 1) sign rule flipped                      the 50 Stage::Zero cases, the least by 4.4e12 x
  * the FIR remainder loop one tap short               38 (every case with (nmcp - 2) % 4 != 0), the least by 6.4e10 x
  * MGLSA: ds[i - 1] read before its update            the 18 MGLSA cases, the least by 9.2e10 x
  * the interpolation one sample ahead (i + 1)         the 2 ramp cases, the least by 5.6e11 x
Each change shows only in the cases that reach the code, and there by three orders of magnitude or more."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mlsa_cases as C
from tests import mlsa_ref as R

pytestmark = pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")

WORST_ZERO_U, WORST_MGLSA_U = 31.3, 475.3  # measured (profiles/r20_mlsa_transfer.txt)
GATE_ZERO_U, GATE_MGLSA_U = 8 * WORST_ZERO_U, 8 * WORST_MGLSA_U
# post-filter energy: shapes where the 576-term truncation of b2en is below its rounding, and three where it is not
PF_SHAPES = [(3, 0.42), (3, 0.55), (5, 0.42), (5, 0.55), (8, 0.42), (12, 0.42), (12, 0.55), (25, 0.42), (4, 0.77),
             (8, 0.3), (16, 0.3)]
PF_TRUNCATED = [(25, 0.55), (35, 0.55), (50, 0.77)]
PF_BETA = 0.3
GATE_B2EN_U, GATE_SHIFT_U = 8 * 8.5, 8 * 4.1
PF_GRID = 4096

def gate_of(case):
    return GATE_MGLSA_U if case.stage else GATE_ZERO_U


def test_long_double_is_wider_than_f64():
    assert np.finfo(R.LD).eps <= 2.0 ** -63


def test_table_covers_what_it_says():
    zero = [C.build_case(s, "pulses") for s in C.ZERO_SHAPES]
    assert {c.nmcp for c in zero} == {2, 3, 4, 5, 6, 7, 25, 35, 50, 64}
    assert {(c.nmcp - 2) % 4 for c in zero} == {0, 1, 2, 3}
    assert {c.alpha for c in zero} == {0.0, 0.42, 0.55, 0.77}
    assert {c.fperiod for c in zero} == {37, 64, 65, 80, 240}
    assert sum(c.volume != 1.0 for c in zero) == 2
    assert all(24 <= c.frames <= 40 for c in zero)
    assert {C.build_case(s, "noise").stage for s in C.MGLSA_SHAPES} == {1, 2, 4, 8, 9, 12}
    assert len(C.all_cases()) == 3 * (len(C.ZERO_SHAPES) + len(C.MGLSA_SHAPES)) + 2
    vuv = C.build_case("n6_a55_f240", "vuv").voiced
    assert vuv[0] and vuv[-1] and not vuv.all() and np.count_nonzero(np.diff(vuv.astype(int))) == 2
    ramp = C.build_case("ramp_noise_n35_a55_f80")
    assert ramp.ramp and len(np.unique(ramp.mc[:, 0])) == ramp.frames and np.all(ramp.mc[:, 1:] == ramp.mc[0, 1:])


def test_reference_pieces():
    """The pieces of the reference against closed forms: the all-pass has modulus 1 and Phi_1 = (1 - a^2) z^-1 / (1 -
    a z^-1) expands to (1 - a^2) a^(n-1) from sample 1; R(u) R(-u) = 1; a first-order response decays as alpha^n, so
    the grid search must stop where alpha^N falls under the tolerance; convolve() against numpy's direct sum; the
    pulse positions against the sample-by-sample counter; the gain schedule against a walk over the frames."""
    a = 0.55
    zi = R.unit_circle(64)
    phi1 = R.warped_sum([1.0], a, zi)
    h = np.fft.ifft(phi1).real
    want = np.concatenate(([0.0], (1 - a * a) * a ** np.arange(63)))
    assert float(np.abs(h - want).max()) <= 1e-16  # (a^64 = 2e-17 wraps around)
    phi3 = R.warped_sum([0.0, 0.0, 1.0], a, zi)
    assert float(np.abs(np.abs(phi3 / phi1) - 1).max()) <= 1e-18
    u = (0.7 * phi1 - 0.3 * phi3)
    assert float(np.abs(R.pade(u) * R.pade(-u) - 1).max()) <= 1e-17
    hh, N, m = R.impulse_response(lambda n: R.warped_sum([1.0], 0.99, R.unit_circle(n)))
    assert N == 4096 and 0.99 ** N < R.ALIAS_TOL < 0.99 ** (N // 2)
    rng = np.random.default_rng(5)
    x, k = rng.standard_normal(300), rng.standard_normal(77)
    assert float(np.abs(R.convolve(x, k) - np.convolve(x.astype(R.LD), k.astype(R.LD))[:300]).max()) <= 1e-16
    for p in (C.PITCH, 20.5001, 333.3337):
        cnt, pos = p, []
        for n in range(5000):
            cnt += 1.0
            if cnt >= p:
                cnt -= p
                pos.append(n)
        assert np.array_equal(R.pulse_positions(p, 5000), pos)
    with pytest.raises(AssertionError):
        R.pulse_positions(57.25, 5000)  # 4 p is an integer
    b0, f = rng.standard_normal(6), 7
    sched, c = [], b0[0]
    for t in range(6):
        for i in range(f):
            sched.append(c + i * (b0[t] - c) / f)
        c = b0[t]
    assert float(np.abs(R.gain_schedule(b0, f) - np.asarray(sched)).max()) <= 4 * R.U  # (the walk is in f64)


@pytest.mark.parametrize("shape", C.SHAPES)
def test_oracle_against_transfer_function(shape):
    for case in C.shape_cases(shape):
        h, N, m = C.response(case)
        assert m["agree"] <= R.ALIAS_TOL and m["tail"] <= R.ALIAS_TOL, (case.name, m)
        for nlpf in (0, 1):
            want = C.expected_pcm(case, nlpf)
            got = C.oracle_pcm(case, nlpf)
            assert got.shape == want.shape and np.isfinite(got).all()
            e = C.err_in_u(got, want)
            print("%-34s nlpf %d  N %6d  peak %.3g  err %.2f u (gate %g u)" % (case.name, nlpf, N, float(np.abs(want).max()),
                                                                              e, gate_of(case)))
            assert e <= gate_of(case), (case.name, nlpf, e)
    if shape.startswith("slow"):
        # no 18-frame warm-up holds this response: 18 frames behind its peak it is still above 1e-6 of it
        k = 18 * case.fperiod
        assert N >= 8192 and float(np.abs(h[k:]).max() / np.abs(h).max()) > 1e-6


def test_excitation_draws_the_noise_the_oracle_draws():
    """The reference excitation against the oracle's dump, sample for sample: the pulses' places and sqrt(p), the noise
    stream on unvoiced samples only (nlpf = 0) or on every sample (nlpf = 1), where a one-cell ring buffer returns
    noise + (pulse - noise)."""
    for shape in ("n6_a55_f240", "n3_a55_f37"):
        for case in C.shape_cases(shape):
            for nlpf in (0, 1):
                lpf = np.ones((case.frames, 1)) if nlpf else None
                _, exc, _ = O.vocoder(case.fs, case.fperiod, case.alpha, 1.0, case.lf0_track(), case.mc, lpf, dumps=True)
                want = R.excitation(case.voiced, case.fperiod, R.pitch_of(case.lf0, case.fs), nlpf, C.noise())
                assert np.array_equal(want != 0, exc != 0), (case.name, nlpf)
                assert float(np.abs(want - exc).max()) <= 4 * R.U * float(np.abs(want).max()), (case.name, nlpf)


def pf_cepstrum(nmcp, alpha):
    rng = np.random.default_rng(nmcp * 100 + int(alpha * 100))
    return np.concatenate(([rng.uniform(-0.5, 1.0)], 0.5 * rng.standard_normal(nmcp - 1) / np.sqrt(np.arange(1, nmcp))))


def postfilter_errors(nmcp, alpha):
    """(|E_M - E_2M| / E, O.b2en's relative error in u, the b_0 shift's absolute error in u)."""
    mc = pf_cepstrum(nmcp, alpha)
    b = np.asarray(R.mc2b(mc, alpha), dtype=np.float64)
    e1, e1d = R.reversed_energy(b, alpha, PF_GRID), R.reversed_energy(b, alpha, 2 * PF_GRID)
    b2en = float(abs(R.LD(O.b2en(b, alpha)) - e1d) / e1d) / R.U
    bi = R.mc2b(mc, alpha)
    bo = R.mc2b(O.postfilter_mcp(mc, alpha, PF_BETA), alpha)
    e2d = R.reversed_energy(np.asarray(R.postfiltered_b(bi, alpha, PF_BETA), dtype=np.float64), alpha, 2 * PF_GRID)
    ein = R.reversed_energy(np.asarray(bi, dtype=np.float64), alpha, 2 * PF_GRID)
    shift = float(abs((bo[0] - bi[0]) - np.log(ein / e2d) / 2)) / R.U
    # everything behind b_0 is what postfiltered_b says, to rounding
    assert float(np.abs(bo[1:] - R.postfiltered_b(bi, alpha, PF_BETA)[1:]).max()) <= 8 * R.U * float(np.abs(bi).max())
    return float(abs(e1 - e1d) / e1d), b2en, shift


@pytest.mark.parametrize("nmcp,alpha", PF_SHAPES)
def test_postfilter_energy_against_the_integral(nmcp, alpha):
    grid, b2en, shift = postfilter_errors(nmcp, alpha)
    print("nmcp %d alpha %g: grid %.1e, b2en %.2f u, shift %.2f u" % (nmcp, alpha, grid, b2en, shift))
    assert grid <= 1e-17
    assert b2en <= GATE_B2EN_U and shift <= GATE_SHIFT_U
    # the sequence as it stands, not reversed, is another number altogether
    mc = pf_cepstrum(nmcp, alpha)
    b = np.asarray(R.mc2b(mc, alpha), dtype=np.float64)
    plain = R.reversed_energy(np.asarray(R.mc2b(R.b2mc(b, alpha)[::-1], alpha), dtype=np.float64), alpha, PF_GRID)
    assert abs(float(plain) / O.b2en(b, alpha) - 1) > 1e-3


@pytest.mark.parametrize("nmcp,alpha", PF_TRUNCATED)
def test_postfilter_energy_where_the_truncation_shows(nmcp, alpha):
    """Recorded, not gated: b2en keeps 576 terms of the cepstrum and of the impulse response (coefficients.rs:76)."""
    grid, b2en, shift = postfilter_errors(nmcp, alpha)
    print("nmcp %d alpha %g: grid %.1e, b2en %.3g u, shift %.3g u" % (nmcp, alpha, grid, b2en, shift))
    assert b2en > GATE_B2EN_U and b2en * R.U < 1e-3
