"""The frame-to-frame part of the vocoder, without a GPU: the extended-precision reference (tests/vocoder_tv_ref.py) checked
against what already stands, then the CPU oracle held to it on the whole table of tests/vocoder_tv_cases.py -- pitch
interpolation, the low-pass mixed excitation at every tap count the launch code tells apart, every filter coefficient
interpolating, beta > 0 at PCM level.

The reference first (nothing is held to it before these pass):
  * its warped delay line, one dense matrix, has the impulse responses of Phi_1 .. Phi_K that mlsa_ref evaluates on the
    unit circle;
  * with one repeated row it gives the PCM of mlsa_ref.expected_pcm (transfer function, inverse FFT, convolution) on four
    Stage::Zero shapes (orders 3, 34, 49 and 63) and two MGLSA shapes, and on the two RAMP shapes the gain-schedule form,
    within AGREE_U = 4 u x peak: mlsa_ref allows itself 1e-16 of the response's peak twice (ALIAS_TOL: grid, tail) and
    takes sqrt(p) in f64.  Measured: 0.004 to 0.81 u (profiles/r26_vocoder_tv.txt) -- three orders under the f64 gates;
  * the gather form of the excitation with one tap of 1.0 and a constant f64 period equals mlsa_ref.excitation bit for
    bit once rounded to f64;
  * the closed-form schedule equals mlsa_ref.gain_schedule in its first column; periods() clamps and maps NODATA to 0;
  * every case of the table keeps its pulse decisions 1e-6 samples clear of a tie.

Then the oracle.  Measures: the excitation's max error over the case's peak; PCM in u x peak (mlsa_cases.err_in_u).
Gates: 8 x the worst measured per class (profiles/r26_vocoder_tv.txt, written by tests/tools/vocoder_tv_study.py):
  excitation   worst 4.91e-15 of the peak (frame period 240: the f64 loop ADDS the pitch increment 240 times and takes
               sqrt of the sum, the reference has start + i inc in closed form)
  Stage::Zero  worst 158 u (frame period 240, against 31 u frozen: the same drift of c += cinc, 240 roundings in b_0,
               which the output follows through exp(b_0); the shapes of 80 samples and less stay under 60 u)
  with beta    worst 48.4 u
  MGLSA        worst 4198 u (against 475 u frozen; these cascades reach levels of 1e15)
JB_VOCODER_TV_REPORT=<file> appends the measured worst values per class.

What the gates see, on scratch copies of the oracle with one change each (same profile; the factor is the largest
err / gate over the table): the coefficient increment before df 2.8e11 x, the first frame from the filtered row 1.4e12 x
(the beta shapes alone, as it must be), the pitch increment from the new period on both sides 2.9e13 x, the antipode at
nlpf / 2 4.2e13 x (the even tap counts alone), the taps of the destination's frame 1.5e13 x, no noise on voiced samples
3.4e13 x.  NOT seen: the coefficients' end-of-frame snap dropped, 0.19 x -- c + fperiod ((cc - c) / fperiod) IS cc up
to fperiod roundings, so the snap of the coefficients only resets a drift of the size the gates allow for, and the
next frame's increment is taken from wherever the coefficients stand, so without the snap the drift does not even
accumulate over the frames: no table can see it."""
import os
import time

import numpy as np
import pytest

from tests import mlsa_cases as C
from tests import mlsa_ref as R
from tests import vocoder_tv_cases as T
from tests import vocoder_tv_ref as V

pytestmark = pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")

WORST, GATE, AGREE_U, FROZEN = T.WORST, T.GATE, T.AGREE_U, T.FROZEN

_worst = {}
_t0 = time.time()


def _note(key, value):
    _worst[key] = max(_worst.get(key, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    path = os.environ.get("JB_VOCODER_TV_REPORT")
    if path and _worst:
        with open(path, "a") as fh:
            fh.write("oracle against the time-varying reference (tests/test_vocoder_tv_ref.py), %.1f s for the file\n" % (time.time() - _t0))
            for k, v in _worst.items():
                fh.write("%-28s %12.4g\n" % (k, v))


def test_warp_operator_has_the_responses_of_phi_k():
    for alpha, K in ((0.55, 6), (0.0, 4), (0.77, 9)):
        M, g = V.warp_operator(K, alpha)
        n = 1024 if alpha < 0.7 else 4096
        s, h = np.zeros(K, dtype=R.LD), np.zeros((n, K), dtype=R.LD)
        for i in range(1, n):  # u = the unit impulse at 0
            s = M @ s + (g if i == 1 else 0)
            h[i] = s
        zi = R.unit_circle(n)
        for k in range(K):
            want = np.fft.ifft(R.warped_sum(np.eye(K)[k], alpha, zi)).real
            assert float(np.abs(h[:, k] - want).max()) <= 1e-17, (alpha, k)


@pytest.mark.parametrize("shape,exc", FROZEN)
def test_frozen_rows_agree_with_the_transfer_function(shape, exc):
    case = C.build_case(shape, exc)
    want = C.expected_pcm(case, 1)
    e, margin = V.excitation(case.lf0_track(), case.fs, case.fperiod, np.ones((case.frames, 1)), C.noise())
    assert margin >= T.MARGIN
    if case.stage:
        c = C.oracle_coefficients(case)
        rows, first = np.tile(c, (case.frames, 1)), c
    else:
        rows, first = V.zero_rows(case.mc, case.alpha, 0.0)
    got = V.synthesize([e], [rows], [first], case.fperiod, case.alpha, case.volume, case.stage)[0]
    a = C.err_in_u(got, want)
    print("%-34s agreement %.3f u x peak" % (case.name, a))
    _note("agreement with mlsa_ref / u", a)
    assert a <= AGREE_U, (case.name, a)


def test_gather_form_with_one_unit_tap_is_the_plain_excitation():
    for shape in ("n6_a55_f240", "n3_a55_f37"):
        for case in C.shape_cases(shape):
            p = R.pitch_of(case.lf0, case.fs)
            want = R.excitation(case.voiced, case.fperiod, p, 1, C.noise())
            pulse, margin = V.pulses(np.where(case.voiced, R.LD(p), R.LD(0)), case.fperiod)
            got = V.mixed_excitation(pulse, case.voiced, case.fperiod, np.ones((case.frames, 1)), C.noise())
            assert margin >= T.MARGIN
            assert np.array_equal(np.asarray(got, dtype=np.float64), want), case.name
            # and without a ring buffer
            want = R.excitation(case.voiced, case.fperiod, p, 0, C.noise())
            got = V.mixed_excitation(pulse, case.voiced, case.fperiod, None, C.noise())
            assert np.array_equal(np.asarray(got, dtype=np.float64), want), case.name


def test_schedule_and_periods():
    rng = np.random.default_rng(3)
    rows, first = rng.standard_normal((6, 4)), rng.standard_normal(4)
    s = V.schedule(rows, rows[0], 7)
    assert float(np.abs(s[:, 0] - R.gain_schedule(rows[:, 0], 7)).max()) <= 1e-18
    assert np.array_equal(s[:7], np.tile(rows[0].astype(R.LD), (7, 1)))  # the first frame is flat ...
    s = V.schedule(rows, first, 7)
    assert np.array_equal(s[0], first.astype(R.LD)) and not np.array_equal(s[6], s[0])  # ... unless it starts elsewhere
    assert np.array_equal(s[7::7], rows[:-1].astype(R.LD))  # the target is reached at the next frame's sample 0
    mid = s[7 + 3]
    assert float(np.abs(mid - (rows[0] + 3 * (rows[1] - rows[0]) / 7)).max()) <= 4 * R.U
    p = V.periods([R.NODATA, 1.0, np.log(160.0), 12.0], 16000)
    assert p[0] == 0 and abs(float(p[2]) - 100.0) < 1e-12
    assert abs(float(p[1]) - 16000 / np.exp(V.MIN_LF0)) < 1e-9 and abs(float(p[3]) - 16000 / np.exp(V.MAX_LF0)) < 1e-12


def test_pulse_walk_on_a_glide_a_snap_and_a_restart():
    """By hand on a frame period of 4: the period 2.5 restarts the counter (a pulse on sample 0), the glide to 4.5 moves
    the period by 0.5 a sample and reaches 4.5 only by the snap at the frame's end, an unvoiced frame clears it."""
    pulse, margin = V.pulses(np.array([2.5, 4.5, 0.0, 3.25], dtype=R.LD), 4)
    # frame 0: counter 2.5 -> 3.5 fires (1.0) -> 2.0 -> 3.0 fires (0.5) -> 1.5
    # frame 1: periods 2.5, 3.0, 3.5, 4.0: 2.5 fires (0.0) -> 1.0 -> 2.0 -> 3.0; frame 3: restart, sample 0 fires
    want = np.zeros(16, dtype=R.LD)
    want[[0, 2, 4]], want[[12, 15]] = np.sqrt(R.LD(2.5)), np.sqrt(R.LD(3.25))  # (15: 1.0 -> 2 -> 3 -> 4 >= 3.25)
    assert float(np.abs(pulse - want).max()) <= 1e-18
    assert margin == 0.0  # (frame 1, sample 0: 2.5 against 2.5 -- a tie, which the table's tracks must stay clear of)


def test_table_covers_what_it_says():
    ex = T.EXC_SHAPES
    assert {(f, n) for f, n, _, _ in ex.values()} >= {(240, 31), (80, 15), (32, 31), (30, 31), (64, 64), (37, 2), (65, 64),
                                                       (80, 16), (29, 15), (64, 65), (37, 39), (37, 2047), (80, 1), (80, 0)}
    assert all(12 <= t <= 40 for f, n, _, t in ex.values() if n != 2047)
    assert ex["any_f37_l2047"][3] * 37 > 2047 and 2046 // 37 + 1 == 56  # the window of a late sample: 56 frames
    for s in ("split_f240_l31", "split_f80_l15", "split_f32_l31"):
        rows, per = T.exc_utt(s, "glide")[0].lpf, T.exc_utt(s + "_frame", "glide")[0].lpf
        assert np.all(rows == rows[0]) and not np.any(np.all(per[1:] == per[:-1], axis=1))
    assert T.exc_utt("any_f37_l39", "one")[0].samples < 39 and T.exc_utt("staged_f80_l1", "glide")[0].lpf[0, 0] != 1.0
    runs = T.exc_utt("staged_f80_l16", "runs")[0].voiced.astype(int)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], runs, [0]))))
    assert {1, 2, 3} <= set(edges[1::2] - edges[0::2]) and {1, 2} <= set(edges[2::2] - edges[1:-1:2])
    for s in ("split_f240_l31", "any_f29_l15"):
        f = ex[s][0]
        p = np.concatenate([V.periods(u.lf0, T.FS) for u in T.exc_cases(s)]).astype(np.float64)
        assert p[p > 0].min() < 6 and p.max() > f
    octave = V.periods(T.exc_utt("staged_f64_l64", "octave")[0].lf0, T.FS).astype(np.float64)
    assert (octave[2:8] / octave[:6]).min() > 1.8  # a factor of two inside two frames
    fs = T.FILTER_SHAPES
    zero = [v for v in fs.values() if v[0] == 0]
    assert {v[1] for v in zero} == {3, 5, 25, 35, 50, 64} and {v[2] for v in zero} == {0.0, 0.42, 0.55, 0.77}
    assert {v[3] for v in zero} == {37, 64, 65, 80, 240} and sum(v[4] != 1.0 for v in zero) == 1
    assert sorted(v[6] for v in zero if v[6]) == [0.1, 0.3] and sum(v[1] > 35 for v in fs.values()) == 2
    assert {v[0] for v in fs.values() if v[0]} == {1, 4, 8, 9} and sum(v[8] for v in fs.values()) == 1
    assert sorted(v[7] for v in fs.values() if v[7] not in (15, 31)) == [0, 1]
    lpf = T.filter_utt("z25_a55_f80_table", "glide")[0].lpf
    assert np.all(lpf == lpf[0]) and np.array_equal(lpf, T.filter_utt("z25_a55_f80_table", "runs")[0].lpf)
    assert all(12 <= v[5] <= 40 for v in fs.values())
    mc = T.filter_utt("z35_a55_f240", "glide")[0].spectrum
    step = np.abs(np.diff(mc, axis=0))
    assert step[:, :4].mean() > 0.1 and np.all(step.max(axis=0) > 0)  # every coefficient moves, the low orders by tenths


def test_every_pulse_decision_is_clear_of_a_tie():
    m = T.margins()
    assert len(m) == 5 * len(T.EXC_SHAPES) + 3 * len(T.FILTER_SHAPES)
    worst = min(m.items(), key=lambda kv: kv[1])
    print("smallest margin: %s %.3g samples" % worst)
    assert worst[1] >= T.MARGIN, worst
    assert not T.RESEED or set(T.RESEED) <= set(m)


@pytest.mark.parametrize("shape", list(T.EXC_SHAPES))
def test_oracle_excitation_against_the_gather_form(shape):
    for u in T.exc_cases(shape):
        want = T.expected_excitation(shape, u.name.rsplit("-", 1)[1])
        got = T.oracle_excitation(u)
        assert got.shape == want.shape and np.isfinite(got).all()
        e = T.exc_err(got, want)
        print("%-30s %6d samples  peak %.3g  err %.3g of the peak (gate %.3g)" % (u.name, u.samples, float(np.abs(want).max()), e, GATE["exc"]))
        _note("excitation / peak", e)
        assert e <= GATE["exc"], (u.name, e)
        fired = np.asarray(V.pulses(V.periods(u.lf0, T.FS), u.fperiod)[0] != 0)
        if u.lpf.shape[1] == 0:  # without a ring buffer the pulses themselves are in the output
            assert np.array_equal(fired, (got != 0) & np.repeat(u.voiced, u.fperiod)), u.name


@pytest.mark.parametrize("shape", list(T.FILTER_SHAPES))
def test_oracle_pcm_against_the_time_varying_filters(shape):
    cls = T.filter_class(shape)
    for u, want in zip(T.filter_cases(shape), T.expected_pcm(shape)):
        got = T.oracle_pcm(shape, u)
        assert got.shape == want.shape and np.isfinite(got).all()
        e = C.err_in_u(got, want)
        print("%-30s %6d samples  peak %.3g  err %.2f u (gate %g u)" % (u.name, u.samples, float(np.abs(want).max()), e, GATE[cls]))
        _note("PCM %s / u" % cls, e)
        assert e <= GATE[cls], (u.name, e)


def test_beta_moves_the_first_frame():
    """What the beta shapes are for: the first frame runs from the unfiltered row to the filtered one, so it differs
    from both a flat first frame and the beta = 0 output by far more than any gate."""
    shape = "zb3_n35_a55_f65"
    u = T.filter_cases(shape)[0]
    _, _, alpha, fperiod, volume, _, beta, _, _ = T.FILTER_SHAPES[shape]
    want = T.expected_pcm(shape)[0]
    rows, first = V.zero_rows(u.spectrum, alpha, beta)
    assert float(np.abs(rows[0] - first).max()) > 1e-3
    e = T.expected_excitation(shape, "glide", True)
    flat = V.synthesize([e], [rows], [rows[0]], fperiod, alpha, volume)[0]
    assert C.err_in_u(flat[:fperiod], want[:fperiod]) > 1e6 * GATE["zero_beta"]
    assert C.err_in_u(T.expected_pcm(shape, 0.0)[0], want) > 1e6 * GATE["zero_beta"]
