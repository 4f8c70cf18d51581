"""The true-peak ceiling on the GPU (jb_loudness.hip k_ln_true_peak): the measurement on PCM the test holds against
the numpy restatement of the definition (tests/true_peak_ref.py), then every entry that honours the mode -- batches
with per-utterance modes, output rates, the 16-bit sink, FLAC, redo rounds, the fast invariant mode, the engine entries
and the generator.

Sizes assumed at 48 kHz: hop H = 4800 samples, two measure tiles per hop of G = 2560 and 2240 samples (tile
boundaries of a two-hop utterance at 2560, 4800, 7360, 9600).  At another rate: H = (hz + 5) // 10,
tph = ceil(H / 4096), G = 256 ceil(H / (256 tph)); a hop's first tile ends at min(G, H).

Gate of the measurement: |TP - ref| <= 1e-10 dB.  The device's twelve-term FMA chain differs from numpy's sum by at
most 12 * 2^-53 * sum|h| * max|x| with sum|h| <= 1.77, and TPlin >= max|x|: about 2e-14 dB; the table's rounding
(1e-14 per tap) adds about 1e-12 dB.  The gate is two orders above that sum."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.flac_ref import decode
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.loudness_ref import gain_db, integrated
from tests.true_peak_ref import factor, true_peak, true_peak_lin

pytestmark = pytest.mark.gpu

IN = 48000
H = 4800
G = 2560
TP_TOL = 1e-10
PAIR = 1.24054  # two equal neighbours at F = 4: h(1/2) + h(-1/2)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def close_db(got, want, tol):
    if math.isinf(want):
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= tol, (got, want)


def sample_peak(x):
    m = float(np.max(np.abs(x))) if len(x) else 0.0
    return 20.0 * math.log10(m / 32768.0) if m > 0 else -math.inf


def tile_of(hz):
    h = (hz + 5) // 10
    tph = -(-h // 4096)
    g = 256 * -(-h // (256 * tph))
    return h, min(g, h)


def quarter_sine(n, amp=20000.0):
    return amp * np.sin(0.5 * np.pi * np.arange(n) + 0.25 * np.pi)


def pair(n, k, v=10000.0):
    x = np.zeros(n)
    x[k] = x[k + 1] = v
    return x


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def native(eng):
    return eng.synthesize(SAMPLE_SENTENCE_1)


@pytest.fixture(scope="module")
def oracle_pcm():
    return np.asarray(O.Voice(VOICE).synthesize(SAMPLE_SENTENCE_1), dtype=np.float64)


def with_mode(eng, target, ceiling, mode=J.PEAK_TRUE, fast_invariant=False, out_hz=0):
    e = eng.clone()
    e.condition.set_loudness_target(target)
    e.condition.set_peak_ceiling(ceiling)
    e.condition.set_peak_mode(mode)
    e.condition.set_fast_invariant(fast_invariant)
    e.condition.set_output_sampling_frequency(out_hz)
    return e


# ---- the measurement alone (jb_true_peak_pcm_batch) ------------------------------------------------------------------
LENGTHS = (0, 1, 5, 6, 11, 12, 13, G - 1, G, G + 1, H - 1, H, H + 1, 2 * H + 13)


def test_seam_against_numpy(oracle_pcm):
    rng = np.random.default_rng(11)
    sigs = []
    for N in LENGTHS:
        white = rng.standard_normal(N) * 3000.0
        sigs += [white, 0.5 * (white + np.concatenate([np.zeros(min(N, 1)), white[:-1]])), quarter_sine(N), np.zeros(N)]
    sigs.append(oracle_pcm)
    got = J.true_peak(sigs, IN)
    peaks = J.loudness(sigs, IN)
    for i, (x, tp, (_, P)) in enumerate(zip(sigs, got, peaks)):
        close_db(tp, true_peak(x, IN), TP_TOL)
        assert tp >= P, (i, tp, P)
        if not np.any(x):
            assert tp == -math.inf, i
    # what the cases claim, on the reference alone: the long quarter-rate sine reads at least 2.9 dB over its samples,
    # the sentence a little
    long_sine = quarter_sine(2 * H + 13)
    assert true_peak(long_sine, IN) - sample_peak(long_sine) >= 2.9
    assert 0.0 < true_peak(oracle_pcm, IN) - sample_peak(oracle_pcm) < 0.1


def test_pulse_pairs_at_every_boundary():
    N = 2 * H + 13
    ks = [0, N - 2]
    for b in (G, H, H + G, 2 * H):
        ks += list(range(b - 7, b + 6))
    sigs = [pair(N, k) for k in ks]
    want = true_peak(sigs[0], IN)
    # the reference's value: 1.24054 x 10000, 1.87 dB over the sample peak
    assert true_peak_lin(sigs[0], IN) == pytest.approx(PAIR * 10000.0, abs=0.05)
    assert want - 20.0 * math.log10(10000.0 / 32768.0) == pytest.approx(1.87, abs=0.005)
    for k, x, tp in zip(ks, sigs, J.true_peak(sigs, IN)):
        close_db(true_peak(x, IN), want, 1e-12)
        close_db(tp, want, TP_TOL)


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 96000, 192000])
def test_seam_at_other_rates(hz):
    rng = np.random.default_rng(hz)
    h, b = tile_of(hz)
    N = b + h + 13
    sigs = [rng.standard_normal(N) * 2000.0, quarter_sine(N)] + [pair(N, k) for k in range(b - 7, b + 6)]
    got = J.true_peak(sigs, hz)
    peaks = J.loudness(sigs, hz)
    for x, tp, (_, P) in zip(sigs, got, peaks):
        close_db(tp, true_peak(x, hz), TP_TOL)
        assert tp >= P
    if factor(hz) == 1:
        assert got == [P for _, P in peaks]
    elif factor(hz) % 2 == 0:  # the half-sample phase exists: the pair's midpoint is reached
        assert got[2] == pytest.approx(20.0 * math.log10(PAIR * 10000.0 / 32768.0), abs=1e-4)


# ---- batches --------------------------------------------------------------------------------------------------------
def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, T, seed + T) for T in frames]


def test_batch_true_mode_holds_the_ceiling_sample_mode_does_not(eng):
    vi, utts = _utts(eng, (300, 900, 500), 500)
    C = -1.0
    over = []   # sample mode: each output's true peak over the ceiling
    for mode in (J.PEAK_TRUE, J.PEAK_SAMPLE):
        with J.Batch(vi, utts) as b:
            b.set_peak_mode(mode)           # before the target: either order
            b.set_loudness_target(0.0, C)   # far above what the voice reaches: the ceiling binds
            b.run()
            b.sync()
            for i in range(len(utts)):
                nat, out = b.pcm_native(i), b.pcm(i)
                L, P = integrated(nat, IN)
                tp = true_peak(nat, IN)
                rep = b.loudness_report(i)
                lufs, peak, gain = b.loudness(i)
                assert P == sample_peak(nat)
                close_db(lufs, L, 1e-8)
                close_db(peak, P, 1e-12)            # jb_batch_loudness still reports the sample peak
                assert (rep["lufs"], rep["sample_peak_dbfs"], rep["gain_db"]) == (lufs, peak, gain)
                assert rep["peak_mode"] == mode
                np.testing.assert_allclose(out, nat * 10.0 ** (gain / 20.0), rtol=1e-15, atol=0)
                if mode == J.PEAK_TRUE:
                    close_db(rep["true_peak_dbtp"], tp, TP_TOL)
                    assert rep["oversampling"] == 4
                    assert gain == pytest.approx(min(0.0 - L, C - tp), abs=1e-8)
                    assert abs(true_peak(out, IN) - C) <= 1e-9
                else:
                    assert math.isnan(rep["true_peak_dbtp"]) and rep["oversampling"] == 1
                    assert gain == pytest.approx(gain_db(L, P, 0.0, C), abs=1e-8)
                    assert abs(sample_peak(out) - C) <= 1e-9
                    # the sample-peak ceiling lets through what the input's true peak has over its sample peak
                    over.append(true_peak(out, IN) - C)
                    assert abs(over[-1] - (tp - P)) <= 1e-9
    # the mode matters: the sample-mode run of the same batch exceeds C in true peak (an utterance whose largest
    # sample is not overshot between the samples has TP = P and sits at C in both modes)
    assert max(over) > 1e-6


def test_modes_mixed_per_utterance(eng):
    vi, utts = _utts(eng, (300, 500, 700), 500)
    modes = [J.PEAK_TRUE, J.PEAK_SAMPLE, J.PEAK_TRUE]
    C = -2.0
    with J.Batch(vi, utts) as b:
        b.set_loudness_target([0.0, 0.0, -40.0], C)
        b.set_peak_mode(modes)
        b.run()
        b.sync()
        for i, mode in enumerate(modes):
            nat, out = b.pcm_native(i), b.pcm(i)
            L, P = integrated(nat, IN)
            rep = b.loudness_report(i)
            assert rep["peak_mode"] == mode
            if mode == J.PEAK_TRUE:
                tp = true_peak(nat, IN)
                close_db(rep["true_peak_dbtp"], tp, TP_TOL)
                assert rep["gain_db"] == pytest.approx(min([0.0, 0.0, -40.0][i] - L, C - tp), abs=1e-8)
            else:
                assert math.isnan(rep["true_peak_dbtp"])
                assert rep["gain_db"] == pytest.approx(C - P, abs=1e-8)
            np.testing.assert_allclose(out, nat * 10.0 ** (rep["gain_db"] / 20.0), rtol=1e-15, atol=0)
        # utterance 2: the target binds, not the ceiling
        assert b.loudness_report(2)["gain_db"] < C - true_peak(b.pcm_native(2), IN) - 1.0


# ---- chain interactions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hz", [8000, 16000])
def test_taken_at_the_output_rate(eng, out_hz):
    vi, utts = _utts(eng, (300, 900), 300)
    C = -1.0
    with J.Batch(vi, utts) as b:
        b.set_loudness_target(0.0, C)
        b.set_output_rate(out_hz)
        b.set_peak_mode(J.PEAK_TRUE)
        b.run()
        b.sync()
        for i in range(len(utts)):
            conv = J.resample(b.pcm_native(i), IN, out_hz)
            rep = b.loudness_report(i)
            tp = true_peak(conv, out_hz)
            close_db(rep["true_peak_dbtp"], tp, TP_TOL)
            assert rep["oversampling"] == factor(out_hz)
            assert rep["gain_db"] == pytest.approx(C - tp, abs=1e-8)
            out = b.pcm(i)
            np.testing.assert_allclose(out, conv * 10.0 ** (rep["gain_db"] / 20.0), rtol=1e-15, atol=0)
            assert abs(true_peak(out, out_hz) - C) <= 1e-9


def test_i16_sink_and_flac_on_top(eng):
    vi, utts = _utts(eng, (300, 900, 90), 900)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_loudness_target([-10.0, -30.0, 0.0], -0.5)
        b.set_peak_mode(J.PEAK_TRUE)
        b.set_flac()
        b.run()
        b.sync()
        streams = b.flac_all()
        for i in range(len(utts)):
            nat = b.pcm_native(i)
            rep = b.loudness_report(i)
            close_db(rep["true_peak_dbtp"], true_peak(nat, IN), TP_TOL)
            want = np.clip(nat * 10.0 ** (rep["gain_db"] / 20.0), -32768.0, 32767.0).astype(np.int16)
            same_bits(b.pcm_i16(i), want)
            got, info = decode(streams[i])
            same_bits(np.asarray(got, dtype=np.int16), want)
            assert info["rate"] == IN


def test_redo_rounds_report_the_final_pcm(eng):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12): redo rounds rewrite most chunks after run()
    measured them.  The report's TP must be that of the FINAL native PCM, and the output its normalization."""
    vi, utts = _utts(eng, (600, 1100), 40)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([0.0, -26.0], -3.0)
        b.set_peak_mode(J.PEAK_TRUE)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        for i, t in enumerate((0.0, -26.0)):
            nat = b.pcm_native(i)
            rep = b.loudness_report(i)
            L, P = integrated(nat, IN)
            tp = true_peak(nat, IN)
            close_db(rep["true_peak_dbtp"], tp, TP_TOL)
            close_db(rep["sample_peak_dbfs"], P, 1e-12)
            assert rep["gain_db"] == pytest.approx(min(t - L, -3.0 - tp), abs=1e-8)
            np.testing.assert_allclose(b.pcm(i), nat * 10.0 ** (rep["gain_db"] / 20.0), rtol=1e-15, atol=0)
        assert abs(true_peak(b.pcm(0), IN) + 3.0) <= 1e-9


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_loudness_target(0.0, -2.0)
            b.set_peak_mode(J.PEAK_TRUE)
            b.run()
            b.sync()
            res.append((b.pcm(pos), b.loudness_report(pos)))
    same_bits(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    assert res[0][1]["peak_mode"] == J.PEAK_TRUE and math.isfinite(res[0][1]["true_peak_dbtp"])


# ---- engine entries and the generator --------------------------------------------------------------------------------
def test_engine_entries(eng, native):
    C = -1.0
    et, es = with_mode(eng, -16.0, C), with_mode(eng, -16.0, C, J.PEAK_SAMPLE)
    tp0 = true_peak(native, IN)
    one = et.synthesize(SAMPLE_SENTENCE_1)
    assert abs(true_peak(one, IN) - C) <= 1e-9            # -16 LUFS is out of reach under the ceiling: it binds
    np.testing.assert_allclose(one, native * 10.0 ** ((C - tp0) / 20.0), rtol=1e-8, atol=0)
    assert true_peak(es.synthesize(SAMPLE_SENTENCE_1), IN) > C + 1e-9
    bat = et.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
    b16 = et.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], i16=True)
    for x, y in zip(bat, b16):
        assert true_peak(np.asarray(x), IN) <= C + 1e-9
        same_bits(np.asarray(y), np.clip(np.asarray(x), -32768.0, 32767.0).astype(np.int16))
    # each engine its own mode; the engine without a target leaves its utterance alone
    each = J.synthesize_batch_each([et, es, eng], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_1])
    assert abs(true_peak(np.asarray(each[0]), IN) - C) <= 1e-9
    assert abs(sample_peak(np.asarray(each[1])) - C) <= 1e-9
    assert true_peak(np.asarray(each[1]), IN) > C + 1e-9
    assert abs(true_peak(np.asarray(each[2]), IN) - tp0) <= 1e-6
    # the FLAC and the device-list entries
    got, _ = decode(et.synthesize_flac(SAMPLE_SENTENCE_1))
    (p16,) = et.synthesize_batch([SAMPLE_SENTENCE_1], i16=True)
    same_bits(np.asarray(got, dtype=np.int16), np.asarray(p16))
    ef = with_mode(eng, -16.0, C, fast_invariant=True)
    texts = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    for a, c in zip(ef.synthesize_batch(texts), ef.synthesize_batch(texts, devices=[0, 0])):
        same_bits(np.asarray(a), np.asarray(c))
        assert true_peak(np.asarray(a), IN) <= C + 1e-9


@pytest.mark.parametrize("out_hz", [0, 16000])
def test_generator_steps(eng, out_hz):
    e = with_mode(eng, -16.0, -3.0, out_hz=out_hz)
    want = e.synthesize(SAMPLE_SENTENCE_1)
    g = e.generator(SAMPLE_SENTENCE_1)
    buf, parts = np.zeros(g.fperiod()), []
    while True:
        n = g.generate_step(buf)
        if n == 0:
            break
        parts.append(buf[:n].copy())
    same_bits(np.concatenate(parts), want)
    assert abs(true_peak(want, out_hz or IN) + 3.0) <= 1e-9


# ---- rules and the default -------------------------------------------------------------------------------------------
def test_setter_rules(eng):
    vi, utts = _utts(eng, (300, 400), 5)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError):
            b.set_peak_mode([1, 1, 1])
        with pytest.raises(J.JbError):
            b.set_peak_mode([])
        with pytest.raises(J.JbError):
            b.set_peak_mode(2)
        with pytest.raises(J.JbError):
            b.set_peak_mode([0, 7])
        b.set_peak_mode([1, 0])
        with pytest.raises(J.JbError):
            b.loudness_report(0)        # no target: the mode alone measures nothing
        b.run()
        b.sync()
        plain = b.pcm_all()
        with pytest.raises(J.JbError):
            b.loudness_report(0)
        with pytest.raises(J.JbError):
            b.set_peak_mode(1)          # after the first run
    with J.Batch(vi, utts) as b:
        b.run()
        b.sync()
        for a, c in zip(plain, b.pcm_all()):
            same_bits(a, c)
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError):
            b.set_peak_mode(1)


def test_default_is_sample_mode(eng):
    vi, utts = _utts(eng, (700, 1300), 11)
    for i16 in (False, True):
        res = []
        for explicit in (False, True):
            with J.Batch(vi, utts, pcm_i16=i16) as b:
                b.set_loudness_target([-16.0, 0.0], -1.0)
                if explicit:
                    b.set_peak_mode(J.PEAK_SAMPLE)
                b.run()
                b.sync()
                res.append((b.pcm_all(), [b.loudness(i) for i in range(len(utts))],
                            [b.loudness_report(i) for i in range(len(utts))],
                            [b.pcm_native(i) for i in range(len(utts))]))
        for a, c in zip(res[0][0], res[1][0]):
            same_bits(a, c)
        assert res[0][1] == res[1][1]
        for (lufs, peak, gain), rep, nat, t in zip(res[0][1], res[0][2], res[0][3], (-16.0, 0.0)):
            assert rep["peak_mode"] == J.PEAK_SAMPLE and math.isnan(rep["true_peak_dbtp"])
            L, P = integrated(nat, IN)
            assert gain == pytest.approx(gain_db(L, P, t, -1.0), abs=1e-8)
