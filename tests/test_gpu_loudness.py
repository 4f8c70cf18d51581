"""Loudness normalization on the GPU (jb_loudness.hip): the measurement on PCM the test holds against a numpy
evaluation of the definition, then every entry that honours a target -- batches with per-utterance targets, the
ceiling, the 16-bit sink, output rates, redo rounds, the fast invariant mode, the engine entries and the generator."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import PCM_TOL, rel_rms
from tests.loudness_ref import gain_db, integrated

pytestmark = pytest.mark.gpu

IN = 48000
H = 4800


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def close_lu(got, want, tol):
    if math.isinf(want):
        assert got == want, (got, want)
    else:
        assert abs(got - want) <= tol, (got, want)


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def native(eng):
    return eng.synthesize(SAMPLE_SENTENCE_1)


@pytest.fixture(scope="module")
def oracle_pcm():
    return O.Voice(VOICE).synthesize(SAMPLE_SENTENCE_1)


def with_target(eng, target, ceiling=None, fast_invariant=False, out_hz=0):
    e = eng.clone()
    e.condition.set_loudness_target(target)
    if ceiling is not None:
        e.condition.set_peak_ceiling(ceiling)
    e.condition.set_fast_invariant(fast_invariant)
    e.condition.set_output_sampling_frequency(out_hz)
    return e


# ---- the measurement alone (jb_loudness_pcm_batch) -------------------------------------------------------------------
def test_seam_against_numpy(oracle_pcm):
    rng = np.random.default_rng(7)
    n = np.arange(10 * IN)
    sine = 32768.0 * np.sin(2 * np.pi * 997 * n / IN)
    sigs = [sine]
    for N in (4 * H - 1, 4 * H, 4 * H + 1, 7 * H - 1, 7 * H + 1, 23 * H, 23 * H + 1):
        sigs.append(rng.standard_normal(N) * 3000.0)
    sigs.append(np.zeros(9 * H))                               # silence
    sigs.append(rng.standard_normal(9 * H) * 0.02)             # under -70 LUFS
    loud = rng.standard_normal(12 * H) * 8000.0
    sigs.append(np.concatenate([loud, loud[: 30 * H // 3] * 0.01, loud[:6 * H] * 0.01]))  # 40 dB quieter tail
    sigs.append(np.asarray(oracle_pcm, dtype=np.float64))
    sigs.append(np.zeros(0))
    got = J.loudness(sigs, IN)
    for i, (x, (L, P)) in enumerate(zip(sigs, got)):
        wL, wP = integrated(x, IN)
        close_lu(L, wL, 1e-8)
        close_lu(P, wP, 1e-12)
    assert abs(got[0][0] + 3.01) <= 0.01 and got[0][1] == 0.0
    assert got[8][0] == -math.inf and got[8][1] == -math.inf
    assert got[9][0] == -math.inf
    # the relative gate drops the quiet part: near the loud part's loudness (the blocks across the step stay), where the
    # absolute gate alone would give about 3.8 LU less
    assert integrated(loud, IN)[0] - 1.0 < got[10][0] < integrated(loud, IN)[0]
    assert abs(got[11][0] + 27.14) < 0.01 and abs(got[11][1] + 9.30) < 0.01
    assert got[12] == (-math.inf, -math.inf)


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 96000])
def test_seam_at_other_rates(hz):
    rng = np.random.default_rng(hz)
    h = (hz + 5) // 10
    sigs = [rng.standard_normal(N) * 2000.0 for N in (4 * h - 1, 4 * h + 1, 9 * h + 17, 5 * hz)]
    n = np.arange(3 * hz)
    sigs.append(32768.0 * np.sin(2 * np.pi * 997 * n / hz))
    for x, (L, P) in zip(sigs, J.loudness(sigs, hz)):
        wL, wP = integrated(x, hz)
        close_lu(L, wL, 1e-8)
        close_lu(P, wP, 1e-12)


# ---- batches --------------------------------------------------------------------------------------------------------
def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, T, seed + T) for T in frames]


def test_batch_per_utterance_targets(eng):
    vi, utts = _utts(eng, (700, 2500, 1300), 500)
    targets = [-16.0, -23.0, math.nan]
    with J.Batch(vi, utts) as b:
        b.set_loudness_target(targets, math.inf)
        b.run()
        b.sync()
        allv = b.pcm_all()
        for i, t in enumerate(targets):
            nat = b.pcm_native(i)
            lufs, peak, gain = b.loudness(i)
            wL, wP = integrated(nat, IN)
            close_lu(lufs, wL, 1e-8)
            close_lu(peak, wP, 1e-12)
            assert gain == pytest.approx(gain_db(wL, wP, t, math.inf), abs=1e-8)
            out = b.pcm(i)
            want = nat * 10.0 ** (gain / 20.0)
            np.testing.assert_allclose(out, want, rtol=1e-15, atol=0)
            same_bits(allv[i], out)
            if math.isnan(t):
                assert gain == 0.0
                same_bits(out, nat)
            else:
                close_lu(integrated(out, IN)[0], t, 1e-6)


def test_ceiling_binds(eng, native):
    e = with_target(eng, -16.0, -1.0)
    out = e.synthesize(SAMPLE_SENTENCE_1)
    L0, P0 = integrated(native, IN)
    assert abs(P0 + 9.30) < 0.01
    g = out[np.argmax(np.abs(native))] / native[np.argmax(np.abs(native))]
    assert abs(20 * math.log10(g) - (-1.0 - P0)) < 1e-9
    L1, P1 = integrated(out, IN)
    assert abs(P1 + 1.0) <= 1e-9
    assert L1 < -16.0


def test_i16_is_the_gained_f64_clamped(eng):
    vi, utts = _utts(eng, (700, 2500, 90), 900)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_loudness_target([-10.0, -30.0, -14.0], -0.5)
        b.run()
        b.sync()
        allv = b.pcm_all()
        for i in range(len(utts)):
            nat = b.pcm_native(i)
            _, _, gain = b.loudness(i)
            want = np.clip(nat * 10.0 ** (gain / 20.0), -32768.0, 32767.0).astype(np.int16)
            same_bits(b.pcm_i16(i), want)
            same_bits(allv[i], want)
    # the engine's 16-bit entry is the clamp and truncation of its f64 entry
    e = with_target(eng, -12.0, math.inf)
    f64, = e.synthesize_batch([SAMPLE_SENTENCE_2])
    i16, = e.synthesize_batch([SAMPLE_SENTENCE_2], i16=True)
    same_bits(np.asarray(i16), np.clip(np.asarray(f64), -32768.0, 32767.0).astype(np.int16))


@pytest.mark.parametrize("out_hz", [16000, 22050])
def test_measured_at_the_output_rate(eng, out_hz):
    vi, utts = _utts(eng, (700, 1900), 300)
    with J.Batch(vi, utts) as b:
        b.set_loudness_target(math.nan, math.inf)
        b.set_output_rate(out_hz)
        b.run()
        b.sync()
        for i in range(len(utts)):
            conv = b.pcm(i)
            same_bits(conv, J.resample(b.pcm_native(i), IN, out_hz))
            lufs, peak, gain = b.loudness(i)
            wL, wP = integrated(conv, out_hz)
            close_lu(lufs, wL, 1e-8)
            close_lu(peak, wP, 1e-12)
            assert gain == 0.0
    # a target on a 16-bit batch with a rate, the rate set first
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_output_rate(out_hz)
        b.set_loudness_target(-18.0, math.inf)
        b.run()
        b.sync()
        for i in range(len(utts)):
            conv = J.resample(b.pcm_native(i), IN, out_hz)
            lufs, _, gain = b.loudness(i)
            close_lu(lufs, integrated(conv, out_hz)[0], 1e-8)
            want = np.clip(conv * 10.0 ** (gain / 20.0), -32768.0, 32767.0).astype(np.int16)
            same_bits(b.pcm_i16(i), want)


def test_redo_rounds_normalize_the_final_pcm(eng):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12): redo rounds rewrite most chunks after run()
    measured them.  The output must be the normalization of the FINAL native PCM."""
    vi, utts = _utts(eng, (600, 1100), 40)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], math.inf)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        for i, t in enumerate((-20.0, -26.0)):
            nat = b.pcm_native(i)
            lufs, _, gain = b.loudness(i)
            close_lu(lufs, integrated(nat, IN)[0], 1e-8)
            np.testing.assert_allclose(b.pcm(i), nat * 10.0 ** (gain / 20.0), rtol=1e-15, atol=0)
            close_lu(integrated(b.pcm(i), IN)[0], t, 1e-6)


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_loudness_target(-19.0, -2.0)
            b.run()
            b.sync()
            res.append((b.pcm(pos), b.loudness(pos)))
    same_bits(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]


# ---- engine entries -------------------------------------------------------------------------------------------------
def test_engine_entries_each_engine_its_target(eng, native):
    e1, e2 = with_target(eng, -16.0, math.inf), with_target(eng, -28.0, math.inf)
    n2 = eng.synthesize(SAMPLE_SENTENCE_2)
    for e, t in ((e1, -16.0), (e2, -28.0)):
        one = e.synthesize(SAMPLE_SENTENCE_1)
        close_lu(integrated(one, IN)[0], t, 1e-6)
        g = 10.0 ** ((t - integrated(native, IN)[0]) / 20.0)
        np.testing.assert_allclose(one, native * g, rtol=1e-8, atol=0)
        bat = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
        for x in bat:
            close_lu(integrated(np.asarray(x), IN)[0], t, 1e-6)
        b16 = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], i16=True)
        for x, y in zip(bat, b16):
            same_bits(np.asarray(y), np.clip(np.asarray(x), -32768.0, 32767.0).astype(np.int16))
    each = J.synthesize_batch_each([e1, e2, eng], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_2])
    close_lu(integrated(np.asarray(each[0]), IN)[0], -16.0, 1e-6)
    close_lu(integrated(np.asarray(each[1]), IN)[0], -28.0, 1e-6)
    # the engine without a target: its utterance as it is
    assert rel_rms(np.asarray(each[2]), n2) <= PCM_TOL


def test_multi_device_list(eng):
    e = with_target(eng, -20.0, -1.0, fast_invariant=True)
    texts = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    one = e.synthesize_batch(texts)
    two = e.synthesize_batch(texts, devices=[0, 0])
    for a, b in zip(one, two):
        same_bits(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("out_hz", [0, 22050])
def test_generator_steps(eng, out_hz):
    e = with_target(eng, -21.0, -3.0, out_hz=out_hz)
    want = e.synthesize(SAMPLE_SENTENCE_1)
    g = e.generator(SAMPLE_SENTENCE_1)
    F = g.fperiod()
    buf, parts = np.zeros(F), []
    while True:
        n = g.generate_step(buf)
        if n == 0:
            break
        parts.append(buf[:n].copy())
    same_bits(np.concatenate(parts), want)
    L, P = integrated(want, out_hz or IN)
    assert L <= -21.0 + 1e-6 and P <= -3.0 + 1e-9


def test_off_means_unchanged(eng, native):
    vi, utts = _utts(eng, (700, 1300), 11)
    for i16 in (False, True):
        outs = []
        for set_it in (False, True):
            with J.Batch(vi, utts, pcm_i16=i16) as b:
                if set_it:
                    b.set_loudness_target(math.nan, math.inf)
                b.run()
                b.sync()
                outs.append(b.pcm_all())
        for a, c in zip(*outs):
            same_bits(a, c)
    e = with_target(eng, math.nan, -1.0)
    same_bits(e.synthesize(SAMPLE_SENTENCE_1), native)


def test_setter_rules(eng):
    vi, utts = _utts(eng, (300, 400), 5)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError):
            b.set_loudness_target([-16.0, -16.0, -16.0])
        with pytest.raises(J.JbError):
            b.loudness(0)
        b.set_loudness_target(-16.0)
        b.run()
        b.sync()
        with pytest.raises(J.JbError):
            b.set_loudness_target(-20.0)
