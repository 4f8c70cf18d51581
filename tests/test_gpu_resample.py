"""Output-rate conversion on the GPU (k_resample): the converter on PCM the test holds (impulses, sines, random
signals against a numpy polyphase over the library's own taps), then every entry that honours an output rate --
jb_synthesize, the 16-bit sink, redo rounds, mixed rates in one batch, the generator, _multi -- and the native rate."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import PCM_TOL, rel_rms

pytestmark = pytest.mark.gpu

IN = 48000
RATES = [8000, 16000, 22050, 24000, 44100]


def polyphase(x, L, M, taps):
    """y[k] = sum_j h[p][j] x[q - C + 1 + j], x = 0 outside [0, N): numpy, the library's taps."""
    x = np.asarray(x, dtype=np.float64)
    ntaps = taps.shape[1]
    C = ntaps // 2
    n_out = -(-x.size * L // M)
    k = np.arange(n_out, dtype=np.int64)
    q, p = (k * M) // L, (k * M) % L
    xp = np.concatenate([np.zeros(C), x, np.zeros(ntaps + 1)])
    idx = (q - C + 1 + C)[:, None] + np.arange(ntaps)[None, :]
    return np.einsum("kj,kj->k", taps[p], xp[idx])


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


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


def with_rate(eng, hz, fast_invariant=False):
    e = eng.clone()
    e.condition.set_output_sampling_frequency(hz)
    e.condition.set_fast_invariant(fast_invariant)
    return e


# ---- the converter alone (jb_resample_pcm_batch) ---------------------------------------------------------------------
@pytest.mark.parametrize("out_hz", [16000, 22050, 44100, 96000])
def test_impulses_give_the_taps(out_hz):
    """An impulse at sample 0, at N-1 and in the middle: every output is one tap times 1.0, so the taps come back bit
    for bit -- the phase and window indexing and both edges."""
    L, M, taps = J.resample_filter(IN, out_hz)
    ntaps = taps.shape[1]
    C = ntaps // 2
    N = 4000
    xs = []
    for n0 in (0, N // 2 + 7, N - 1):
        x = np.zeros(N)
        x[n0] = 1.0
        xs.append(x)
    ys = J.resample(xs, IN, out_hz)
    for n0, y in zip((0, N // 2 + 7, N - 1), ys):
        n_out = -(-N * L // M)
        assert y.shape == (n_out,)
        k = np.arange(n_out, dtype=np.int64)
        q, p = (k * M) // L, (k * M) % L
        j = n0 - q + C - 1
        hit = (j >= 0) & (j < ntaps)
        want = np.zeros(n_out)
        want[hit] = taps[p[hit], j[hit]]
        assert hit.sum() > 0
        assert np.array_equal(y, want), (out_hz, n0, np.flatnonzero(y != want)[:5])
        assert y[hit].tobytes() == want[hit].tobytes()


def _amplitude(y, f, fs):
    n = np.arange(y.size)
    A = np.stack([np.sin(2 * np.pi * f * n / fs), np.cos(2 * np.pi * f * n / fs)], axis=1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    return float(np.hypot(*c))


@pytest.mark.parametrize("out_hz", RATES)
def test_sines(out_hz):
    """Passband (up to 0.8 of the output Nyquist): amplitude within 0.001 dB.  Above the output Nyquist: <= -95 dB."""
    N = 24000
    n = np.arange(N)
    nyq = out_hz / 2
    pas = [0.05 * nyq, 0.37 * nyq, 0.8 * nyq]
    stop = list(np.linspace(1.02 * nyq, 0.98 * IN / 2, 3))  # (below the input's Nyquist: a sine above it would alias)
    xs = [np.sin(2 * np.pi * f * n / IN + 0.3) for f in pas + stop]
    ys = J.resample(xs, IN, out_hz)
    edge = 400  # outputs whose filter reaches past either end of the input
    for f, y in zip(pas, ys[:3]):
        a = _amplitude(y[edge:-edge], f, out_hz)
        assert abs(20 * np.log10(a)) <= 0.001, (out_hz, f, a)
    for f, y in zip(stop, ys[3:]):
        r = np.sqrt(np.mean(y[edge:-edge] ** 2)) * np.sqrt(2)
        assert 20 * np.log10(r) <= -95.0, (out_hz, f, r)


@pytest.mark.parametrize("out_hz", RATES + [96000])
def test_random_signals(out_hz):
    """Lengths 0, 1, 2, ntaps - 1 and long in one call: 1e-13 relative RMS of a numpy polyphase."""
    L, M, taps = J.resample_filter(IN, out_hz)
    rng = np.random.default_rng(out_hz)
    lens = [0, 1, 2, taps.shape[1] - 1, 50021]
    xs = [rng.standard_normal(n) * 3000.0 for n in lens]
    ys = J.resample(xs, IN, out_hz)
    for x, y in zip(xs, ys):
        want = polyphase(x, L, M, taps)
        assert y.shape == want.shape == (-(-x.size * L // M),)
        if x.size:
            assert rel_rms(y, want) <= 1e-13, (out_hz, x.size, rel_rms(y, want))


# ---- the engine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hz", RATES)
def test_synthesize_at_rate(eng, native, oracle_pcm, out_hz):
    L, M, taps = J.resample_filter(IN, out_hz)
    got = with_rate(eng, out_hz).synthesize(SAMPLE_SENTENCE_1)
    assert native.size == 66480
    assert got.size == -(-66480 * L // M)
    if out_hz == 16000:
        assert got.size == 22160
    if out_hz == 22050:
        assert got.size == 30540
    assert rel_rms(got, J.resample(native, IN, out_hz)) <= 1e-13
    assert rel_rms(got, polyphase(oracle_pcm, L, M, taps)) <= PCM_TOL


def test_native_rate_is_unchanged(eng, native):
    same_bits(with_rate(eng, IN).synthesize(SAMPLE_SENTENCE_1), native)
    same_bits(with_rate(eng, 0).synthesize(SAMPLE_SENTENCE_1), native)


@pytest.mark.parametrize("out_hz", [16000, 22050])
def test_i16_is_the_converted_f64_clamped(eng, out_hz):
    """The 16-bit sink with a rate: clamp-and-truncate of the f64 conversion of the batch's own native PCM, byte for
    byte; the engine's i16 entry agrees with its f64 entry the same way."""
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 900 + T) for T in (700, 2500, 1300)]
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_output_rate(out_hz)
        b.run()
        b.sync()
        allv = b.pcm_all()
        for i in range(len(utts)):
            nat = b.pcm_native(i)
            assert nat.size == b.num_frames(i) * vi.fperiod
            want = np.clip(J.resample(nat, IN, out_hz), -32768.0, 32767.0).astype(np.int16)
            got = b.pcm_i16(i)
            same_bits(got, want)
            same_bits(allv[i], want)
            assert b.output_rate(i) == out_hz
    e = with_rate(eng, out_hz)
    f64, = e.synthesize_batch([SAMPLE_SENTENCE_2])
    i16, = e.synthesize_batch([SAMPLE_SENTENCE_2], i16=True)
    same_bits(np.asarray(i16), np.clip(np.asarray(f64), -32768.0, 32767.0).astype(np.int16))


def test_redo_rounds_convert_the_final_pcm(eng):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12): redo rounds rewrite most chunks after run()
    converted them.  The output must be the conversion of the FINAL native PCM."""
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (600, 1100)]
    for rate in (16000, [22050, 24000]):
        with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
            b.set_output_rate(rate)
            b.run()
            b.sync()
            assert b.info()["n_redo"] >= 4
            for i in range(len(utts)):
                hz = b.output_rate(i)
                assert hz == (rate if np.isscalar(rate) else rate[i])
                got, want = b.pcm(i), J.resample(b.pcm_native(i), IN, hz)
                assert got.size == want.size
                assert rel_rms(got, want) <= 1e-13, (rate, i, rel_rms(got, want))


def test_mixed_rates_fast_invariant(eng):
    """jb_synthesize_batch_each with engines at native, 16, 22.05 and 24 kHz (the output rate is not among the fields
    the engines must agree on): in the fast invariant mode every utterance has the bits of its engine's jb_synthesize
    alone, and of the same utterance inside another batch."""
    rates = [0, 16000, 22050, 24000]
    engines = [with_rate(eng, r, fast_invariant=True) for r in rates]
    texts = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    batch = J.synthesize_batch_each(engines, texts)
    other = J.synthesize_batch_each(engines[::-1] + engines[1:2], texts[::-1] + texts[1:2])
    for u, (e, t) in enumerate(zip(engines, texts)):
        alone = e.synthesize(t)
        same_bits(np.asarray(batch[u]), alone)
        same_bits(np.asarray(other[len(rates) - 1 - u]), alone)
    same_bits(np.asarray(other[-1]), np.asarray(batch[1]))
    assert np.asarray(batch[0]).size == 66480 and np.asarray(batch[3]).size == 33240


@pytest.mark.parametrize("out_hz", [22050, 24000, 96000, 11025, 400])
def test_generator_steps(eng, out_hz):
    """96 kHz: an upsampling step of 2 F; 11.025 kHz: a 1-wave padded table, steps of 55 and 56; 400 Hz: the
    global-memory path, two samples per frame."""
    L, M, _ = J.resample_filter(IN, out_hz)
    e = with_rate(eng, out_hz)
    want = e.synthesize(SAMPLE_SENTENCE_1)
    g = e.generator(SAMPLE_SENTENCE_1)
    F = g.fperiod()
    step_max = -(-F * L // M)
    with pytest.raises(J.JbError) as ei:
        g.generate_step(np.zeros(step_max - 1))
    assert ei.value.code == -8
    buf, parts, k = np.zeros(step_max), [], 0
    while True:
        n = g.generate_step(buf)
        if n == 0:
            break
        assert n == -(-(k + 1) * F * L // M) - (-(-k * F * L // M)), (k, n)
        parts.append(buf[:n].copy())
        k += 1
    assert k == g.total_frames()
    if out_hz == 22050:
        assert {p.size for p in parts} == {110, 111}
    if out_hz in (96000, 11025, 400):
        assert {p.size for p in parts} == {96000: {2 * F}, 11025: {55, 56}, 400: {2}}[out_hz]
    same_bits(np.concatenate(parts), want)
    # steps of several frames at once: the same samples
    g2 = e.generator(SAMPLE_SENTENCE_1)
    big = np.zeros(want.size + step_max)
    pos = 0
    while True:
        n = g2.generate_steps(big[pos:], 97)
        if n == 0:
            break
        pos += n
    same_bits(big[:pos], want)


def test_multi_device_list(eng):
    """_multi over {0, 0} with a rate: the single-device result (fast invariant mode: the same bits whatever the
    split)."""
    e = with_rate(eng, 16000, fast_invariant=True)
    one = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1])
    two = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1], devices=[0, 0])
    for a, b in zip(one, two):
        same_bits(np.asarray(a), np.asarray(b))
    assert np.asarray(one[0]).size == 22160


@pytest.mark.parametrize("pcm_i16", [False, True])
def test_native_utterances_in_a_converting_batch(eng, pcm_i16):
    """Native utterances of a batch that converts others are copied (identity table, tiles of 16,384 samples): the
    values of the vocoder's own PCM, or its clamp-and-truncate, whatever else the batch holds."""
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 70 + T) for T in (700, 1500, 90)]
    with J.Batch(vi, utts, pcm_i16=pcm_i16) as b:
        b.set_output_rate([0, 16000, IN])
        b.run()
        b.sync()
        allv = b.pcm_all()
        for i in (0, 2):
            nat = b.pcm_native(i)
            assert b.output_rate(i) == IN and b.num_samples(i) == nat.size
            want = np.clip(nat, -32768.0, 32767.0).astype(np.int16) if pcm_i16 else nat
            got = b.pcm_i16(i) if pcm_i16 else b.pcm(i)
            same_bits(got, want)
            same_bits(allv[i], want)
        conv = J.resample(b.pcm_native(1), IN, 16000)
        if pcm_i16:
            same_bits(allv[1], np.clip(conv, -32768.0, 32767.0).astype(np.int16))
        else:
            same_bits(allv[1], conv)
