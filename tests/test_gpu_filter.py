"""The filter stage on the GPU (jb_filter.hip): the device seam against the long-double reference of
tests/filter_ref.py under its gate over the whole table of filters and lengths; then the stage in a batch -- bit for bit
the seam applied to the PCM in front of it, in f64 and through the 16-bit sink, behind the converter and in front of the
loudness measurement -- with the encoders and the join reading the filtered PCM; redo rounds; the fast invariant mode;
the engine entries."""
import hashlib
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import filter_ref as R
from tests import format_ref, join_ref
from tests.conftest import VOICE
from tests.flac_meta_ref import check as flac_check
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def quant(y):
    """The 16-bit sink's rule (fmt_quant): clamp, then truncate toward zero."""
    return np.trunc(np.clip(y, -32768.0, 32767.0)).astype(np.int16)


def cascade4():
    return J.highpass(70.0) + J.peaking(3000.0, 6.0, 2.0) + J.lowshelf(200.0, -6.0) + J.highshelf(8000.0, 4.0)


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
def test_seam_is_the_reference():
    """One launch with every filter at every length, and a zero-section utterance of every length among them: mixed
    section counts and the copy class run together."""
    pcms, filts, rates, which = [], [], [], []
    for i, (_, f, hz) in enumerate(R.filters()):
        for n in R.LENGTHS:
            pcms.append(R.signal_at(hz)[:n])
            filts.append(f)
            rates.append(hz)
            which.append(i)
    for n in R.LENGTHS:
        pcms.append(R.signal_at(48000)[:n])
        filts.append(None)
        rates.append(48000)
        which.append(None)
    got = J.filter_pcm(pcms, filts, rates)
    gate, worst = R.gate(), 0.0
    assert len(got) == len(pcms) == (len(R.filters()) + 1) * len(R.LENGTHS)
    for x, y, i in zip(pcms, got, which):
        assert y.dtype == np.float64 and y.size == x.size
        if i is None:
            assert y.tobytes() == x.tobytes()  # no section: the input, bit for bit
            continue
        err = R.error(y, i)
        worst = max(worst, err)
        assert err <= gate, (R.filters()[i][0], x.size, err, gate)
    print(f"floor {R.floor():.3e}  gate {gate:.3e}  device's largest error {worst:.3e}")
    # the 16-bit seam is the 16-bit sink's rule on the same y
    sel = [k for k, x in enumerate(pcms) if x.size in (17, 4097, 2 * 4096 + 3)]
    got16 = J.filter_pcm([pcms[k] for k in sel], [filts[k] for k in sel], [rates[k] for k in sel], i16=True)
    for k, y16 in zip(sel, got16):
        assert same(y16, quant(got[k])), k


# ---- 2. what a high-pass is for -------------------------------------------------------------------------------------
def test_removes_dc_and_keeps_a_passband_tone():
    from scipy import signal

    hz, f = 48000, J.highpass(70.0)
    t = np.arange(3 * hz, dtype=np.float64)
    x = 1000.0 + 8000.0 * np.sin(2.0 * np.pi * 1000.0 * t / hz)
    (y,) = J.filter_pcm([x], f, hz)
    rest = y[hz:]  # 2 s: whole periods of the tone
    assert abs(np.mean(rest)) < R.gate() * 1000.0
    _, h = signal.sosfreqz(J.filter_sos(f, hz), worN=[1000.0], fs=hz)
    ph = 2.0 * np.pi * 1000.0 * t[hz:] / hz
    amp = 2.0 * math.hypot(np.mean(rest * np.sin(ph)), np.mean(rest * np.cos(ph)))
    assert abs(amp / 8000.0 - abs(h[0])) < 1e-6


# ---- 3. the batch path ----------------------------------------------------------------------------------------------
FRAMES = (700, 2500, 1300)


@pytest.fixture(scope="module")
def batch_utts(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 3 + t) for t in FRAMES]


@pytest.fixture(scope="module")
def plain_pcm(batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.run()
        return [b.pcm(i) for i in range(len(utts))]


def batch_filters():
    return [J.highpass(70.0), None, cascade4()]


def test_batch_is_the_seam_bit_for_bit(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz, filts = vi.sampling_frequency, batch_filters()
    with J.Batch(vi, utts) as b:
        b.set_filter(filts)
        b.run()
        native = [b.pcm_native(i) for i in range(3)]
        want = J.filter_pcm(native, filts, hz)
        for i in range(3):
            assert same(native[i], plain_pcm[i])  # the native read stays the unfiltered vocoder PCM
            assert same(b.pcm(i), want[i]), i
            f = filts[i] if filts[i] is not None else J.no_filter()
            assert np.array_equal(b.filter_coefficients(i), J.filter_design(f, hz))
        assert same(b.pcm(1), native[1]) and not same(b.pcm(0), native[0])
        assert [x.tobytes() for x in b.pcm_all()] == [x.tobytes() for x in want]
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_filter(filts)
    # one filter for the whole batch; a request withdrawn, or without sections, is the batch of today
    with J.Batch(vi, utts) as b:
        b.set_filter(J.highpass(70.0))
        b.run()
        assert same(b.pcm(2), J.filter_pcm([plain_pcm[2]], J.highpass(70.0), hz)[0])
    for req in ("withdrawn", "empty"):
        with J.Batch(vi, utts) as b:
            b.set_filter(filts)
            b.set_filter(None if req == "withdrawn" else [None, J.no_filter(), None])
            b.run()
            assert all(same(b.pcm(i), plain_pcm[i]) for i in range(3))
            assert b.filter_coefficients(0).shape == (0, 5)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one filter, or one per utterance"):
            b.set_filter(filts[:2])
        with pytest.raises(J.JbError, match="utterance 1, section 0: q"):
            b.set_filter([None, J.highpass(70.0, 0.0), None])


def test_i16_is_the_quantised_f64(batch_utts):
    vi, utts = batch_utts
    filts = batch_filters()
    with J.Batch(vi, utts) as b:
        b.set_filter(filts)
        b.run()
        f64 = [b.pcm(i) for i in range(3)]
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_filter(filts)
        b.run()
        for i in range(3):
            assert same(b.pcm_i16(i), quant(f64[i])), i


def test_in_front_of_loudness_and_behind_the_converter(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz, filts = vi.sampling_frequency, batch_filters()
    filtered = J.filter_pcm(plain_pcm, filts, hz)
    with J.Batch(vi, utts) as b:
        b.set_filter(filts)
        b.set_loudness_target([-20.0, -26.0, -16.0], math.inf)
        b.run()
        for i, (L, _) in enumerate(J.loudness(filtered, hz)):
            lufs, _, gain = b.loudness(i)
            assert abs(lufs - L) <= 1e-8  # (the tolerance of tests/test_gpu_loudness.py for the same comparison)
            np.testing.assert_allclose(b.pcm(i), filtered[i] * 10.0 ** (gain / 20.0), rtol=1e-15, atol=0)
    # behind the converter: coefficients per rate, the filter over the converted PCM
    rates = [8000, 0, 16000]
    with J.Batch(vi, utts) as b:
        b.set_output_rate(rates)
        b.run()
        conv = [b.pcm(i) for i in range(3)]
    tel = J.telephone_band()
    for filts2 in ([tel, None, None], [tel, None, tel]):
        with J.Batch(vi, utts) as b:
            b.set_filter(filts2)
            b.set_output_rate(rates)
            assert np.array_equal(b.filter_coefficients(0), J.filter_design(tel, 8000))
            assert b.filter_coefficients(1).shape == (0, 5)
            if filts2[2] is not None:
                assert np.array_equal(b.filter_coefficients(2), J.filter_design(tel, 16000))
                assert not np.array_equal(b.filter_coefficients(2), b.filter_coefficients(0))
            # 3400 Hz is at or above half of 6000 Hz: the later rate request is refused and changes nothing
            with pytest.raises(J.JbError, match="utterance 0, section 1: f0_hz"):
                b.set_output_rate([6000, 0, 16000])
            with pytest.raises(J.JbError, match="utterance 0, section 1: f0_hz"):
                b.set_output_rate(6800)
            assert [b.output_rate(i) for i in range(3)] == [8000, hz, 16000]
            b.run()
            want = J.filter_pcm(conv, filts2, [8000, hz, 16000])
            for i in range(3):
                assert same(b.pcm(i), want[i]), i
    # the other order: the filter is checked against the rates already requested
    with J.Batch(vi, utts) as b:
        b.set_output_rate(6000)
        with pytest.raises(J.JbError, match="utterance 0, section 1: f0_hz"):
            b.set_filter(tel)


def test_encoders_see_the_filtered_pcm(batch_utts):
    vi, utts = batch_utts
    tel = J.telephone_band()
    with J.Batch(vi, utts) as b:
        b.set_output_rate(8000)
        b.set_filter(tel)
        b.set_format("ulaw")
        b.run()
        with J.Batch(vi, utts) as plain:
            plain.set_output_rate(8000)
            plain.run()
            conv = [plain.pcm(i) for i in range(3)]
        want = J.filter_pcm(conv, tel, 8000)
        for i in range(3):
            assert same(b.pcm(i), want[i])
            assert b.formatted(i) == format_ref.encode(b.pcm(i), "ulaw"), i
            assert b.formatted(i) != format_ref.encode(conv[i], "ulaw")
    filts = batch_filters()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_filter(filts)
        b.set_flac(md5=True)
        b.run()
        for i in range(3):
            x = b.pcm_i16(i)
            dec, _, meta = flac_check(b.flac(i))
            assert np.array_equal(dec, x) and meta["total"] == x.size
            assert meta["md5"] == hashlib.md5(np.ascontiguousarray(x, dtype="<i2").tobytes()).digest()
    req = [(0, 100, 3, 48, 48), (None, 1, 1, 0, 0), (0, 7, 2400, 48, 48)]
    for i16 in (False, True):
        with J.Batch(vi, utts, pcm_i16=i16) as b:
            b.set_filter(filts)
            b.set_join(req)
            b.run()
            pcms = [b.pcm_i16(i) if i16 else b.pcm(i) for i in range(3)]
            progs, _, _ = join_ref.join(pcms, req)
            assert b.num_outputs() == 2 and b.programme_layout(0)[0] == 2
            for p, w in enumerate(progs):
                assert same(b.programme_pcm(p), w.astype(np.int16 if i16 else np.float64)), p


# ---- 4. redo rounds -------------------------------------------------------------------------------------------------
def test_redo_rounds_filter_the_final_pcm(eng, tab):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12): redo rounds rewrite most chunks after run() has
    filtered the first PCM.  A recursive filter carries a changed sample to the utterance's end, so the touched
    utterances are filtered again whole: the output is the seam applied to the final native PCM, the samples in front
    of the first redone chunk included."""
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    utts = [synth.synth_utterance(tab, t, 40 + t) for t in (600, 1100)]
    filts = [cascade4(), J.highpass(20.0, 0.7071)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_filter(filts)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        native = [b.pcm_native(i) for i in range(2)]
        want = J.filter_pcm(native, filts, hz)
        for i in range(2):
            assert same(b.pcm(i), want[i]), i
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_filter(filts)
        b.set_loudness_target(-21.0, math.inf)
        b.set_loudness_groups([0, 0])
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        for i in range(2):
            assert same(b.pcm_native(i), native[i])
        L = J.loudness_groups(want, hz, group=[0, 0])["groups"][0]["lufs"]  # of the filtered members, on the seam
        gains = [b.loudness(i)[2] for i in range(2)]
        assert gains[0] == gains[1] and abs(b.loudness_group(0)["lufs"] - L) <= 1e-8
        for i in range(2):
            np.testing.assert_allclose(b.pcm(i), want[i] * 10.0 ** (gains[i] / 20.0), rtol=1e-15, atol=0)


# ---- 5. invariance --------------------------------------------------------------------------------------------------
def test_invariance_alone_and_among_64(eng, tab):
    vi = eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    pf = cascade4()
    of = [[J.highpass(30.0 + k), J.telephone_band(), None, J.notch(50.0 + k, 30.0) + J.lowpass(9000.0)][k % 4]
          for k in range(63)]
    res = []
    for utts, filts, pos in (([probe], [pf], 0), (others[:20] + [probe] + others[20:], of[:20] + [pf] + of[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_filter(filts)
            b.run()
            res.append(b.pcm(pos).tobytes())
    assert res[0] == res[1] and len(res[0]) == 8 * 900 * vi.fperiod


# ---- 6. the engine entries ------------------------------------------------------------------------------------------
def test_engine_entries(eng):
    hz = eng._out_hz()
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    plain = [np.array(x) for x in eng.synthesize_batch(sents)]
    plain16 = [np.array(x) for x in eng.synthesize_batch(sents, i16=True)]
    plain_flac, _ = eng.synthesize_programme(sents, sink="flac", md5=True, gap_ms=100.0)
    plain_gen = eng.generator(SAMPLE_SENTENCE_1).generate_all()
    hp, tel = J.highpass(70.0), J.telephone_band()
    ef = eng.clone()
    ef.set_filter(hp)
    assert ef.get_filter().n_sections == 1 and eng.get_filter().n_sections == 0
    assert ef.clone().get_filter().section[0].f0_hz == 70.0  # copied with the Condition
    want = J.filter_pcm(plain, hp, hz)
    assert same(ef.synthesize(SAMPLE_SENTENCE_1), want[0])
    got = ef.synthesize_batch(sents)
    assert all(same(np.array(g), w) for g, w in zip(got, want))
    got16 = ef.synthesize_batch(sents, i16=True)
    assert all(same(np.array(g), quant(w)) for g, w in zip(got16, want))
    # _each: one filter per utterance
    et = eng.clone()
    et.set_filter(tel)
    each = J.synthesize_batch_each([ef, et], sents)
    assert same(np.array(each[0]), want[0]) and same(np.array(each[1]), J.filter_pcm([plain[1]], tel, hz)[0])
    each = J.synthesize_batch_each([eng, et], sents)
    assert same(np.array(each[0]), plain[0]) and same(np.array(each[1]), J.filter_pcm([plain[1]], tel, hz)[0])
    # a programme as FLAC: the join of the filtered 16-bit members
    stream, starts = ef.synthesize_programme(sents, sink="flac", md5=True, gap_ms=100.0)
    parts = [quant(w) for w in want]
    (prog,), _, want_starts = join_ref.join(parts, join_ref.chapter([x.size for x in parts], hz, gap_ms=100.0))
    dec, _, meta = flac_check(stream)
    assert np.array_equal(dec, prog) and starts == want_starts
    assert meta["md5"] == hashlib.md5(np.ascontiguousarray(prog, dtype="<i2").tobytes()).digest()
    # the generator
    assert same(ef.generator(SAMPLE_SENTENCE_1).generate_all(), want[0])
    # behind the engine's output rate: designed at that rate, refused where f0 does not fit under it
    e8 = eng.clone()
    e8.condition.set_output_sampling_frequency(8000)
    conv = e8.synthesize(SAMPLE_SENTENCE_1)
    e8.set_filter(tel)
    assert same(e8.synthesize(SAMPLE_SENTENCE_1), J.filter_pcm([conv], tel, 8000)[0])
    with pytest.raises(J.JbError, match="f0_hz"):
        e8.set_filter(J.lowpass(4000.0))
    e8.condition.set_output_sampling_frequency(6000)
    with pytest.raises(J.JbError, match="utterance 0, section 1: f0_hz"):
        e8.synthesize(SAMPLE_SENTENCE_1)
    # without a filter (never set, or set and withdrawn) every entry returns today's bytes
    ef.set_filter(None)
    for e in (eng, ef):
        assert all(same(np.array(g), w) for g, w in zip(e.synthesize_batch(sents), plain))
        assert all(same(np.array(g), w) for g, w in zip(e.synthesize_batch(sents, i16=True), plain16))
        assert same(e.synthesize(SAMPLE_SENTENCE_1), plain[0])
        assert e.synthesize_programme(sents, sink="flac", md5=True, gap_ms=100.0)[0] == plain_flac
        assert same(e.generator(SAMPLE_SENTENCE_1).generate_all(), plain_gen)
