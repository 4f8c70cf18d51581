"""Round 4 boundary additions (VERDICT r3 "next" 6):

  jb_generator_new_from_tracks   SpeechGenerator::new + generate_step on caller-held tracks   src/speech.rs:25-82
  jb_vocoder_synthesize_batch    Vocoder::new + Vocoder::synthesize per frame                 src/vocoder/mod.rs:45-178
      -- the one way to nlpf == 0, Excitation::get without a ring buffer                      src/vocoder/excitation.rs:87-100
  the streaming generator serves no frame of an utterance whose resident GV kernel timed out in formation
"""
import os

import numpy as np
import pytest

import jbonsai_amd as J
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import BENCH_LETTER, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import assert_pcm_close, rel_rms, voice_info

pytestmark = pytest.mark.gpu
NODATA = -1e10


@pytest.fixture(scope="module")
def vi(oracle_voice):
    assert J.lib().jb_device_count() > 0
    return voice_info(oracle_voice)


def oracle_tracks(v, labels):
    r = v.synthesize(labels, want_tracks=True)
    return J.TrackUtterance(r["mcp"], r["lf0"], r["lpf"]), r["pcm"]


def test_generator_from_tracks_streams_the_oracles_audio(oracle_voice, vi):
    tu, ref = oracle_tracks(oracle_voice, SAMPLE_SENTENCE_2)
    g = J.generator_from_tracks(vi, tu)
    fp = g.fperiod()
    assert fp == 240 and g.total_frames() == len(tu.lf0) and g.synthesized_frames() == 0
    out = np.zeros(len(ref))
    buf = np.zeros(fp)
    n = 0
    for _ in range(13):  # single steps: the first ones come from the serial recursion
        assert g.generate_step(buf) == fp
        out[n * fp:(n + 1) * fp] = buf
        n += 1
    assert g.synthesized_frames() == 13
    big = np.zeros(50 * fp)
    got = g.generate_steps(big, 50)
    assert got == 50 * fp
    out[n * fp:(n + 50) * fp] = big
    n += 50
    rest = g.generate_all()
    out[n * fp:] = rest
    assert g.generate_step(buf) == 0 and g.synthesized_frames() == g.total_frames()
    assert_pcm_close(out, ref, 240)
    with pytest.raises(J.JbError):  # "The length of speech buffer must be larger than fperiod."
        J.generator_from_tracks(vi, tu).generate_step(np.zeros(fp - 1))
    g.close()


def test_generator_from_tracks_mirrors_the_reference_panics(oracle_voice, vi):
    tu, _ = oracle_tracks(oracle_voice, SAMPLE_SENTENCE_1)
    T = len(tu.lf0)
    for u, msg in [
        (J.TrackUtterance(tu.spectrum[:-1], tu.lf0, tu.lpf), "The length of spectrum, lf0, and lpf must be the same."),
        (J.TrackUtterance(tu.spectrum, np.zeros((T, 2)), tu.lpf), "The size of lf0 static vector must be 1."),
        (J.TrackUtterance(tu.spectrum, tu.lf0, np.zeros((T, 30))),
         "The number of low-pass filter coefficient must be odd numbers."),
    ]:
        with pytest.raises(J.JbError) as ei:
            J.generator_from_tracks(vi, u)
        assert ei.value.code == -1 and msg in str(ei.value)
    g = J.generator_from_tracks(vi, J.TrackUtterance(np.zeros((0, 35)), np.zeros((0, 1)), np.zeros((0, 31))))
    assert g.total_frames() == 0 and g.generate_step(np.zeros(240)) == 0  # empty tracks: nothing to do, no panic


def _no_lpf_voice(vi):
    streams = list(vi.streams)
    streams[2] = J.StreamInfo(0, False, False, [[1.0]])
    return J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha, streams)


def test_vocoder_level_entry_without_ring_buffer(oracle_voice, vi):
    """nlpf == 0: voiced samples are the bare pulse, the noise stream is drawn on unvoiced samples only and there
    is no delay (excitation.rs:87-100) -- against the oracle's restatement of that branch, for the voice's own
    voicing and for patterns that shift the noise stream's position."""
    v0 = _no_lpf_voice(vi)
    tu, _ = oracle_tracks(oracle_voice, SAMPLE_SENTENCE_2)
    T = len(tu.lf0)
    base = np.where(tu.lf0[:, 0] == NODATA, 5.0, tu.lf0[:, 0])
    pats = {
        "as the voice": tu.lf0[:, 0],
        "all unvoiced": np.full(T, NODATA),
        "all voiced": base,
        "runs of 7/3": np.where(np.arange(T) % 10 < 7, base, NODATA),
        "first frame voiced only": np.where(np.arange(T) < 1, base, NODATA),
    }
    utts = [J.TrackUtterance(tu.spectrum, lf0, np.zeros((T, 0))) for lf0 in pats.values()]
    got = J.vocoder_synthesize_batch(v0, utts)
    for (name, lf0), g in zip(pats.items(), got):
        ref = O.vocoder(vi.sampling_frequency, vi.fperiod, vi.alpha, 1.0, lf0, tu.spectrum, None)
        assert_pcm_close(g, ref, 240, what=name)
    # with a ring buffer the same entry equals the SpeechGenerator one
    a = J.vocoder_synthesize_batch(vi, [tu])[0]
    b = J.vocode_tracks_batch(vi, [tu])[0]
    assert np.array_equal(a, b)
    # SpeechGenerator::new refuses nlpf == 0 (0 is even, speech.rs:38-40): the tracks entries still do
    with pytest.raises(J.JbError) as ei:
        J.vocode_tracks_batch(v0, [utts[0]])
    assert ei.value.code == -1 and "odd numbers" in str(ei.value)
    # an even count above zero: Vocoder::new takes it (the noise tap of the ring sits at (nlpf - 1) / 2 either way,
    # excitation.rs:137-140), SpeechGenerator::new does not -- 30 of the voice's 31 taps, and 2
    for ne in (30, 2):
        ve = J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha,
                         [vi.streams[0], vi.streams[1], J.StreamInfo(ne, False, False, [[1.0]])])
        te = J.TrackUtterance(tu.spectrum, tu.lf0, np.ascontiguousarray(tu.lpf[:, :ne]))
        g = J.vocoder_synthesize_batch(ve, [te])[0]
        ref = O.vocoder(vi.sampling_frequency, vi.fperiod, vi.alpha, 1.0, tu.lf0[:, 0], tu.spectrum, te.lpf)
        assert_pcm_close(g, ref, 240, what=ne)
        with pytest.raises(J.JbError) as ei:
            J.vocode_tracks_batch(ve, [te])
        assert ei.value.code == -1 and "odd numbers" in str(ei.value)


def test_generator_serves_no_frame_of_a_timed_out_gv(oracle_voice):
    """the first frames a generator hands out come from the serial recursion while the whole utterance
    is in flight; if the resident GV kernel gave up in formation they must come from the redone step."""
    eng = J.Engine.load([VOICE])
    ref = oracle_voice.synthesize(BENCH_LETTER)
    os.environ["JB_GENERATOR_TEST_GANG_TIMEOUT"] = "1"
    try:
        g = eng.generator(BENCH_LETTER)
    finally:
        del os.environ["JB_GENERATOR_TEST_GANG_TIMEOUT"]
    fp = g.fperiod()
    out = np.zeros(len(ref))
    buf = np.zeros(fp)
    for k in range(6):
        assert g.generate_step(buf) == fp
        out[k * fp:(k + 1) * fp] = buf
    out[6 * fp:] = g.generate_all()
    assert_pcm_close(out, ref, 240)
    assert rel_rms(out[:6 * fp], ref[:6 * fp]) <= 1e-8
