"""The pitch stage in a batch's chain and behind the engine (jb_batch_set_pitch, jb_synthesize_pitch and their kin): the
batch path equals the seam jb_pitch_pcm_batch on the PCM of the same batch bit for bit -- alone, behind the converter at
16 kHz, behind a join, behind a mix with stems (P + S units), through forced redo rounds, and under the fast invariant
mode in two different batches; with the request added the batch's PCM and its fbank bytes keep their bits, and without
it the batch is the one that never heard of the request; the engine's [T][3] has synthesize_fbank's T."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (9, 40, 23)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 5)


def check_units(b, o, pcm_of):
    """read_pitch(i) == read_pitch_all()[i] == the seam on unit i's PCM of the same batch, bit for bit"""
    every = b.read_pitch_all()
    assert len(every) == b.num_outputs()
    for i in range(b.num_outputs()):
        x = pcm_of(i)
        T, width, hz = b.pitch_shape(i)
        g = J.pitch_geometry(o, hz, x.size)
        assert (T, width) == (g.T, g.width) and every[i].shape == (T, width) and b.pitch_size(i) == every[i].nbytes
        assert np.array_equal(b.read_pitch(i), every[i], equal_nan=True)
        want = J.pitch_pcm([x], hz, o)[0][0]
        assert every[i].tobytes() == want.tobytes(), i
    return every


@pytest.mark.parametrize("kw", [dict(), dict(grid="snip", raw=True, f64=True), dict(raw_log=True, f64=True, hop_ms=5)])
def test_batch_path_equals_the_seam(eng, batch_utts, kw):
    vi, utts = batch_utts
    o = J.pitch(**kw)
    with J.Batch(vi, utts) as b:
        b.set_pitch(o)
        b.run()
        every = check_units(b, o, b.pcm)
        assert every[1].shape[0] > 10
    with J.Batch(vi, utts) as b:  # behind the converter and a loudness target
        b.set_output_rate(16000)
        b.set_loudness_target(-23.0)
        b.set_pitch(o)
        b.run()
        assert b.output_rate(0) == 16000 and b.pitch_shape(0)[2] == 16000
        check_units(b, o, b.pcm)


def test_request_changes_no_other_byte(eng, batch_utts):
    vi, utts = batch_utts
    fo = J.fbank(n_mels=40)
    with J.Batch(vi, utts) as b:
        b.set_fbank(fo)
        b.run()
        plain = [b.pcm(i).tobytes() for i in range(len(utts))]
        feats = [f.tobytes() for f in b.read_fbank_all()]
        info = b.info()
        with pytest.raises(J.JbError, match="jb_batch_set_pitch was not called"):
            b.pitch_size(0)
    o = J.kaldi_pitch()
    with J.Batch(vi, utts) as b:
        b.set_fbank(fo)
        b.set_pitch(o)
        b.run()
        check_units(b, o, b.pcm)
        assert [f.tobytes() for f in b.read_fbank_all()] == feats  # the fbank sink keeps its bytes
        assert [b.pcm(i).tobytes() for i in range(len(utts))] == plain  # ... and the PCM its own
        assert b.info() == info  # ... and the vocoder its work items
        T = [b.pitch_shape(i)[0] for i in range(len(utts))]
    with J.Batch(vi, utts) as b:  # the same frame grid: the rows concatenate
        b.set_fbank(J.fbank(n_mels=40))
        b.set_frame(J.frame(reflect=True))
        b.run()
        assert [b.read_fbank(i).shape[0] for i in range(len(utts))] == T
    with J.Batch(vi, utts) as b:  # set and withdrawn: the batch that never heard of the request
        b.set_fbank(fo)
        b.set_pitch(o)
        b.set_pitch(None)
        b.run()
        assert [b.pcm(i).tobytes() for i in range(len(utts))] == plain and b.info() == info
        assert [f.tobytes() for f in b.read_fbank_all()] == feats


def test_join_and_mix_with_stems(eng, batch_utts):
    vi, utts = batch_utts
    o = J.pitch(raw_log=True, f64=True)
    with J.Batch(vi, utts) as b:
        b.set_join([(0, 100, 333, 16, 16), (None, 0, 0, 0, 0), (0, 7, 2001, 0, 24)])
        b.set_pitch(o)
        b.run()
        assert b.num_outputs() == 2
        check_units(b, o, b.programme_pcm)  # the normalisation runs over the whole programme
        with pytest.raises(J.JbError):
            b.pitch_shape(2)
    with J.Batch(vi, utts) as b:
        b.set_mix([(0, 0, 0.0, 0, 0, 0), (0, 2000, -6.0, 0, 0, 0), (0, 500, -3.0, 0, 0, 0)])
        b.set_mix_stems([0, 1, 0])
        b.set_pitch(o)
        b.run()
        assert b.num_programmes() == 1 and b.num_outputs() == 3  # P + S units
        check_units(b, o, b.programme_pcm)


def test_redo_rounds_see_the_final_pcm(eng):
    """Redo rounds forced the way tests/test_gpu_chain_redo.py forces them"""
    vi, utts = _utts(eng, (600, 1100), 40)
    o = J.pitch(raw_log=True, f64=True)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_pitch(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_units(b, o, b.pcm)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], float("inf"))
        b.set_join([(0, 0, 480, 0, 0), (0, 0, 0, 0, 0)])
        b.set_pitch(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_units(b, o, b.programme_pcm)


def test_invariance_alone_and_among_24(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 40, 77)
    others = [synth.synth_utterance(tab, 15 + k % 26, 1000 + k) for k in range(23)]
    o = J.kaldi_pitch()
    res = []
    for utts, pos in (([probe], 0), (others[:9] + [probe] + others[9:], 9)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_pitch(o)
            b.run()
            res.append(b.read_pitch(pos))
    assert res[0].tobytes() == res[1].tobytes() and res[0].shape[1] == 3 and res[0].shape[0] > 10


def test_engine_entries(eng):
    hz = eng.condition.get_sampling_frequency()
    o = J.kaldi_pitch()
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    one = eng.synthesize_pitch(SAMPLE_SENTENCE_1, o)
    assert one.ndim == 2 and one.shape[1] == 3 and one.dtype == np.float32
    assert one.shape[0] == J.pitch_geometry(o, hz, pcm.size).T
    assert one.tobytes() == J.pitch_pcm([pcm], hz, o)[0][0].tobytes()
    snip = J.pitch(grid="snip")
    assert eng.synthesize_pitch(SAMPLE_SENTENCE_1, snip).shape[0] == eng.synthesize_fbank(SAMPLE_SENTENCE_1).shape[0]
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    for got, x in zip(eng.synthesize_pitch_batch(sents, o), eng.synthesize_batch(sents)):
        assert got.tobytes() == J.pitch_pcm([x], hz, o)[0][0].tobytes()
    prog, starts = eng.synthesize_programme(sents, sink="f64", gap_ms=120.0, fade_ms=2.0)
    feat, starts2 = eng.synthesize_programme(sents, sink="pitch", gap_ms=120.0, fade_ms=2.0, opts=o)
    assert starts == starts2 and feat.tobytes() == J.pitch_pcm([prog], hz, o)[0][0].tobytes()
    with pytest.raises(J.JbError, match="win_us"):
        eng.synthesize_pitch(SAMPLE_SENTENCE_1, win_ms=25.1)
    from jbonsai_amd import _ffi as F
    from jbonsai_amd.engine import _byte_outs, _utt_lines
    e16 = eng.clone()
    e16.condition.set_output_sampling_frequency(16000)
    lines, offs, B = _utt_lines(sents)
    bufs, ns, nf = _byte_outs(B, counts=True)
    hs = (C.c_void_p * B)(eng._h, e16._h)
    F.check(J.lib().jb_synthesize_batch_each_pitch(hs, lines, offs, B, -1, C.byref(o), bufs, ns, nf))
    out = F.take_pitch(J.lib(), bufs, ns, B, o)
    for got, x, r, T in zip(out, J.synthesize_batch_each([eng, e16], sents), (hz, 16000), nf):
        assert got.shape[0] == T and got.tobytes() == J.pitch_pcm([x], r, o)[0][0].tobytes()


def test_rules(eng, batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts, pcm_i16=True) as b:
        with pytest.raises(J.JbError, match="f64"):
            b.set_pitch(J.kaldi_pitch())
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="hop_us"):
            b.set_pitch(hop_ms=10.1)
        b.set_pitch(J.kaldi_pitch())
        with pytest.raises(J.JbError):
            b.set_output_rate(3000)  # below the analysis rate
        b.run()
        with pytest.raises(J.JbError):
            b.set_pitch(None)
