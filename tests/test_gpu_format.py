"""Output sample formats on the GPU (jb_format.hip): the device seam against the numpy reference (tests/format_ref.py)
and against the host seam byte for byte, over tails, S24 groups and 16-byte starts; then the stage in a batch -- tied
to the fused 16-bit sink, behind the converter and the loudness apply pass, through redo rounds, in the fast invariant
mode -- the engine entries and the rules of jb_batch_set_format.  Every comparison is bit-exact."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import format_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# the kernel's tile length (samples per workgroup)
T = int(re.search(r"kFmtTile = (\d+);", (ROOT / "jbonsai_amd" / "csrc" / "jb_format.h").read_text()).group(1))
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3]
CASES = [(f, False) for f in R.FORMATS] + [("s16", True), ("s24", True)]


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def seam_inputs():
    """One utterance per length of LENGTHS, drawn from the shared value set, and the whole value set as a last one
    (every integer of the 16-bit range: G.711 exhaustively)."""
    rng = np.random.default_rng(2024)
    utts = [R.VALUES[rng.integers(0, R.VALUES.size, n)] for n in LENGTHS]
    return utts + [R.VALUES]


@pytest.mark.parametrize("fmt,dither", CASES)
def test_seam_is_the_reference(eng, seam_inputs, fmt, dither):
    assert T % 16 == 0
    seed = 0x0123456789ABCDEF
    got = J.format_pcm(seam_inputs, fmt, dither=dither, seed=seed)
    assert len(got) == len(seam_inputs)
    for x, g in zip(seam_inputs, got):
        assert len(g) == x.size * R.BYTES[fmt]
        assert g == R.encode(x, fmt, dither_on=dither, seed=seed), (fmt, x.size)
        assert g == J.format_pcm_host(x, fmt, dither=dither, seed=seed), (fmt, x.size)
    if dither:  # the seed matters, and k counts within the utterance: equal utterances get equal bytes
        a, b = J.format_pcm([seam_inputs[-2], seam_inputs[-2]], fmt, dither=True, seed=seed + 1)
        assert a == b and a != got[-2]


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (700, 2500, 1300)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 3)


def check_batch(b, fmt, dither=False, seed=0):
    """formatted(i) == formatted_all()[i] == the reference applied to pcm(i) of the same batch."""
    every = b.formatted_all()
    pcms = [b.pcm(i) for i in range(len(b))]
    for i, x in enumerate(pcms):
        assert b.formatted(i) == every[i]
        assert len(every[i]) == x.size * R.BYTES[fmt]
        assert every[i] == R.encode(x, fmt, dither_on=dither, seed=seed), i
    return every, pcms


def test_s16_is_the_fused_sink_and_f32_the_scaled_f64(eng, batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.run()
        sink = [b.pcm_i16(i) for i in range(len(utts))]
    with J.Batch(vi, utts) as b:
        b.set_format("s16")
        b.run()
        every, pcms = check_batch(b, "s16")
        for i in range(len(utts)):
            assert every[i] == sink[i].astype("<i2").tobytes(), i
    with J.Batch(vi, utts) as b:
        b.set_format("f32")
        b.run()
        every, pcms = check_batch(b, "f32")
        for i in range(len(utts)):
            assert every[i] == (pcms[i] / 32768).astype(np.float32).tobytes(), i
    # the f64 read entries kept working above; what they hand out is what a batch without the stage hands out
    with J.Batch(vi, utts) as plain:
        plain.run()
        for i in range(len(utts)):
            assert plain.pcm(i).tobytes() == pcms[i].tobytes()


def test_behind_the_converter_and_behind_the_apply_pass(eng, batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.set_output_rate(8000)
        b.set_format("ulaw")
        b.run()
        every, pcms = check_batch(b, "ulaw")
        assert [len(e) for e in every] == [b.num_samples(i) for i in range(len(utts))]
        assert b.output_rate(0) == 8000 and len(every[0]) == FRAMES[0] * vi.fperiod // 6
    with J.Batch(vi, utts) as b:
        b.set_loudness_target([-20.0, -26.0, -16.0], -1.0)
        b.set_format("s24", dither=True, seed=5)
        b.run()
        check_batch(b, "s24", dither=True, seed=5)
    with J.Batch(vi, utts) as b:
        b.set_output_rate([22050, 0, 16000])
        b.set_loudness_target(-23.0)
        b.set_format("alaw")
        b.run()
        check_batch(b, "alaw")


def test_redo_rounds_format_the_final_pcm(eng):
    vi, utts = _utts(eng, (600, 1100), 40)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_format("s16", dither=True, seed=11)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, "s16", dither=True, seed=11)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], math.inf)
        b.set_format("f32")
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, "f32")


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_format("s16", dither=True, seed=42)
            b.run()
            res.append(b.formatted(pos))
    assert res[0] == res[1] and len(res[0]) == 2 * 900 * vi.fperiod


def test_engine_entries(eng):
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    assert eng.synthesize_formatted(SAMPLE_SENTENCE_1, "f32") == R.encode(pcm, "f32")
    e8 = eng.clone()
    e8.condition.set_output_sampling_frequency(8000)
    pcm8 = e8.synthesize(SAMPLE_SENTENCE_1)
    assert pcm8.size == math.ceil(pcm.size / 6)
    assert e8.synthesize_formatted(SAMPLE_SENTENCE_1, "alaw") == R.encode(pcm8, "alaw")
    e2 = eng.clone()
    e2.condition.set_output_sampling_frequency(22050)
    e2.condition.set_loudness_target(-18.0)
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    engines = [eng, e2, e8]
    ref = J.synthesize_batch_each(engines, sents)
    out = J.synthesize_batch_each_formatted(engines, sents, "s24", dither=True, seed=3)
    for data, x in zip(out, ref):
        assert data == R.encode(x, "s24", dither_on=True, seed=3)
    (one,) = e2.synthesize_batch_formatted([SAMPLE_SENTENCE_2], "ulaw")
    assert one == R.encode(ref[1], "ulaw")


def test_rules(eng):
    vi, utts = _utts(eng, (100,), 1)
    with J.Batch(vi, utts, pcm_i16=True) as b:  # the stage reads f64
        with pytest.raises(J.JbError, match="f64"):
            b.set_format("s16")
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError, match="no PCM"):
            b.set_format("s16")
    with J.Batch(vi, utts) as b:
        for fmt, dither in ((0, False), (9, False), ("f32", True), ("ulaw", True), ("alaw", True)):
            with pytest.raises(J.JbError):
                b.set_format(fmt, dither=dither)
        with pytest.raises(J.JbError):  # no format set
            b.formatted(0)
        b.set_format("s24")
        with pytest.raises(J.JbError, match="has not run"):
            b.formatted(0)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_format("s16")
        n = b.num_samples(0) * 3
        buf = np.zeros(n, dtype=np.uint8)
        L = J.lib()
        assert L.jb_batch_read_formatted(b._h, 0, buf.ctypes.data, n - 1) == -8  # a short cap
        assert L.jb_batch_read_formatted(b._h, 0, None, n) == -1
        assert L.jb_batch_read_formatted(b._h, 1, buf.ctypes.data, n) == -1
        assert L.jb_batch_formatted_size(b._h, 0, None) == -1
        assert L.jb_batch_read_formatted_all(b._h, None) == -1
        assert L.jb_batch_read_formatted(b._h, 0, buf.ctypes.data, n) == 0
        assert buf.tobytes() == R.encode(b.pcm(0), "s24")
        with pytest.raises(J.JbError):  # the 16-bit read entry behaves as before on an f64 batch
            b.pcm_i16(0)
    with J.Batch(vi, utts) as b:  # without a call: nothing to read
        b.run()
        with pytest.raises(J.JbError, match="was not called"):
            b.formatted(0)
