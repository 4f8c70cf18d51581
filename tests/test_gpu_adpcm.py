"""IMA ADPCM on the GPU (jb_adpcm.hip): the device seam against the host encoder byte for byte (the host encoder is
held to the pure-Python model by tests/test_adpcm_abi.py) over block, wave and workgroup boundaries; then the stage in
a batch -- from f64 and from the 16-bit sink, behind the converter and the loudness apply pass, beside the sample
format and FLAC, through redo rounds, in the fast invariant mode -- the engine entries and the rules of
jb_batch_set_adpcm.  Every comparison is bit-exact."""
import math
import struct

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import flac_ref
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def pcm_of(n, seed):
    """n f64 samples in 16-bit scale: noise under a slow envelope, with stretches of out-of-range and off-integer
    values and of silence."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    x = rng.standard_normal(n) * 6000.0 * (0.6 + 0.5 * np.sin(k / 97.0))
    odd = np.array([40000.7, -40000.7, 32767.999, -32768.999, 12.999, -12.999, 0.999, -0.999])
    m = (k // 40) % 7 == 3
    x[m] = odd[rng.integers(0, odd.size, int(m.sum()))]
    x[(k // 100) % 5 == 4] = 0.0
    return x


def check_seam(lengths, rates, align):
    utts = [pcm_of(n, 7 * n + 1) for n in lengths]
    got = J.adpcm_encode(utts, rates, align)
    assert len(got) == len(utts)
    hz = [rates] * len(utts) if np.isscalar(rates) else rates
    for x, h, g in zip(utts, hz, got):
        assert len(g) == J.adpcm_geometry(h, x.size, align)[3]
        assert g == J.adpcm_encode_host(x, h, align), (x.size, h, align)


def test_seam_is_the_host_encoder_over_wave_and_workgroup_boundaries(eng):
    """A = 32 (57 samples per block) keeps the shapes tiny: one call with ragged lengths around a block, a wave's 64
    blocks and a workgroup's 256."""
    check_seam([0, 1, 9, 56, 57, 58, 64 * 57 - 1, 64 * 57, 64 * 57 + 1, 256 * 57 + 3], 16000, 32)


@pytest.mark.parametrize("A", [256, 1024])
def test_seam_at_the_default_block_sizes(eng, A):
    spb = 2 * (A - 4) + 1
    check_seam([0, 1, 9, spb - 1, spb, spb + 1, 2 * spb, 2 * spb + 1, 3 * spb], 16000, A)


def test_seam_block_size_follows_each_rate(eng):
    check_seam([3000, 3000, 1200, 5000], [8000, 48000, 48000, 8000], 0)
    one = pcm_of(700, 1)
    assert J.adpcm_encode(one, 22050) == J.adpcm_encode_host(one, 22050, 512)


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (1, 7, 40)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 3)


def check_batch(b, i16, align=0):
    """read_adpcm(i) == read_adpcm_all()[i] == the host encoder applied to the PCM of the same batch."""
    every = b.read_adpcm_all()
    for i in range(len(b)):
        x = b.pcm_i16(i) if i16 else b.pcm(i)
        hz = b.output_rate(i)
        A = J.adpcm_geometry(hz, 0, align)[0]
        assert b.adpcm_block_align(i) == A
        assert b.read_adpcm(i) == every[i]
        assert len(every[i]) == b.adpcm_size(i) == J.adpcm_geometry(hz, x.size, align)[3]
        assert every[i] == J.adpcm_encode_host(x, hz, align), i
    return every


def both(vi, utts, align=0, setup=lambda b: None):
    """The stage on an f64 batch and on a 16-bit batch of the same utterances: each right, and the two equal."""
    res = []
    for i16 in (False, True):
        with J.Batch(vi, utts, pcm_i16=i16) as b:
            setup(b)
            b.set_adpcm(align)
            b.run()
            res.append(check_batch(b, i16, align))
    assert res[0] == res[1]
    return res[0]


@pytest.mark.parametrize("align", [0, 32])
def test_batch_from_f64_and_from_the_16_bit_sink(eng, batch_utts, align):
    vi, utts = batch_utts
    every = both(vi, utts, align)
    assert [len(e) for e in every] == [J.adpcm_geometry(vi.sampling_frequency, t * vi.fperiod, align)[3]
                                       for t in FRAMES]


def test_behind_the_converter_and_behind_the_apply_pass(eng, batch_utts):
    vi, utts = batch_utts

    def rate8(b):
        b.set_output_rate(8000)

    def loud(b):
        b.set_loudness_target([-20.0, -26.0, -16.0], -1.0)

    def mixed(b):
        b.set_output_rate([8000, 0, 22050])
        b.set_loudness_target(-23.0)

    both(vi, utts, 0, rate8)
    both(vi, utts, 0, loud)
    both(vi, utts, 32, mixed)
    with J.Batch(vi, utts) as b:
        mixed(b)
        b.set_adpcm()
        assert [b.adpcm_block_align(i) for i in range(3)] == [256, J.adpcm_geometry(vi.sampling_frequency, 0)[0], 512]


def test_beside_the_sample_format_and_beside_flac(eng, batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.set_format("s16")
        b.set_adpcm()
        b.run()
        check_batch(b, False)
        for i in range(len(utts)):
            assert b.formatted(i) == J.format_pcm_host(b.pcm(i), "s16")
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_adpcm(64)
        b.set_flac()
        b.run()
        check_batch(b, True, 64)
        for i in range(len(utts)):
            dec, _ = flac_ref.decode(b.flac(i))
            assert np.array_equal(dec, b.pcm_i16(i))


def test_redo_rounds_encode_the_final_pcm(eng):
    vi, utts = _utts(eng, (600, 1100), 40)
    for i16 in (False, True):
        with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
            b.set_adpcm()
            b.run()
            b.sync()
            assert b.info()["n_redo"] >= 4
            check_batch(b, i16)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], math.inf)
        b.set_adpcm(256)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, False, 256)


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_adpcm()
            b.run()
            res.append(b.read_adpcm(pos))
    assert res[0] == res[1] and len(res[0]) == J.adpcm_geometry(vi.sampling_frequency, 900 * vi.fperiod)[3]


def test_engine_entries(eng, tmp_path):
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    hz = eng.condition.get_sampling_frequency()
    one = eng.synthesize_adpcm(SAMPLE_SENTENCE_1)
    assert (one.n_samples, one.hz, one.block_align) == (pcm.size, hz, J.adpcm_geometry(hz, 0)[0])
    assert one.data == J.adpcm_encode_host(pcm, hz)
    e8 = eng.clone()
    e8.condition.set_output_sampling_frequency(8000)
    pcm8 = e8.synthesize(SAMPLE_SENTENCE_1)
    s8 = e8.synthesize_adpcm(SAMPLE_SENTENCE_1)
    assert (s8.n_samples, s8.hz, s8.block_align) == (pcm8.size, 8000, 256)
    assert s8.data == J.adpcm_encode_host(pcm8, 8000)
    e2 = eng.clone()
    e2.condition.set_output_sampling_frequency(22050)
    e2.condition.set_loudness_target(-18.0)
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
    engines = [eng, e2, e8]
    ref = J.synthesize_batch_each(engines, sents)
    out = J.synthesize_batch_each_adpcm(engines, sents)
    assert [s.block_align for s in out] == [J.adpcm_geometry(hz, 0)[0], 512, 256]
    for s, x, e in zip(out, ref, engines):
        assert s.n_samples == x.size and s.data == J.adpcm_encode_host(x, s.hz)
    (b2,) = e2.synthesize_adpcm_batch([SAMPLE_SENTENCE_2], block_align=128)
    assert b2.block_align == 128 and b2.data == J.adpcm_encode_host(ref[1], 22050, 128)
    # the WAV round trip: the file's data chunk decodes to the decoder's samples, close to the PCM
    path = tmp_path / "a.wav"
    s8.write_wav(path)
    raw = path.read_bytes()
    assert struct.unpack_from("<H", raw, 20)[0] == 0x11 and struct.unpack_from("<I", raw, 48)[0] == pcm8.size
    dec = J.adpcm_decode_host(raw[60:], 256, pcm8.size)
    assert np.array_equal(dec, s8.decode())
    q = np.trunc(np.clip(pcm8, -32768, 32767))
    assert np.array_equal(dec[::505], q[::505].astype(np.int16))
    with pytest.raises(J.JbError):
        eng.synthesize_adpcm(SAMPLE_SENTENCE_1, block_align=30)


def test_rules(eng):
    vi, utts = _utts(eng, (100,), 1)
    n = 100 * vi.fperiod
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError, match="no PCM"):
            b.set_adpcm()
    with J.Batch(vi, utts) as b:  # without a call: nothing to read, and the run of today
        b.run()
        with pytest.raises(J.JbError, match="was not called"):
            b.read_adpcm(0)
        with pytest.raises(J.JbError, match="was not called"):
            b.adpcm_size(0)
        plain, info = b.pcm(0).tobytes(), b.info()
    with J.Batch(vi, utts) as b:
        for bad in (4, 30, 8196):
            with pytest.raises(J.JbError, match="block_align"):
                b.set_adpcm(bad)
        o = J._ffi.adpcm_opts(0)
        o.reserved[2] = 7
        L = J.lib()
        assert L.jb_batch_set_adpcm(b._h, o) == -1 and L.jb_batch_set_adpcm(b._h, None) == -1
        b.set_adpcm(64)
        b.set_adpcm()  # the last request before the run wins
        # sizes before the run, from geometry alone
        A, _, _, nby = J.adpcm_geometry(vi.sampling_frequency, n)
        assert b.adpcm_size(0) == nby and b.adpcm_block_align(0) == A
        with pytest.raises(J.JbError, match="has not run"):
            b.read_adpcm(0)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_adpcm()
        buf = np.zeros(nby, dtype=np.uint8)
        assert L.jb_batch_read_adpcm(b._h, 0, buf.ctypes.data, nby - 1) == -8  # a short cap
        assert L.jb_batch_read_adpcm(b._h, 0, None, nby) == -1
        assert L.jb_batch_read_adpcm(b._h, 1, buf.ctypes.data, nby) == -1
        assert L.jb_batch_adpcm_size(b._h, 0, None) == -1
        assert L.jb_batch_read_adpcm_all(b._h, None) == -1
        assert L.jb_batch_read_adpcm(b._h, 0, buf.ctypes.data, nby) == 0
        assert buf.tobytes() == J.adpcm_encode_host(b.pcm(0), vi.sampling_frequency)
        # the request changed neither the PCM nor the vocoder's work items
        assert b.pcm(0).tobytes() == plain and b.info() == info
