"""Filterbank features on the GPU (jb_fbank.hip): the device seam under the precision gates of tests/fbank_ref.py (the
long double model; see tests/test_fbank_abi.py for the gates and for why the f64 log gate runs in unit scale) over
every frame-to-lane mapping, both windows and both frame modes, workgroup boundaries and odd slab offsets; then the
stage in a batch -- equal to the seam on the batch's own PCM bit for bit: plain, behind the converter and the loudness
target, beside the sample format, behind a join, through redo rounds, in the fast invariant mode -- the engine entries
and the rules of jb_batch_set_fbank.

Measured on an MI355X at the six gate shapes: see the ratios this file prints (-s) and DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import fbank_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.mark.parametrize("hz,n_mels,n_fft", R.SHAPES)
@pytest.mark.parametrize("window", [R.HANN, R.HAMMING])
@pytest.mark.parametrize("center", [False, True])
def test_seam_under_the_gates(eng, hz, n_mels, n_fft, window, center):
    """Every frame-to-lane mapping against the long double model: four frames to a workgroup up to n_fft 1024, two at
    2048, one at 4096 (an odd log2 of n_fft / 2: the single last pass), and one filter alone."""
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.fbank_pcm(x, hz, o), hz, n_mels, window, center, "device", n_fft)


def close_to_host(got, x, hz, o):
    """The seam's frames against the host form of the same rule: equal shape, and equal values to a few ulp of the
    frame's power (linear) -- the precise comparison is the gate above; this one catches a misplaced frame."""
    want = J.fbank_host(x, hz, o)
    assert got.shape == want.shape and got.dtype == want.dtype
    if want.size:
        scale = np.abs(want).max(axis=1, keepdims=True)
        assert np.all(np.abs(got - want) <= 1e-13 * scale), (x.size, hz)


# (hz, n_mels, n_fft): a wave per frame and four frames to a workgroup up to 1024, two waves and two frames at 2048,
# the whole workgroup on one frame at 4096
GEOMETRIES = list(R.SHAPES)


def seam_boundaries(hz, n_mels, n_fft, center, win_ms=25, hop_ms=10):
    """One call of many short inputs: T = 0, 1 and one less than, equal to and one more than a multiple of the frames a
    workgroup takes; odd sample counts, so that the inputs start on odd offsets of the packed slab; every frame of
    every input (the first and the last among them) against the host form, and against the same input run alone."""
    wl, hop, nf = R.geometry(hz, 1000 * win_ms, 1000 * hop_ms, n_fft)
    per = 4 if nf <= 1024 else 2 if nf == 2048 else 1
    o = J.fbank(win_ms=win_ms, hop_ms=hop_ms, n_mels=n_mels, n_fft=n_fft, center=center, linear=True, f64=True,
                window="hamming")

    def length(T):  # an odd count of samples that gives T frames
        if center:
            n = T * hop - (hop // 2)
        else:
            n = wl + (T - 1) * hop + 1 if T else wl - 2
        n = max(n, 0)
        n += (n % 2 == 0) if n else 0
        assert R.n_frames(n, wl, hop, center) == T, (n, T)
        return n

    frames = [0, 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per + 1, 1, 0, 5 * per]
    rng = np.random.default_rng(hz + n_mels)
    xs = [rng.normal(0, 4000, length(T)) for T in frames]
    got = J.fbank_pcm(xs, hz, o)
    assert [g.shape[0] for g in got] == frames
    for x, g in zip(xs, got):
        close_to_host(g, x, hz, o)
    # deterministic: the same input alone and among the others, as the 5th of 9
    assert np.array_equal(J.fbank_pcm(xs[4], hz, o), got[4])
    assert np.array_equal(J.fbank_pcm([xs[4]], hz, o)[0], got[4])


@pytest.mark.parametrize("hz,n_mels,n_fft", GEOMETRIES)
@pytest.mark.parametrize("center", [False, True])
def test_seam_over_workgroup_boundaries_and_odd_offsets(eng, hz, n_mels, n_fft, center):
    seam_boundaries(hz, n_mels, n_fft, center)


# The smallest transforms: fewer groups of four points (M / 4 = 8, 16) than the 64 lanes of a frame, log2(M) 5 and 6
@pytest.mark.parametrize("n_fft,win_ms,hop_ms", [(64, 8, 4), (128, 16, 8)])
@pytest.mark.parametrize("center", [False, True])
def test_seam_over_workgroup_boundaries_at_the_smallest_transforms(eng, n_fft, win_ms, hop_ms, center):
    seam_boundaries(8000, 10, n_fft, center, win_ms, hop_ms)


def test_seam_rates_in_one_call_and_the_f32_rows(eng):
    rng = np.random.default_rng(3)
    rates = [8000, 48000, 16000, 48000, 22050]
    xs = [rng.normal(0, 3000, n) for n in (1001, 3001, 1603, 1199, 2207)]
    for o in (J.fbank(n_mels=40), J.fbank(n_mels=23, center=True, unit=True, window="hamming")):
        got = J.fbank_pcm(xs, rates, o)
        o64 = J.fbank(n_mels=o.n_mels, center=bool(o.flags & J.FBANK_CENTER), unit=bool(o.flags & J.FBANK_UNIT),
                      window=o.window, f64=True)
        got64 = J.fbank_pcm(xs, rates, o64)
        for x, hz, g, g64 in zip(xs, rates, got, got64):
            assert g.dtype == np.float32 and g.shape == (R.n_frames(x.size, *R.geometry(hz)[:2], bool(o.flags & 1)), o.n_mels)
            assert np.array_equal(g, g64.astype(np.float32))  # one rounding of the f64 value
            assert np.allclose(g64, J.fbank_host(x, hz, o64), rtol=0, atol=1e-11)
    assert J.fbank_pcm(xs[1], 96000, J.fbank()).shape == (1, 80)  # wl = 2400 in n_fft = 4096
    with pytest.raises(J.JbError, match="win_us"):  # one rate of the call refuses the options: wl = 4800
        J.fbank_pcm(xs, [8000, 48000, 16000, 48000, 192000], J.fbank())


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (9, 40, 23)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 5)


def check_batch(b, o):
    """read_fbank(i) == read_fbank_all()[i] == the seam on the PCM of the same batch, bit for bit."""
    every = b.read_fbank_all()
    assert len(every) == len(b)
    for i in range(len(b)):
        x, hz = b.pcm(i), b.output_rate(i)
        T, m, rate = b.fbank_shape(i)
        assert (m, rate) == (o.n_mels, hz) and T == J.fbank_geometry(hz, o, x.size)[3]
        assert every[i].shape == (T, m) and b.fbank_size(i) == every[i].nbytes
        assert np.array_equal(b.read_fbank(i), every[i])
        assert np.array_equal(every[i], J.fbank_pcm(x, hz, o)), i
    return every


@pytest.mark.parametrize("kw", [dict(), dict(center=True, f64=True, window="hamming", n_mels=40)])
def test_batch_path_equals_the_seam(eng, batch_utts, kw):
    vi, utts = batch_utts
    o = J.fbank(**kw)
    with J.Batch(vi, utts) as b:
        b.set_fbank(o)
        b.run()
        check_batch(b, o)
    with J.Batch(vi, utts) as b:  # behind the converter and the loudness target
        b.set_output_rate(16000)
        b.set_loudness_target(-23.0)
        b.set_fbank(o)
        b.run()
        assert b.output_rate(0) == 16000
        check_batch(b, o)


def test_beside_the_sample_format_and_the_f64_read(eng, batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.run()
        plain = [b.pcm(i).tobytes() for i in range(len(utts))]
        info = b.info()
    o = J.fbank(n_mels=64)
    with J.Batch(vi, utts) as b:
        b.set_format("s16")
        b.set_fbank(o)
        b.run()
        check_batch(b, o)
        for i in range(len(utts)):
            assert b.formatted(i) == J.format_pcm_host(b.pcm(i), "s16")
            assert b.pcm(i).tobytes() == plain[i]  # the request changed no byte of the PCM
        assert b.info() == info  # ... and none of the vocoder's work items


def test_join_features_of_the_programme(eng, batch_utts):
    vi, utts = batch_utts
    o = J.fbank(center=True)
    with J.Batch(vi, utts) as b:
        b.set_join([(0, 100, 333, 16, 16), (None, 0, 0, 0, 0), (0, 7, 2001, 0, 24)])
        b.set_fbank(o)
        b.run()
        assert b.num_outputs() == 2
        every = b.read_fbank_all()
        for p in range(2):
            x = b.programme_pcm(p)
            T, m, hz = b.fbank_shape(p)
            assert (T, m, hz) == (J.fbank_geometry(vi.sampling_frequency, o, x.size)[3], 80, vi.sampling_frequency)
            assert np.array_equal(every[p], J.fbank_pcm(x, hz, o)) and np.array_equal(b.read_fbank(p), every[p])
        with pytest.raises(J.JbError):
            b.fbank_shape(2)


def test_redo_rounds_see_the_final_pcm(eng):
    """Redo rounds forced the way tests/test_gpu_adpcm.py forces them: the features are the seam's on the final PCM,
    every frame of every unit (those in front of the first redone chunk included)."""
    vi, utts = _utts(eng, (600, 1100), 40)
    o = J.fbank(f64=True)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_fbank(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, o)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], float("inf"))
        b.set_join([(0, 0, 480, 0, 0), (0, 0, 0, 0, 0)])
        b.set_fbank(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        x = b.programme_pcm(0)
        assert np.array_equal(b.read_fbank(0), J.fbank_pcm(x, vi.sampling_frequency, o))


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 300, 77)
    others = [synth.synth_utterance(tab, 50 + 13 * k, 1000 + k) for k in range(63)]
    o = J.fbank()
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_fbank(o)
            b.run()
            res.append(b.read_fbank(pos))
    assert np.array_equal(res[0], res[1])
    assert res[0].shape == (J.fbank_geometry(vi.sampling_frequency, o, 300 * vi.fperiod)[3], 80)


def test_engine_entries(eng):
    hz = eng.condition.get_sampling_frequency()
    o = J.fbank(n_mels=40, center=True)
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    one = eng.synthesize_fbank(SAMPLE_SENTENCE_1, o)
    assert np.array_equal(one, J.fbank_pcm(pcm, hz, o)) and one.shape[1] == 40
    assert np.array_equal(eng.synthesize_fbank(SAMPLE_SENTENCE_1, n_mels=40, center=True), one)
    e16 = eng.clone()
    e16.condition.set_output_sampling_frequency(16000)
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    for got, x in zip(e16.synthesize_fbank_batch(sents, o), e16.synthesize_batch(sents)):
        assert np.array_equal(got, J.fbank_pcm(x, 16000, o))
    engines = [eng, e16]
    ref = J.synthesize_batch_each(engines, sents)
    out = J.synthesize_batch_each_fbank(engines, sents, o)
    for got, x, r in zip(out, ref, (hz, 16000)):
        assert np.array_equal(got, J.fbank_pcm(x, r, o))
    prog, starts = eng.synthesize_programme(sents, sink="f64", gap_ms=120.0, fade_ms=2.0)
    feat, starts2 = eng.synthesize_programme(sents, sink="fbank", gap_ms=120.0, fade_ms=2.0, opts=o)
    assert starts == starts2 and np.array_equal(feat, J.fbank_pcm(prog, hz, o))
    with pytest.raises(J.JbError, match="n_mels"):
        eng.synthesize_fbank(SAMPLE_SENTENCE_1, n_mels=200)


def test_rules(eng):
    vi, utts = _utts(eng, (30,), 1)
    L = J.lib()
    UNSUPPORTED = -2
    o = J.fbank()
    with J.Batch(vi, utts, mlpg_only=True) as b:
        assert L.jb_batch_set_fbank(b._h, C.byref(o)) == UNSUPPORTED and b"no PCM" in L.jb_last_error()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        assert L.jb_batch_set_fbank(b._h, C.byref(o)) == UNSUPPORTED and b"JB_BATCH_PCM_I16" in L.jb_last_error()
    with J.Batch(vi, utts) as b:  # without a call: nothing to read
        b.run()
        with pytest.raises(J.JbError, match="was not called"):
            b.fbank_size(0)
        assert L.jb_batch_read_fbank_all(b._h, None) == -1
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="n_mels"):
            b.set_fbank(n_mels=0)
        with pytest.raises(J.JbError, match="win_us"):
            b.set_fbank(win_ms=100)  # 4800 samples at the voice's 48 kHz
        b.set_fbank(win_ms=50)
        with pytest.raises(J.JbError, match="win_us"):
            b.set_fbank(win_ms=50, n_fft=2048)  # 2400 samples do not fit
        with pytest.raises(J.JbError, match="win_us"):
            b.set_output_rate(192000)  # the combined request: 50 ms are 9600 samples there
        b.set_fbank(None)  # withdrawn
        with pytest.raises(J.JbError, match="was not called"):
            b.fbank_size(0)
        b.set_fbank(o)
        n = 30 * vi.fperiod
        T = J.fbank_geometry(vi.sampling_frequency, o, n)[3]
        assert b.fbank_shape(0) == (T, 80, vi.sampling_frequency) and b.fbank_size(0) == T * 80 * 4
        with pytest.raises(J.JbError, match="has not run"):
            b.read_fbank(0)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_fbank(o)
        nby = b.fbank_size(0)
        buf = np.zeros(nby, dtype=np.uint8)
        assert L.jb_batch_read_fbank(b._h, 0, buf.ctypes.data, nby - 1) == -8
        assert L.jb_batch_read_fbank(b._h, 0, None, nby) == -1
        assert L.jb_batch_read_fbank(b._h, 1, buf.ctypes.data, nby) == -1
        assert L.jb_batch_fbank_shape(b._h, 0, None, None, None) == 0
        assert L.jb_batch_read_fbank(b._h, 0, buf.ctypes.data, nby) == 0
        assert np.array_equal(np.frombuffer(buf.tobytes(), dtype=np.float32).reshape(T, 80),
                              J.fbank_pcm(b.pcm(0), vi.sampling_frequency, o))
