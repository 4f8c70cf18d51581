"""Mel spectrograms on the GPU (jb_melspec.hip): the device seam under the precision gates of tests/melspec_ref.py (the
long double model; see tests/test_melspec_abi.py for the gates) over the ten shapes -- each radix alone, mixed radices,
a window shorter than the transform, one, two and four frames to a workgroup -- then bit equality of the seam with
itself across workgroup boundaries, odd slab offsets, rates and neighbours; the stage in a batch -- equal to the seam on
the batch's own PCM bit for bit: plain, behind the converter and the loudness target, beside an fbank request, behind a
join, through redo rounds with a range clamp, in the fast invariant mode -- the engine entries and the rules of
jb_batch_set_melspec.

Measured on an MI355X: see the ratios this file prints (-s) and profiles/r24_melspec.txt."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import melspec_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.mark.parametrize("shape", R.SHAPES)
def test_seam_under_the_gates(eng, shape):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.melspec_pcm(x, shape[0], o), shape, "device")


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[5], R.SHAPES[6], R.SHAPES[7]])
@pytest.mark.parametrize("pad,magnitude", [(R.ZERO, False), (R.NONE, False), (R.REFLECT, True), (R.NONE, True)])
def test_seam_under_the_gates_other_modes(eng, shape, pad, magnitude):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.melspec_pcm(x, shape[0], o), shape, "device", pad, magnitude)


def close_to_host(got, x, hz, o):
    """The seam's frames against the host form of the same rule (the same butterflies; the logarithm is each side's
    own): equal shape, and equal values to 1e-9 of the unit's largest -- the precise comparison is the gate above (a
    filter that holds 1e-7 of its frame's spectrum may differ by 1e-9 in its logarithm); this one catches a misplaced
    frame, a wrong reflection or a wrong maximum."""
    want = J.melspec_host(x, hz, o)
    assert got.shape == want.shape and got.dtype == want.dtype
    if want.size:
        assert np.all(np.abs(got - want) <= 1e-9 * max(1.0, float(np.abs(want).max()))), (x.size, hz)


def _lengths(N, H, pad):
    """Odd sample counts (so that the inputs start on odd offsets of the packed slab) whose frame counts are 0, the
    smallest the padding allows, and one less than, equal to and one more than multiples of the frames a workgroup
    takes."""
    per = 4 if N <= 1024 else 2 if N <= 2048 else 1
    t_min = R.n_frames(N // 2 + 1 if pad == R.REFLECT else N if pad == R.NONE else 0, N, H, pad)
    frames = [t_min, t_min + 1, 2 * per - 1, 2 * per, 2 * per + 1, 3 * per + 1, 5 * per, 9 * per + 1]
    ns = [0, (N // 2 - 1) | 1]
    for T in frames:
        if T < t_min:
            continue
        n = (T - 1) * H + (N if pad == R.NONE else 0)
        n = max(n + 1 - n % 2, (N // 2 + 1) | 1 if pad == R.REFLECT else 1)
        ns.append(n)
    return ns


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("pad", [R.REFLECT, R.ZERO, R.NONE])
def test_seam_over_workgroup_boundaries_and_odd_offsets(eng, shape, pad):
    """One call of many short inputs, with a range clamp (all three kernels) and without: every frame of every input
    against the host form, the f32 rows one rounding of the f64 rows, and each input run alone equal to itself among
    the others, bit for bit."""
    hz, N, W, H, n_mels, _ = shape
    rng = np.random.default_rng(hz + N + pad)
    xs = [rng.normal(0, 4000, n) * (1e-3 if k % 3 == 2 else 1.0) for k, n in enumerate(_lengths(N, H, pad))]
    name = ("reflect", "zero", "none")[pad]
    for kw in (dict(log="log10", range=3.0, offset=4.0, scale=0.25), dict(log="db", drop_last=pad != R.NONE),
               dict(log="none")):
        o = R.opts_of(shape, f64=True, pad=name, **kw)
        got = J.melspec_pcm(xs, hz, o)
        assert [g.shape[0] for g in got] == [R.n_frames(x.size, N, H, pad, kw.get("drop_last", False)) for x in xs]
        for x, g in zip(xs, got):
            close_to_host(g, x, hz, o)
        got32 = J.melspec_pcm(xs, hz, R.opts_of(shape, pad=name, **kw))
        for g, g32 in zip(got, got32):
            assert g32.dtype == np.float32 and np.array_equal(g32, g.astype(np.float32))
        for k in (len(xs) - 1, len(xs) // 2, 2):
            assert np.array_equal(J.melspec_pcm(xs[k], hz, o), got[k])
            assert np.array_equal(J.melspec_pcm([xs[k]], hz, o)[0], got[k])
    # the clamp is each unit's own: a quiet input (60 dB down) is not flattened by its loud neighbours' maximum
    got = J.melspec_pcm(xs, hz, R.opts_of(shape, f64=True, pad=name, log="log10", range=3.0))
    assert all(g.min() >= g.max() - 3.0 for g in got if g.size)
    k = max(i for i in range(len(xs)) if i % 3 == 2)
    quiet, loud = got[k], got[k - 1]
    assert quiet.size and loud.size and quiet.max() < loud.max() - 3.0 and quiet.max() > quiet.min()


def test_seam_rates_in_one_call(eng):
    """Several rates in one call: window and hop are in samples, the filters follow each unit's rate; each unit equals
    itself run alone at its rate."""
    rng = np.random.default_rng(3)
    rates = [8000, 48000, 16000, 48000, 22050]
    xs = [rng.normal(0, 3000, n) for n in (2001, 6001, 3203, 2399, 4407)]
    for o in (J.melspec(n_fft=400, hop=160, n_mels=40, f_max=4000.0, log="db", range=80.0),
              J.melspec(n_fft=600, win=500, hop=150, n_mels=23, mel_scale="htk", norm="none", pad="zero", f64=True)):
        got = J.melspec_pcm(xs, rates, o)
        for x, hz, g in zip(xs, rates, got):
            assert g.dtype == o.dtype and g.shape == (R.n_frames(x.size, o.n_fft, o.hop_length, o.pad), o.n_mels)
            assert np.array_equal(g, J.melspec_pcm(x, hz, o))
            close_to_host(g, x, hz, o)
    assert not np.array_equal(got[1], J.melspec_pcm(xs[1], 16000, o))  # (the rate matters)
    with pytest.raises(J.JbError, match="f_max_hz"):  # one rate of the call refuses the options
        J.melspec_pcm(xs, rates, J.melspec(n_fft=400, hop=160, f_max=8000.0))


@pytest.mark.parametrize("pad", ["none", "reflect"])
def test_seam_rates_and_workgroup_edges_in_one_call_with_a_range(eng, pad):
    """What the pass builder numbers (class, T, g0, the workgroup count) under range = 8.0, whose maxima per workgroup
    and per unit lie at g0 and at the unit's place: eight units at 16 and 48 kHz interleaved, n_fft 512 (four frames to
    a workgroup), of 0, 1, n_fft - 1, n_fft, n_fft + 4 hop (one frame past a workgroup without padding) and n_fft + 3 hop
    (exactly one workgroup) samples -- the last two at both rates.  Each unit of the one call has the bytes of its own
    call.  (test_seam_rates_in_one_call compares the same way at ordinary lengths.)"""
    rng = np.random.default_rng(512)
    N, hop = 512, 128
    o = J.melspec(n_fft=N, hop=hop, n_mels=23, pad=pad, range=8.0)
    rates = [16000, 48000] * 4
    xs = [rng.normal(0, 3000, n) * np.where(np.arange(n) < n // 2, 1e-3, 1.0)  # (60 dB under the rest: 13.8 > 8)
          for n in (0, 1, N - 1, N, N + 4 * hop, N + 3 * hop, N + 3 * hop, N + 4 * hop)]
    got = J.melspec_pcm(xs, rates, o)
    if pad == "none":
        assert [g.shape[0] for g in got] == [0, 0, 0, 1, 5, 4, 4, 5]
    for x, hz, g in zip(xs, rates, got):
        assert g.shape == (J.melspec_geometry(hz, o, x.size)[3], 23)
        assert g.tobytes() == J.melspec_pcm(x, hz, o).tobytes()
    assert any(np.sum(g == g.min()) > 1 for g in got if g.size)  # (the range bites: a unit's quiet head is clamped)


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (9, 40, 23)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 5)


def check_batch(b, o):
    """read_melspec(i) == read_melspec_all()[i] == the seam on the PCM of the same batch, bit for bit."""
    every = b.read_melspec_all()
    assert len(every) == len(b)
    for i in range(len(b)):
        x, hz = b.pcm(i), b.output_rate(i)
        T, m, rate = b.melspec_shape(i)
        assert (m, rate) == (o.n_mels, hz) and T == J.melspec_geometry(hz, o, x.size)[3] and T > 0
        assert every[i].shape == (T, m) and b.melspec_size(i) == every[i].nbytes
        assert np.array_equal(b.read_melspec(i), every[i])
        assert np.array_equal(every[i], J.melspec_pcm(x, hz, o)), i
    return every


@pytest.mark.parametrize("kw", [dict(n_fft=1200, hop=480), dict(n_fft=2048, win=1500, hop=512, n_mels=40, log="db",
                                                                range=60.0, f64=True, pad="zero"),
                                dict(n_fft=4000, hop=400, n_mels=128, log="log10", range=8.0, offset=4.0, scale=0.25)])
def test_batch_path_equals_the_seam(eng, batch_utts, kw):
    vi, utts = batch_utts
    o = J.melspec(**kw)
    with J.Batch(vi, utts) as b:
        b.set_melspec(o)
        b.run()
        check_batch(b, o)
    with J.Batch(vi, utts) as b:  # behind the converter and the loudness target: Whisper's front end at 16 kHz
        w = J.whisper_mel(80)
        b.set_output_rate(16000)
        b.set_loudness_target(-23.0)
        b.set_melspec(w)
        b.run()
        assert b.output_rate(0) == 16000
        every = check_batch(b, w)
        assert all(e.min() >= e.max() - 2.0 - 1e-6 for e in every)  # (max - 8 + 4) / 4, to an f32 rounding


def test_beside_an_fbank_request_and_the_f64_read(eng, batch_utts):
    vi, utts = batch_utts
    fo = J.fbank(n_mels=64)
    with J.Batch(vi, utts) as b:
        b.set_fbank(fo)
        b.run()
        plain = [b.pcm(i).tobytes() for i in range(len(utts))]
        feats = [f.tobytes() for f in b.read_fbank_all()]
        info = b.info()
    o = J.melspec(n_fft=1200, hop=480, log="db", range=80.0)
    with J.Batch(vi, utts) as b:
        b.set_fbank(fo)
        b.set_melspec(o)
        b.run()
        check_batch(b, o)
        assert [f.tobytes() for f in b.read_fbank_all()] == feats  # the fbank sink keeps its slab and its bytes
        for i in range(len(utts)):
            assert b.pcm(i).tobytes() == plain[i]  # the request changed no byte of the PCM
        assert b.info() == info  # ... and none of the vocoder's work items


def test_join_features_of_the_programme(eng, batch_utts):
    vi, utts = batch_utts
    o = J.melspec(n_fft=1200, hop=480, log="log10", range=8.0, f64=True)
    with J.Batch(vi, utts) as b:
        b.set_join([(0, 100, 333, 16, 16), (None, 0, 0, 0, 0), (0, 7, 2001, 0, 24)])
        b.set_melspec(o)
        b.run()
        assert b.num_outputs() == 2
        every = b.read_melspec_all()
        for p in range(2):
            x = b.programme_pcm(p)
            T, m, hz = b.melspec_shape(p)
            assert (T, m, hz) == (J.melspec_geometry(vi.sampling_frequency, o, x.size)[3], 80, vi.sampling_frequency)
            assert np.array_equal(every[p], J.melspec_pcm(x, hz, o)) and np.array_equal(b.read_melspec(p), every[p])
        # the clamp runs under the whole programme's maximum: the frames inside the trailing pad are silent (log10 of
        # the floor, -10) and sit exactly 8 below it, unless the programme's maximum itself is below -2
        assert every[0].min() == max(every[0].max() - 8.0, -10.0)
        with pytest.raises(J.JbError):
            b.melspec_shape(2)


def test_redo_rounds_see_the_final_pcm(eng):
    """Redo rounds forced the way tests/test_gpu_fbank.py forces them, with a range clamp, so that a redo has to move
    the unit's maximum: the features are the seam's on the final PCM, every frame of every unit."""
    vi, utts = _utts(eng, (600, 1100), 40)
    o = J.melspec(n_fft=1200, hop=480, log="log10", range=4.0, f64=True)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_melspec(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, o)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], float("inf"))
        b.set_join([(0, 0, 480, 0, 0), (0, 0, 0, 0, 0)])
        b.set_melspec(o)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        x = b.programme_pcm(0)
        assert np.array_equal(b.read_melspec(0), J.melspec_pcm(x, vi.sampling_frequency, o))


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 40, 77)
    others = [synth.synth_utterance(tab, 15 + k % 26, 1000 + k) for k in range(63)]
    o = J.melspec(n_fft=1200, hop=480, log="log10", range=8.0, offset=4.0, scale=0.25)
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_melspec(o)
            b.run()
            res.append(b.read_melspec(pos))
    assert np.array_equal(res[0], res[1])
    assert res[0].shape == (J.melspec_geometry(vi.sampling_frequency, o, 40 * vi.fperiod)[3], 80)


def test_engine_entries(eng):
    hz = eng.condition.get_sampling_frequency()
    o = J.melspec(n_fft=1200, hop=480, n_mels=40, log="db", range=80.0)
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    one = eng.synthesize_melspec(SAMPLE_SENTENCE_1, o)
    assert np.array_equal(one, J.melspec_pcm(pcm, hz, o)) and one.shape[1] == 40
    assert np.array_equal(eng.synthesize_melspec(SAMPLE_SENTENCE_1, n_fft=1200, hop=480, n_mels=40, log="db",
                                                 range=80.0), one)
    e16 = eng.clone()
    e16.condition.set_output_sampling_frequency(16000)
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    w = J.whisper_mel(80)
    for got, x in zip(e16.synthesize_melspec_batch(sents, w), e16.synthesize_batch(sents)):
        assert got.shape == (x.size // 160, 80) and np.array_equal(got, J.melspec_pcm(x, 16000, w))
    prog, starts = eng.synthesize_programme(sents, sink="f64", gap_ms=120.0, fade_ms=2.0)
    feat, starts2 = eng.synthesize_programme(sents, sink="melspec", gap_ms=120.0, fade_ms=2.0, opts=o)
    assert starts == starts2 and np.array_equal(feat, J.melspec_pcm(prog, hz, o))
    with pytest.raises(J.JbError, match="n_mels"):
        eng.synthesize_melspec(SAMPLE_SENTENCE_1, n_fft=400, hop=160, n_mels=200)
    # the _each entry: each utterance at its engine's output rate
    L = J.lib()
    from jbonsai_amd.engine import _byte_outs, _utt_lines
    from jbonsai_amd import _ffi as F
    lines, offs, B = _utt_lines(sents)
    bufs, ns, nf = _byte_outs(B, counts=True)
    hs = (C.c_void_p * B)(eng._h, e16._h)
    o4 = J.melspec(n_fft=400, hop=160, n_mels=40)
    F.check(L.jb_synthesize_batch_each_melspec(hs, lines, offs, B, -1, C.byref(o4), bufs, ns, nf))
    out = F.take_melspec(L, bufs, ns, B, o4)
    for got, x, r, T in zip(out, J.synthesize_batch_each([eng, e16], sents), (hz, 16000), nf):
        assert got.shape[0] == T and np.array_equal(got, J.melspec_pcm(x, r, o4))


def test_rules(eng):
    vi, utts = _utts(eng, (30,), 1)
    L = J.lib()
    UNSUPPORTED = -2
    o = J.melspec(n_fft=1200, hop=480)
    with J.Batch(vi, utts, mlpg_only=True) as b:
        assert L.jb_batch_set_melspec(b._h, C.byref(o)) == UNSUPPORTED and b"no PCM" in L.jb_last_error()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        assert L.jb_batch_set_melspec(b._h, C.byref(o)) == UNSUPPORTED and b"JB_BATCH_PCM_I16" in L.jb_last_error()
    with J.Batch(vi, utts) as b:  # without a call: nothing to read
        b.run()
        with pytest.raises(J.JbError, match="was not called"):
            b.melspec_size(0)
        assert L.jb_batch_read_melspec_all(b._h, None) == -1
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="n_mels"):
            b.set_melspec(n_fft=1200, hop=480, n_mels=0)
        with pytest.raises(J.JbError, match="n_fft"):
            b.set_melspec(n_fft=1202, hop=480)
        with pytest.raises(J.JbError, match="f_max_hz"):
            b.set_melspec(n_fft=1200, hop=480, f_max=30000.0)  # above half the voice's 48 kHz
        b.set_melspec(n_fft=1200, hop=480, f_max=12000.0)
        with pytest.raises(J.JbError, match="f_max_hz"):
            b.set_output_rate(16000)  # the combined request: 12 kHz is above half of 16 kHz
        b.set_melspec(None)  # withdrawn
        with pytest.raises(J.JbError, match="was not called"):
            b.melspec_size(0)
        b.set_melspec(o)
        n = 30 * vi.fperiod
        T = J.melspec_geometry(vi.sampling_frequency, o, n)[3]
        assert b.melspec_shape(0) == (T, 80, vi.sampling_frequency) and b.melspec_size(0) == T * 80 * 4
        with pytest.raises(J.JbError, match="has not run"):
            b.read_melspec(0)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_melspec(o)
        nby = b.melspec_size(0)
        buf = np.zeros(nby, dtype=np.uint8)
        assert L.jb_batch_read_melspec(b._h, 0, buf.ctypes.data, nby - 1) == -8
        assert L.jb_batch_read_melspec(b._h, 0, None, nby) == -1
        assert L.jb_batch_read_melspec(b._h, 1, buf.ctypes.data, nby) == -1
        assert L.jb_batch_melspec_shape(b._h, 0, None, None, None) == 0
        assert L.jb_batch_read_melspec(b._h, 0, buf.ctypes.data, nby) == 0
        assert np.array_equal(np.frombuffer(buf.tobytes(), dtype=np.float32).reshape(T, 80),
                              J.melspec_pcm(b.pcm(0), vi.sampling_frequency, o))


ML = J.melspec(n_fft=1200, hop=480, n_mels=40, log="log10", range=8.0)
SINK = ("melspec", "jb_batch_set_melspec", False, lambda b: b.set_melspec(ML), ("melspec_size", "read_melspec"),
        lambda b, i: b.read_melspec(i), lambda b: b.read_melspec_all(), lambda hz, n: J.melspec_geometry(hz, ML, n)[4])


@pytest.mark.parametrize("joined", [False, True])
def test_size_and_read_entries_as_the_other_sinks(joined):
    """The cases tests/test_gpu_sink_reads.py exercises for the other five sinks, through its own check: before the set
    call, between it and the run, after it; short buffers, NULL destinations, indices past the end, an output of no
    samples (no frame under reflection), and the two utterances joined into one programme."""
    from tests import test_gpu_sink_reads as S

    eng = J.Engine.load([VOICE])
    vi, utts = eng.voice_info(), [eng.states(SAMPLE_SENTENCE_1), eng.states([])]
    with mock.patch.dict(S.SINKS, {"melspec": SINK}):
        with J.Batch(vi, utts, serial=True, serial_gv=True) as b:
            if joined:
                b.set_join([(0, 0, 0, 0, 0), (0, 0, 0, 0, 0)])
                samples = [b.programme_layout(0)[1]]
            else:
                samples = [b.num_samples(u) for u in range(len(b))]
                assert samples[0] > 0 and samples[1] == 0
            S.check_reads(b, "melspec", samples)
