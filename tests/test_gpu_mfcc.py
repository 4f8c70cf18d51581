"""Cepstral features on the device (jbonsai_amd/csrc/jb_mfcc.hip) against the host form of the same rule.

jb_mfcc_frames_batch equals jb_mfcc_host bit for bit wherever the device takes no square root (JB_CMVN_NONE and
JB_CMVN_MEAN, every order, f32 and f64); under JB_CMVN_MEAN_VAR it is held to the gate of tests/mfcc_ref.py.  The units
of a call have different lengths -- block edges of the statistics (63, 64, 65, 129), tile edges of the kernels (32),
units shorter than the 4 N + 1 delta-delta kernel, a unit of no frame -- so that workgroups end at unit ends.

Then the stage in a batch (jb_batch_set_mfcc) -- equal to the PCM seam on the batch's own final PCM bit for bit: plain,
behind the converter and the loudness target, beside a plain fbank request and a sample format, behind a join (CMVN
over the programme), through redo rounds, in the fast invariant mode -- the engine entries and the setter's rules."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import fbank_ref
from tests import mfcc_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 300)
SHAPES = ((1, 1), (23, 13), (80, 80), (128, 40), (128, 0))
WINDOWS = (1, 2, 5)


def units_of(n_mels):
    """A unit per length: the short ones from the live part of the shared frames, the long ones from their start (the
    silent frames at the floor included)."""
    L = R.logmel(n_mels)
    return [np.ascontiguousarray(L[8:8 + T] if T < 63 else L[:T]) for T in LENGTHS]


@pytest.mark.parametrize("n_mels,n_ceps", SHAPES)
def test_frames_seam_equals_the_host_rule_bit_for_bit(n_mels, n_ceps):
    units = units_of(n_mels)
    for cmvn in ("none", "mean"):
        for order, windows in ((0, (2,)), (1, WINDOWS), (2, WINDOWS)):
            for N in windows:
                for f64 in (False, True):
                    o = J.mfcc(n_ceps=n_ceps, delta_order=order, delta_window=N, cmvn=cmvn, f64=f64)
                    got = J.mfcc_frames(units, o)
                    assert len(got) == len(units)
                    for T, L, y in zip(LENGTHS, units, got):
                        want = J.mfcc_host(L, o)
                        assert y.dtype == want.dtype and y.shape == want.shape == (T, o.width(n_mels))
                        assert np.array_equal(y, want), (cmvn, order, N, f64, T)
    # one unit alone gives the bits it has among the others
    o = J.mfcc(n_ceps=n_ceps, delta_order=2, cmvn="mean", f64=True)
    assert np.array_equal(J.mfcc_frames(units[9], o), J.mfcc_frames(units, o)[9])


@pytest.mark.parametrize("n_mels,n_ceps", SHAPES)
def test_frames_seam_under_the_gate_with_variance(n_mels, n_ceps):
    """Every unit of two frames or more is gated on its own, e(unit) <= 8 e(model_f64 of that unit), except with one
    filter alone, where the gate is taken over the call: e = max over the units of the call on both sides.  A unit of
    one column has one mean and one variance, and numpy.mean sums its <= 65 near-equal values pairwise, far more
    exactly than any sequential order can: e(model_f64) of such a unit goes down to 7e-18 (and to 2e-20 where all
    frames are equal), while the rule's own order -- blocks of 64 from 0.0, which the device follows bit for bit -- errs
    by 1 to 4e-16, one or two ulps of the bound.  Measured per unit with one filter: ratios up to 9.4 (T = 65; up to 24
    on other stretches of the same signal); over the call 2.0 to 2.8.  With more than one column the maximum over the
    columns meets an ordinary one and the per-unit gate holds as stated (largest ratio 6.1, n_mels 128, T = 3)."""
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    units = units_of(n_mels)
    worst = 0.0
    for order, N in ((0, 2), (2, 1), (2, 2), (2, 5)):
        kw = dict(n_ceps=n_ceps, delta_order=order, delta_window=N, cmvn="mean_var")
        got = J.mfcc_frames(units, J.mfcc(f64=True, **kw))
        got32 = J.mfcc_frames(units, J.mfcc(**kw))
        call_e = call_e64 = 0.0
        for T, L, y, y32 in zip(LENGTHS, units, got, got32):
            assert y.dtype == np.float64 and y.shape == (T, (n_ceps or n_mels) * (order + 1)) and np.all(np.isfinite(y))
            assert y32.dtype == np.float32 and np.array_equal(y32, y.astype(np.float32))
            if T == 1:
                assert np.all(y == 0.0)
            if T >= 2:
                e, e64 = R.errors(y, L, **kw)
                print(f"device T {T} n_mels {n_mels} {kw}: e(model_f64) {e64:.2e}  e {e:.2e}  "
                      f"ratio {e / e64 if e64 else 0:.2f}")
                call_e, call_e64 = max(call_e, e), max(call_e64, e64)
                if n_mels > 1:
                    assert 0 < e64 < 1e-14 and e <= R.GATE * e64, (T, order, N)
                    worst = max(worst, e / e64)
        assert 0 < call_e64 < 1e-14 and call_e <= R.GATE * call_e64, (order, N)
        worst = max(worst, call_e / call_e64) if n_mels == 1 else worst
    print(f"n_mels {n_mels} n_ceps {n_ceps}: worst ratio {worst:.2f}")
    # an explicit floor above every variance: the division is by its root alone
    y = J.mfcc_frames(units[8], J.mfcc(n_ceps=n_ceps, cmvn="mean_var", var_floor=1e12, f64=True))
    mean = J.mfcc_host(units[8], J.mfcc(n_ceps=n_ceps, cmvn="mean", f64=True))
    assert np.array_equal(y, mean / 1e6)


def test_pcm_seam_is_the_frames_seam_behind_the_filterbank():
    """Rates 8000, 16000 and 48000 in one call; a unit too short for a frame among them."""
    pcms, rates = [], (8000, 16000, 48000, 16000, 8000)
    for k, hz in enumerate(rates):
        wl, hop, _ = fbank_ref.geometry(hz)
        n = wl - 1 if k == 3 else (40 + 30 * k) * hop + wl + k
        pcms.append(fbank_ref.gate_signal(hz, n, seed=20 + k))
    for fkw in (dict(n_mels=80), dict(n_mels=23, center=True, unit=True, window="hamming")):
        logmels = J.fbank_pcm(pcms, rates, J.fbank(f64=True, **fkw))
        assert "center" in fkw or logmels[3].shape[0] == 0
        for o in (J.mfcc(delta_order=2, cmvn="mean_var"), J.mfcc(n_ceps=0, delta_order=1, cmvn="mean", f64=True),
                  J.mfcc(n_ceps=13, lifter=0, f64=True)):
            got = J.mfcc_pcm(pcms, rates, J.fbank(**fkw), o)
            want = J.mfcc_frames(logmels, o)
            for y, w, L in zip(got, want, logmels):
                assert y.dtype == w.dtype and y.shape == w.shape == (L.shape[0], o.width(L.shape[1]))
                assert np.array_equal(y, w)
    # one array, one rate
    o = J.mfcc(delta_order=1, cmvn="mean")
    y = J.mfcc_pcm(pcms[1], 16000, J.fbank(), o)
    assert np.array_equal(y, J.mfcc_frames(J.fbank_pcm(pcms[1], 16000, J.fbank(f64=True)), o))
    # and the whole rule on the host agrees with it to the filterbank's own precision (the logarithm is each side's)
    yh = J.mfcc_pcm_host(pcms[1], 16000, J.fbank(), J.mfcc(f64=True))
    yd = J.mfcc_pcm(pcms[1], 16000, J.fbank(), J.mfcc(f64=True))
    assert yh.shape == yd.shape and np.allclose(yh, yd, rtol=0, atol=1e-9)


def test_a_unit_alone_and_among_64_gives_identical_bytes():
    L = R.logmel(80)
    rng = np.random.default_rng(22)
    others = [np.ascontiguousarray(L[a:a + n]) for a, n in zip(rng.integers(0, 100, 63), rng.integers(1, 200, 63))]
    unit = np.ascontiguousarray(L[:171])
    for o in (J.mfcc(delta_order=2, cmvn="mean_var"), J.mfcc(n_ceps=0, delta_order=2, cmvn="mean_var", f64=True)):
        alone = J.mfcc_frames(unit, o)
        for place in (0, 31, 63):
            among = J.mfcc_frames(others[:place] + [unit] + others[place:], o)
            assert among[place].tobytes() == alone.tobytes()


def test_no_unit_and_empty_units():
    assert J.mfcc_frames([], J.mfcc(n_ceps=1)) == []
    got = J.mfcc_frames([np.zeros((0, 23)), np.zeros((0, 23))], J.mfcc(delta_order=2, cmvn="mean_var"))
    assert [g.shape for g in got] == [(0, 39), (0, 39)]


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (9, 40, 23)
FULL = dict(delta_order=2, cmvn="mean_var")


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 5)


def check_batch(b, fo, o):
    """read_mfcc(i) == read_mfcc_all()[i] == the PCM seam on the PCM of the same batch, bit for bit."""
    every = b.read_mfcc_all()
    assert len(every) == len(b)
    for i in range(len(b)):
        x, hz = b.pcm(i), b.output_rate(i)
        T, w, rate = b.mfcc_shape(i)
        assert (T, w, rate) == (*J.mfcc_geometry(hz, fo, o, x.size)[:2], hz) and w == o.width(fo.n_mels)
        assert every[i].shape == (T, w) and every[i].dtype == o.dtype and b.mfcc_size(i) == every[i].nbytes
        assert np.array_equal(b.read_mfcc(i), every[i])
        assert np.array_equal(every[i], J.mfcc_pcm(x, hz, fo, o)), i
    return every


@pytest.mark.parametrize("fkw,kw", [(dict(), FULL), (dict(center=True, window="hamming", n_mels=40),
                                                     dict(n_ceps=0, delta_order=1, delta_window=5, cmvn="mean", f64=True)),
                                    (dict(n_mels=128), dict(n_ceps=128, delta_order=2, lifter=0))])
def test_batch_path_equals_the_seam(eng, batch_utts, fkw, kw):
    vi, utts = batch_utts
    fo, o = J.fbank(**fkw), J.mfcc(**kw)
    with J.Batch(vi, utts) as b:
        b.set_mfcc(o, fbank=fo)
        b.run()
        check_batch(b, fo, o)
    with J.Batch(vi, utts) as b:  # behind the converter and the loudness target
        b.set_output_rate(16000)
        b.set_loudness_target(-23.0)
        b.set_mfcc(o, fbank=fo)
        b.run()
        assert b.output_rate(0) == 16000
        check_batch(b, fo, o)


def test_beside_a_plain_fbank_request_and_a_sample_format(eng, batch_utts):
    vi, utts = batch_utts
    plain_fb = J.fbank(n_mels=64)
    with J.Batch(vi, utts) as b:
        b.set_format("s16")
        b.set_fbank(plain_fb)
        b.run()
        before = ([b.pcm(i).tobytes() for i in range(len(utts))], [b.formatted(i) for i in range(len(utts))],
                  [f.tobytes() for f in b.read_fbank_all()], b.info())
    fo, o = J.fbank(n_mels=40, center=True), J.mfcc(**FULL)
    with J.Batch(vi, utts) as b:
        b.set_format("s16")
        b.set_fbank(plain_fb)
        b.set_mfcc(o, fbank=fo)
        b.run()
        check_batch(b, fo, o)
        after = ([b.pcm(i).tobytes() for i in range(len(utts))], [b.formatted(i) for i in range(len(utts))],
                 [f.tobytes() for f in b.read_fbank_all()], b.info())
        assert after == before  # the request changed no byte of the others, and none of the vocoder's work items
        assert b.read_fbank(0).shape[1] == 64


def test_join_features_of_the_programme(eng, batch_utts):
    vi, utts = batch_utts
    fo, o = J.fbank(center=True), J.mfcc(**FULL)
    with J.Batch(vi, utts) as b:
        req = [(0, 100, 333, 16, 16), (None, 0, 0, 0, 0), (0, 7, 2001, 0, 24)]
        b.set_join(req)
        b.set_mfcc(o, fbank=fo)
        b.run()
        assert b.num_outputs() == 2
        every = b.read_mfcc_all()
        hz = vi.sampling_frequency
        joined = J.join_pcm([b.pcm(i) for i in range(len(utts))], req)  # jb_join_pcm_batch's programmes
        assert len(joined) == 2
        for p in range(2):
            assert np.array_equal(every[p], J.mfcc_pcm(joined[p], hz, fo, o))
        for p in range(2):
            x = b.programme_pcm(p)
            assert b.mfcc_shape(p) == (*J.mfcc_geometry(hz, fo, o, x.size)[:2], hz)
            # the seam on the joined programme: the CMVN runs over the whole programme
            assert np.array_equal(every[p], J.mfcc_pcm(x, hz, fo, o)) and np.array_equal(b.read_mfcc(p), every[p])
            assert every[p].shape[0] > 0
        with pytest.raises(J.JbError):
            b.mfcc_shape(2)


def test_redo_rounds_see_the_final_pcm(eng):
    """Redo rounds forced the way tests/test_gpu_fbank.py forces them: the rows are the seam's on the final PCM, every
    frame of every touched unit, those in front of the first redone chunk included; MEAN_VAR is on, so that a mean or
    a variance left from the first pass would show in every row."""
    vi, utts = _utts(eng, (600, 1100), 40)
    fo, o = J.fbank(), J.mfcc(f64=True, **FULL)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_mfcc(o, fbank=fo)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        check_batch(b, fo, o)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target([-20.0, -26.0], float("inf"))
        b.set_join([(0, 0, 480, 0, 0), (0, 0, 0, 0, 0)])
        b.set_mfcc(o, fbank=fo)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        x = b.programme_pcm(0)
        assert np.array_equal(b.read_mfcc(0), J.mfcc_pcm(x, vi.sampling_frequency, fo, o))


def test_invariance_alone_and_among_64_in_a_batch(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 300, 77)
    others = [synth.synth_utterance(tab, 50 + 13 * k, 1000 + k) for k in range(63)]
    fo, o = J.fbank(), J.mfcc(**FULL)
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_mfcc(o, fbank=fo)
            b.run()
            res.append(b.read_mfcc(pos))
    assert res[0].tobytes() == res[1].tobytes()
    assert res[0].shape == (J.mfcc_geometry(vi.sampling_frequency, fo, o, 300 * vi.fperiod)[0], 39)


def test_engine_entries(eng):
    hz = eng.condition.get_sampling_frequency()
    fo, o = J.fbank(n_mels=40, center=True), J.mfcc(**FULL)
    pcm = eng.synthesize(SAMPLE_SENTENCE_1)
    one = eng.synthesize_mfcc(SAMPLE_SENTENCE_1, o, fbank=fo)
    assert np.array_equal(one, J.mfcc_pcm(pcm, hz, fo, o)) and one.shape[1] == 39
    assert np.array_equal(eng.synthesize_mfcc(SAMPLE_SENTENCE_1, fbank=dict(n_mels=40, center=True), **FULL), one)
    e16 = eng.clone()
    e16.condition.set_output_sampling_frequency(16000)
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    for got, x in zip(e16.synthesize_mfcc_batch(sents, o, fbank=fo), e16.synthesize_batch(sents)):
        assert np.array_equal(got, J.mfcc_pcm(x, 16000, fo, o))
    prog, starts = eng.synthesize_programme(sents, sink="f64", gap_ms=120.0, fade_ms=2.0)
    feat, starts2 = eng.synthesize_programme(sents, sink="mfcc", gap_ms=120.0, fade_ms=2.0, opts=o, fbank=fo)
    assert starts == starts2 and np.array_equal(feat, J.mfcc_pcm(prog, hz, fo, o))
    # jb_synthesize_batch_each_mfcc: each utterance at its engine's rate
    L = J.lib()
    u8p = C.POINTER(C.c_uint8)
    flat = [l.encode() for u in sents for l in u]
    lines = (C.c_char_p * len(flat))(*flat)
    offs = (C.c_size_t * 3)(0, len(sents[0]), len(flat))
    hs = (C.c_void_p * 2)(eng._h, e16._h)
    bufs, ns, nf = (u8p * 2)(), (C.c_size_t * 2)(), (C.c_size_t * 2)()
    assert L.jb_synthesize_batch_each_mfcc(hs, lines, offs, 2, -1, C.byref(fo), C.byref(o), bufs, ns, nf) == 0
    from jbonsai_amd import _ffi

    out = _ffi.take_mfcc(L, bufs, ns, 2, o, 40)
    for got, x, r, frames in zip(out, J.synthesize_batch_each([eng, e16], sents), (hz, 16000), nf):
        assert np.array_equal(got, J.mfcc_pcm(x, r, fo, o)) and got.shape[0] == frames
    with pytest.raises(J.JbError, match="n_ceps"):
        eng.synthesize_mfcc(SAMPLE_SENTENCE_1, n_ceps=81)
    with pytest.raises(J.JbError, match="flags"):
        eng.synthesize_mfcc(SAMPLE_SENTENCE_1, fbank=dict(f64=True))


def test_rules(eng):
    vi, utts = _utts(eng, (30,), 1)
    L = J.lib()
    UNSUPPORTED = -2
    fo, o = J.fbank(), J.mfcc(**FULL)
    with J.Batch(vi, utts, mlpg_only=True) as b:
        assert L.jb_batch_set_mfcc(b._h, C.byref(fo), C.byref(o)) == UNSUPPORTED and b"no PCM" in L.jb_last_error()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        assert L.jb_batch_set_mfcc(b._h, C.byref(fo), C.byref(o)) == UNSUPPORTED
        assert b"JB_BATCH_PCM_I16" in L.jb_last_error()
    with J.Batch(vi, utts) as b:  # without a call: nothing to read
        b.run()
        with pytest.raises(J.JbError, match="was not called"):
            b.mfcc_size(0)
        assert L.jb_batch_read_mfcc_all(b._h, None) == -1
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="n_ceps"):
            b.set_mfcc(n_ceps=81)
        with pytest.raises(J.JbError, match="delta_window"):
            b.set_mfcc(delta_window=0)
        with pytest.raises(J.JbError, match="flags"):
            b.set_mfcc(o, fbank=dict(linear=True))
        with pytest.raises(J.JbError, match="win_us"):
            b.set_mfcc(o, fbank=dict(win_ms=100))  # 4800 samples at the voice's 48 kHz
        assert L.jb_batch_set_mfcc(b._h, C.byref(fo), None) == -1 and L.jb_batch_set_mfcc(b._h, None, C.byref(o)) == -1
        b.set_mfcc(o, fbank=dict(win_ms=50))
        with pytest.raises(J.JbError, match="win_us"):
            b.set_output_rate(192000)  # the combined request, a rate the geometry refuses: 9600 samples there
        b.set_mfcc(None)  # withdrawn
        with pytest.raises(J.JbError, match="was not called"):
            b.mfcc_size(0)
        b.set_mfcc(o, fbank=fo)
        n = 30 * vi.fperiod
        T = J.mfcc_geometry(vi.sampling_frequency, fo, o, n)[0]
        assert b.mfcc_shape(0) == (T, 39, vi.sampling_frequency) and b.mfcc_size(0) == T * 39 * 4
        with pytest.raises(J.JbError, match="has not run"):
            b.read_mfcc(0)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_mfcc(o, fbank=fo)
        nby = b.mfcc_size(0)
        buf = np.zeros(nby, dtype=np.uint8)
        assert L.jb_batch_read_mfcc(b._h, 0, buf.ctypes.data, nby - 1) == -8
        assert L.jb_batch_read_mfcc(b._h, 0, None, nby) == -1
        assert L.jb_batch_read_mfcc(b._h, 1, buf.ctypes.data, nby) == -1
        assert L.jb_batch_mfcc_shape(b._h, 0, None, None, None) == 0
        assert L.jb_batch_read_mfcc(b._h, 0, buf.ctypes.data, nby) == 0
        assert np.array_equal(np.frombuffer(buf.tobytes(), dtype=np.float32).reshape(T, 39),
                              J.mfcc_pcm(b.pcm(0), vi.sampling_frequency, fo, o))
