"""Frame conditioning on the GPU (the conditioned loader of k_fbank, jb_fbank.hip; the energy column of k_ceps,
jb_mfcc.hip): the device seam under the precision gate of tests/frame_ref.py (at most GATE times the error of a float64
numpy model, both against a long double model) at the smallest shapes that reach every frame-to-lane layout -- a wave
a frame up to n_fft 1024, two at 2048, four at 4096, where the mean and the energy cross waves -- with units of no
frame, of one, and of one more than a multiple of the frames a workgroup takes; the exact silence of a constant signal;
reflected units shorter than a window; then the request in a batch and behind the engine, equal to the seam bit for
bit: alone and beside other units, behind a forced redo round, in the fast invariant mode, behind a join; the frame's
log energy as c0 within the device logarithm's 1 ulp (plus half an ulp for the reference's own rounding) on frames
whose energy is an exact integer; and the rules of jb_batch_set_frame_opts.

The gate ratios this file prints (-s) are the measured ones; the largest is quoted in the README."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import fbank_ref as R
from tests import frame_ref as FR
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu
LD = np.longdouble
needs_ld = pytest.mark.skipif(not R.have_long_double(), reason="numpy.longdouble has no 64-bit mantissa here")


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


# (hz, win_ms, hop_ms, n_fft, n_mels, window): wl 2 and 64 in n_fft 64, 400 in 512, 551 (odd) in 1024, 1200 in 2048 (two
# waves a frame), 4096 in 4096 (four).  wl = 2 has no tapered symmetric window but zeros: the rectangular one
LAYOUTS = [(16000, 0.125, 0.0625, 64, 10, FR.RECT), (16000, 4, 2, 64, 10, FR.POVEY), (16000, 25, 10, 0, 80, FR.POVEY),
           (22050, 25, 10, 0, 128, FR.BLACKMAN), (48000, 25, 10, 0, 80, FR.POVEY), (16000, 256, 10, 0, 40, FR.HANN_SYM)]


def close_to_host(got, x, hz, f, fr):
    """Against the host form of the same rule: equal shape, and equal values to a few ulp of the frame's power -- the
    precise comparison is the gate; this one catches a misplaced frame."""
    want = J.fbank_framed_host(x, hz, f, fr)
    assert got.shape == want.shape and got.dtype == want.dtype
    if want.size:
        scale = np.abs(want).max(axis=1, keepdims=True)
        assert np.all(np.abs(got - want) <= 1e-13 * scale), (x.size, hz)


@needs_ld
@pytest.mark.parametrize("hz,win_ms,hop_ms,n_fft,n_mels,window", LAYOUTS)
@pytest.mark.parametrize("reflect", [False, True])
def test_seam_under_the_gate(eng, hz, win_ms, hop_ms, n_fft, n_mels, window, reflect):
    """DC removal and 0.97 pre-emphasis on a signal with a DC offset of 3000, one call of three units: T = 0, T = 1 and
    T one more than a multiple of the workgroup's frames (the gated one)."""
    win_us, hop_us = int(round(1000 * win_ms)), int(round(1000 * hop_ms))
    wl, hop, nf = R.geometry(hz, win_us, hop_us, n_fft)
    per = 4 if nf <= 1024 else 2 if nf == 2048 else 1
    T = 4 * per + 1 if per > 1 else 11
    n = T * hop - hop // 2 if reflect else wl + (T - 1) * hop
    x = FR.gate_signal(hz, n, hop, offset=3000.0)
    xs = [x[:0] if reflect else x[-(wl - 1):], x[-hop:] if reflect else x[-wl:], x]
    kw = dict(window=window, reflect=reflect, preemph=0.97, remove_dc=True, n_fft=n_fft, win_us=win_us, hop_us=hop_us)
    got = {}

    def run(x_, f, fr):
        got["all"] = J.fbank_framed_pcm(xs, hz, f, fr)
        got["opts"] = (f, fr)
        return got["all"][2]

    FR.check_gate(run, x, hz, n_mels, "device", **kw)
    f, fr = got["opts"]
    assert [g.shape[0] for g in got["all"]] == [0, 1, T]
    assert [J.fbank_framed_geometry(hz, f, fr, a.size)[3] for a in xs] == [0, 1, T]
    for a, g in zip(xs, got["all"]):
        close_to_host(g, a, hz, f, fr)
    # deterministic: the gated unit alone gives the bytes it gave as the third of three
    assert np.array_equal(J.fbank_framed_pcm(x, hz, f, fr), got["all"][2])


@needs_ld
@pytest.mark.parametrize("kw", [dict(preemph=1.0), dict(preemph=0.0, remove_dc=True), dict(preemph=0.97),
                                dict(preemph=0.97, remove_dc=True, center=True, fbank_window=R.HAMMING,
                                     window=FR.WINDOW_OPTS)])
def test_seam_under_the_gate_by_step(eng, kw):
    """Each step alone at 48 kHz (two waves a frame), and the padded zeros of centre mode under DC removal."""
    hz, (wl, hop, _) = 48000, R.geometry(48000)
    x = FR.gate_signal(hz, 10 * hop + wl + 3, hop, offset=3000.0)
    kw = dict(dict(window=FR.POVEY, remove_dc=False), **kw)
    FR.check_gate(lambda x_, f, fr: J.fbank_framed_pcm(x_, hz, f, fr), x, hz, 80, "device", **kw)


@pytest.mark.parametrize("hz,win_ms", [(16000, 25), (48000, 25), (16000, 256)])
def test_exact_silence_of_a_constant_signal(eng, hz, win_ms):
    """An integer-valued constant: DC removal (the mean is a division) and preemph = 1.0 each leave exact zeros, with
    the mean folded across one, two and four waves."""
    x = np.full(3 * int(hz * win_ms / 1000), 1234.0)
    f = J.fbank(win_ms=win_ms, linear=True, f64=True)
    for fr in (J.frame(window="rect", remove_dc=True), J.frame(preemph=1.0), J.frame(preemph=1.0, window="povey"),
               J.frame(window="rect", remove_dc=True, reflect=True), J.frame(preemph=1.0, reflect=True)):
        E = J.fbank_framed_pcm(x, hz, f, fr)
        assert E.shape[0] >= 3 and np.all(E == 0.0)
    ln_floor = float(np.log(LD(2.0 ** -52)))
    y = J.fbank_framed_pcm(x, hz, J.fbank(win_ms=win_ms, f64=True), J.frame(window="rect", remove_dc=True))
    assert np.all(y == ln_floor)


@needs_ld
@pytest.mark.parametrize("n", [80, 81])
def test_reflected_units_shorter_than_a_window(eng, n):
    """n = 80 and 81 at 16 kHz (wl 400, hop 160): one frame, mirrored more than once."""
    hz = 16000
    x = np.random.default_rng(n).normal(0.0, 3000.0, n) + 500.0
    kw = dict(window=FR.POVEY, reflect=True, preemph=0.97, remove_dc=True)
    seen = {}

    def run(x_, f, fr):
        seen["o"] = (f, fr)
        return J.fbank_framed_pcm(x_, hz, f, fr)

    FR.check_gate(run, x, hz, 80, "device", **kw)
    f, fr = seen["o"]
    got = J.fbank_framed_pcm(x, hz, f, fr)
    assert got.shape == (1, 80)
    close_to_host(got, x, hz, f, fr)


def test_the_zero_request_gives_the_plain_seams_bytes(eng):
    rng = np.random.default_rng(9)
    xs = [rng.normal(0, 3000, n) for n in (1001, 4801, 0, 2207)]
    rates = [8000, 48000, 16000, 22050]
    for o in (J.fbank(), J.fbank(n_mels=23, center=True, window="hamming", f64=True)):
        for a, b in zip(J.fbank_framed_pcm(xs, rates, o, J.frame()), J.fbank_pcm(xs, rates, o)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    fo, mo = J.fbank(n_mels=40), J.mfcc(delta_order=2, cmvn="mean_var")
    for a, b in zip(J.mfcc_framed_pcm(xs, rates, fo, mo, J.frame()), J.mfcc_pcm(xs, rates, fo, mo)):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(J.JbError, match="flags"):
        J.fbank_framed_pcm(xs, rates, J.fbank(), J.frame(energy=True))
    with pytest.raises(J.JbError, match="flags"):
        J.fbank_framed_pcm(xs, rates, J.fbank(center=True), J.frame(reflect=True))
    with pytest.raises(J.JbError, match="preemph"):
        J.mfcc_framed_pcm(xs, rates, fo, mo, J.frame(preemph=2.0))


@pytest.mark.parametrize("reflect", [False, True])
def test_seam_rates_and_workgroup_edges_in_one_call(eng, reflect):
    """What the pass builder numbers (class, T, g0, the workgroup count), as tests/test_gpu_fbank.py's
    test_seam_rates_in_one_call_and_the_f32_rows has it for the plain seam: eight units at 16 and 48 kHz interleaved,
    n_fft 512 (four frames to a workgroup), of 0, 1, wl - 1, wl, wl + 4 hop (five frames: one past a workgroup) and
    wl + 3 hop (exactly one workgroup) samples -- the last two at both rates.  Each unit of the one call has the bytes
    of its own call, for the filterbank and for the cepstra with the frames' energies."""
    rng = np.random.default_rng(512)
    f = J.fbank(win_ms=10, hop_ms=5, n_fft=512, n_mels=23)
    rates = [16000, 48000] * 4
    xs = []
    for u, hz in enumerate(rates):
        wl, hop, nf = R.geometry(hz, 10000, 5000, 512)
        assert nf == 512
        n = (0, 1, wl - 1, wl, wl + 4 * hop, wl + 3 * hop, wl + 3 * hop, wl + 4 * hop)[u]
        xs.append(rng.normal(0, 3000, n) + 500.0)
    fr = J.frame(preemph=0.97, window="povey", remove_dc=True, reflect=reflect)
    fre, mo = J.frame(preemph=0.97, window="povey", remove_dc=True, reflect=reflect, energy=True), J.mfcc()
    got, gotm = J.fbank_framed_pcm(xs, rates, f, fr), J.mfcc_framed_pcm(xs, rates, f, mo, fre)
    if not reflect:
        assert [g.shape[0] for g in got] == [0, 0, 0, 1, 5, 4, 4, 5]
    for x, hz, g, gm in zip(xs, rates, got, gotm):
        assert g.shape == (J.fbank_framed_geometry(hz, f, fr, x.size)[3], 23) and gm.shape == (g.shape[0], 13)
        assert g.tobytes() == J.fbank_framed_pcm(x, hz, f, fr).tobytes()
        assert gm.tobytes() == J.mfcc_framed_pcm(x, hz, f, mo, fre).tobytes()


@needs_ld
@pytest.mark.parametrize("hz", [16000, 48000])
def test_energy_replaces_c0(eng, hz):
    """Integer samples, no DC removal: e is an exact integer.  c0 = ln(max(e, floor)) within the device logarithm's
    1 ulp plus half an ulp for the reference's rounding; the other cepstra are those of the request without the flag;
    CMVN and the deltas of c0 are jb_mfcc_frames_batch's on the same statics, bit for bit."""
    wl, hop, _ = R.geometry(hz)
    rng = np.random.default_rng(hz)
    xs = [rng.integers(-3000, 3001, n).astype(np.float64) for n in (37 * hop + wl, wl, wl - 1, 70 * hop + wl + 5)]
    xs[0][:wl + hop] = 0.0  # two silent frames: the floor
    f = J.fbank(n_mels=40, log_floor=1e-3)
    m = J.mfcc(n_ceps=13, f64=True)
    for fr_kw in (dict(), dict(preemph=0.97, window="povey"), dict(reflect=True)):
        with_e = J.mfcc_framed_pcm(xs, hz, f, m, J.frame(energy=True, **fr_kw))
        without = J.mfcc_framed_pcm(xs, hz, f, m, J.frame(**fr_kw))
        for x, a, b in zip(xs, with_e, without):
            assert a.shape == b.shape and np.array_equal(a[:, 1:], b[:, 1:])
            _, _, e = FR.model_ld(x, hz, 1, reflect=fr_kw.get("reflect", False))
            assert e.shape == (a.shape[0],) and np.all(e == np.round(e))
            silent = e == 0
            assert np.all(a[silent, 0] == float(np.log(LD(1e-3))))
            ref = np.log(e[~silent])
            ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
            assert np.all(np.abs(a[~silent, 0].astype(LD) - ref) <= LD("1.5") * ulp)
        assert (with_e[0][:2, 0] == float(np.log(LD(1e-3)))).all() or fr_kw.get("reflect")
    # CMVN and the deltas run on the statics with the energy in place
    statics = J.mfcc_framed_pcm(xs, hz, f, m, J.frame(energy=True))
    for cmvn in ("none", "mean"):
        md = J.mfcc(n_ceps=13, f64=True, delta_order=2, cmvn=cmvn)
        full = J.mfcc_framed_pcm(xs, hz, f, md, J.frame(energy=True))
        behind = J.mfcc_frames(statics, J.mfcc(n_ceps=0, f64=True, delta_order=2, cmvn=cmvn))
        for a, b in zip(full, behind):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), cmvn
    # against the host form: c0 to the two logarithms' ulps, the rest as the stage has it
    host = J.mfcc_framed_pcm_host(xs[3], hz, f, m, J.frame(energy=True))
    assert np.all(np.abs(host[:, 0] - statics[3][:, 0]) <= 2 * np.spacing(np.abs(host[:, 0])))


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, t, seed + t) for t in frames]


FRAMES = (9, 40, 23)


@pytest.fixture(scope="module")
def batch_utts(eng):
    return _utts(eng, FRAMES, 5)


def check_batch(b, o, fr):
    """read_fbank(i) == read_fbank_all()[i] == the framed seam on the PCM of the same batch, bit for bit."""
    every = b.read_fbank_all()
    assert len(every) == len(b)
    for i in range(len(b)):
        x, hz = b.pcm(i), b.output_rate(i)
        T, m, rate = b.fbank_shape(i)
        assert (m, rate) == (o.n_mels, hz) and T == J.fbank_framed_geometry(hz, o, fr, x.size)[3]
        assert every[i].shape == (T, m) and b.fbank_size(i) == every[i].nbytes
        assert np.array_equal(b.read_fbank(i), every[i])
        assert np.array_equal(every[i], J.fbank_framed_pcm(x, hz, o, fr)), i
    return every


def kaldi(n_mels=23, **kw):
    f, fr = J.kaldi_frame(n_mels)
    for k, v in kw.items():
        setattr(fr, k, v)
    return f, fr


def test_batch_path_equals_the_seam(eng, batch_utts):
    vi, utts = batch_utts
    o, fr = kaldi()
    with J.Batch(vi, utts) as b:  # the request first
        b.set_frame(fr)
        b.set_fbank(o)
        b.run()
        beside = check_batch(b, o, fr)
        plain = J.fbank_pcm(b.pcm(1), b.output_rate(1), o)
        assert beside[1].shape == plain.shape and not np.array_equal(beside[1], plain)  # (the request was read)
    with J.Batch(vi, utts[1:2]) as b:  # a unit alone gives the bytes it gave beside the others
        b.set_fbank(o)
        b.set_frame(fr)
        b.run()
        assert np.array_equal(b.read_fbank(0), beside[1])
    o, fr = kaldi(80, flags=J.FRAME_REMOVE_DC | J.FRAME_REFLECT)
    with J.Batch(vi, utts) as b:  # reflected T, behind the converter and the loudness target
        b.set_output_rate(16000)
        b.set_loudness_target(-23.0)
        b.set_fbank(o)
        b.set_frame(fr)
        b.run()
        every = check_batch(b, o, fr)
        assert every[0].shape[0] == (b.pcm(0).size + 80) // 160
    with J.Batch(vi, utts) as b:  # the zero request: the plain stage's bytes
        b.set_fbank(o)
        b.set_frame(J.frame())
        b.run()
        for i in range(len(utts)):
            assert np.array_equal(b.read_fbank(i), J.fbank_pcm(b.pcm(i), b.output_rate(i), o))


def test_batch_mfcc_with_the_energy_and_a_join(eng, batch_utts):
    vi, utts = batch_utts
    fo, fr = kaldi(40, flags=J.FRAME_REMOVE_DC | J.FRAME_ENERGY)
    mo = J.mfcc(n_ceps=13, delta_order=2, cmvn="mean_var")
    with J.Batch(vi, utts) as b:
        b.set_mfcc(mo, fbank=fo)
        b.set_fbank(fo)  # the fbank request beside it: the energy is refused for the pair
        with pytest.raises(J.JbError, match="flags"):
            b.set_frame(fr)
        b.set_fbank(None)
        b.set_frame(fr)
        b.run()
        for i in range(len(utts)):
            x, hz = b.pcm(i), b.output_rate(i)
            assert np.array_equal(b.read_mfcc(i), J.mfcc_framed_pcm(x, hz, fo, mo, fr)), i
    fo, fr = kaldi(40, flags=J.FRAME_REMOVE_DC | J.FRAME_REFLECT)
    with J.Batch(vi, utts) as b:  # both stages read one request; behind a join the programme is framed whole
        b.set_join([(0, 100, 333, 16, 16), (None, 0, 0, 0, 0), (0, 7, 2001, 0, 24)])
        b.set_frame(fr)
        b.set_fbank(fo)
        b.set_mfcc(mo, fbank=fo)
        b.run()
        assert b.num_outputs() == 2
        for p in range(2):
            x = b.programme_pcm(p)
            hz = vi.sampling_frequency
            assert b.fbank_shape(p)[0] == b.mfcc_shape(p)[0] == (x.size + hz // 200) // (hz // 100)
            assert np.array_equal(b.read_fbank(p), J.fbank_framed_pcm(x, hz, fo, fr))
            assert np.array_equal(b.read_mfcc(p), J.mfcc_framed_pcm(x, hz, fo, mo, fr))


def test_redo_rounds_see_the_final_pcm(eng):
    """Redo rounds forced the way tests/test_gpu_fbank.py forces them: a unit is recomputed whole, energies included."""
    vi, utts = _utts(eng, (600, 1100), 40)
    o, fr = kaldi(80)
    o.flags |= J.FBANK_F64
    mo = J.mfcc(n_ceps=13, delta_order=1, cmvn="mean", f64=True)
    fe = J.frame(preemph=0.97, window="povey", remove_dc=True, energy=True)
    for mfcc in (False, True):
        with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
            if mfcc:
                b.set_mfcc(mo, fbank=J.fbank(n_mels=40))
                b.set_frame(fe)
            else:
                b.set_fbank(o)
                b.set_frame(fr)
            b.run()
            b.sync()
            assert b.info()["n_redo"] >= 4
            if mfcc:
                for i in range(2):
                    want = J.mfcc_framed_pcm(b.pcm(i), b.output_rate(i), J.fbank(n_mels=40), mo, fe)
                    assert np.array_equal(b.read_mfcc(i), want)
            else:
                check_batch(b, o, fr)


def test_invariance_alone_and_among_others(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 300, 77)
    others = [synth.synth_utterance(tab, 50 + 13 * k, 1000 + k) for k in range(31)]
    o, fr = kaldi(80)
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_fbank(o)
            b.set_frame(fr)
            b.run()
            res.append(b.read_fbank(pos))
    assert np.array_equal(res[0], res[1])
    assert res[0].shape == (J.fbank_geometry(vi.sampling_frequency, o, 300 * vi.fperiod)[3], 80)


def test_engine_entries(eng):
    hz = eng.condition.get_sampling_frequency()
    o, fr = kaldi(40)
    e = eng.clone()
    e.set_frame(fr)
    pcm = e.synthesize(SAMPLE_SENTENCE_1)
    one = e.synthesize_fbank(SAMPLE_SENTENCE_1, o)
    assert np.array_equal(one, J.fbank_framed_pcm(pcm, hz, o, fr)) and one.shape[1] == 40
    assert not np.array_equal(one, eng.synthesize_fbank(SAMPLE_SENTENCE_1, o))
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    e.set_frame(preemph=0.97, window="povey", remove_dc=True, reflect=True)
    frr = J.frame(preemph=0.97, window="povey", remove_dc=True, reflect=True)
    for got, x in zip(e.synthesize_fbank_batch(sents, o), e.synthesize_batch(sents)):
        assert np.array_equal(got, J.fbank_framed_pcm(x, hz, o, frr))
    prog, starts = e.synthesize_programme(sents, sink="f64", gap_ms=120.0, fade_ms=2.0)
    feat, starts2 = e.synthesize_programme(sents, sink="fbank", gap_ms=120.0, fade_ms=2.0, opts=o)
    assert starts == starts2 and np.array_equal(feat, J.fbank_framed_pcm(prog, hz, o, frr))
    # the cepstral entries read it too, the energy with them; an fbank entry refuses the energy
    e.set_frame(remove_dc=True, energy=True)
    fre = J.frame(remove_dc=True, energy=True)
    mo = J.mfcc(n_ceps=13, delta_order=1)
    got = e.synthesize_mfcc(SAMPLE_SENTENCE_1, mo, fbank=o)
    assert np.array_equal(got, J.mfcc_framed_pcm(pcm, hz, o, mo, fre))
    with pytest.raises(J.JbError, match="flags"):
        e.synthesize_fbank(SAMPLE_SENTENCE_1, o)
    # engines of one call must agree; None withdraws
    with pytest.raises(J.JbError, match="agree"):
        J.synthesize_batch_each_fbank([eng, e], sents, o)
    e.set_frame(None)
    assert np.array_equal(e.synthesize_fbank(SAMPLE_SENTENCE_1, o), eng.synthesize_fbank(SAMPLE_SENTENCE_1, o))
    with pytest.raises(J.JbError, match="preemph"):
        e.set_frame(preemph=1.5)


def test_rules(eng):
    vi, utts = _utts(eng, (30,), 1)
    L = J.lib()
    o, fr = kaldi()
    with J.Batch(vi, utts) as b:  # without an fbank or mfcc request: an error at the first run
        b.set_frame(fr)
        with pytest.raises(J.JbError, match="jb_batch_set_fbank or jb_batch_set_mfcc"):
            b.run()
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="window"):
            b.set_frame(window=7)
        b.set_fbank(center=True)
        with pytest.raises(J.JbError, match="flags"):  # the pair, the request second ...
            b.set_frame(reflect=True)
        b.set_fbank(o)
        b.set_frame(reflect=True)
        with pytest.raises(J.JbError, match="flags"):  # ... and first
            b.set_fbank(center=True)
        n = 30 * vi.fperiod
        hop = vi.sampling_frequency // 100
        assert b.fbank_shape(0)[0] == (n + hop // 2) // hop and b.fbank_size(0) == b.fbank_shape(0)[0] * 23 * 4
        b.set_frame(None)  # withdrawn: the plain stage's T
        assert b.fbank_shape(0)[0] == J.fbank_geometry(vi.sampling_frequency, o, n)[3]
        b.set_frame(fr)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_frame(fr)
        assert np.array_equal(b.read_fbank(0), J.fbank_framed_pcm(b.pcm(0), vi.sampling_frequency, o, fr))
    with J.Batch(vi, utts, mlpg_only=True) as b:
        assert L.jb_batch_set_frame_opts(b._h, C.byref(fr)) == -1 and b"no PCM" in L.jb_last_error()
    assert L.jb_batch_set_frame_opts(None, C.byref(fr)) == -1
