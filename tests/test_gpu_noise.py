"""The noise stage on the GPU (jb_noise.hip): the device seam over the lengths, bed lengths and offsets of the host test
-- the power sums bit for bit the host rule's, the gain within an ulp of its division and square root, y bit for bit
the host rule under the device's gain -- then the stage in a batch: bit for bit the seam applied to the PCM in front of
it, behind the convolution and in front of the filter's sections, through the 16-bit sink, behind the converter, with
loudness, the join and the filterbank features reading the noisy PCM; JB_NOISE_VARY; redo rounds; the fast invariant
mode; the engine; and a batch without the request."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import join_ref
from tests import noise_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

HZ = 48000


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


def response(k, seed=2):
    rng = np.random.default_rng(seed + k)
    return rng.standard_normal(k) * np.exp(-np.arange(k) / max(1.0, k / 4.0))


def bed(n, seed=7, rms=500.0):
    return np.round(np.random.default_rng(seed + n).standard_normal(n) * rms, 2)


def same_report(a, b, gain=True):
    return (a.speech_power == b.speech_power and a.noise_power == b.noise_power and
            a.active_samples == b.active_samples and a.snr_db == b.snr_db and a.seed == b.seed and
            a.offset == b.offset and (not gain or a.gain == b.gain))


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam():
    """One launch over all the shapes of the host test: (cases, requests, outputs, reports)."""
    cases = R.cases()
    reqs = [J.noise(b, HZ, **kw) for _, b, kw in cases]
    outs, reps = J.noise_pcm([x for x, _, _ in cases], reqs, HZ)
    return cases, reqs, outs, reps


def test_the_seam_is_the_host_rule(seam):
    """A / C, C and Bs / N are the host's bit for bit (the same sums in the same order, the same division on the
    host).  The gain is one division by r and one square root behind the host's operands, each within an ulp on the
    device: |g_dev / g_host - 1| <= 2^-50 is a margin of four ulps.  y is the host rule under the device's gain."""
    cases, reqs, outs, reps = seam
    worst, mixed = 0.0, 0
    for (x, b, kw), req, y, rep in zip(cases, reqs, outs, reps):
        what = (x.size, None if b is None else b.size, kw)
        _, host = J.noise_host(x, req)
        assert same_report(rep, host, gain=False), what
        if host.gain == 0.0:
            assert rep.gain == 0.0, what
        else:
            worst = max(worst, abs(rep.gain / host.gain - 1.0))
            mixed += 1
        want, _ = J.noise_host(x, req, gain=rep.gain)
        assert y.dtype == np.float64 and same(y, want), what
    print(f"largest |g_dev / g_host - 1| over {mixed} shapes: {worst:.3e} (2^-50 = {2.0 ** -50:.3e})")
    assert mixed > len(cases) * 3 // 4
    assert worst <= 2.0 ** -50


def test_the_sixteen_bit_seam_and_any_company(seam):
    cases, reqs, outs, reps = seam
    sel = [i for i, (x, _, _) in enumerate(cases) if x.size in (257, 1025, 3 * 1024 + 17)]
    got16, rep16 = J.noise_pcm([cases[i][0] for i in sel], [reqs[i] for i in sel], HZ, i16=True)
    for i, y16, r16 in zip(sel, got16, rep16):
        assert same(y16, quant(outs[i])) and same_report(r16, reps[i]), cases[i][2]
    # an utterance's bits do not depend on the launch it is in: alone, and behind others; one without a request among
    # the others returns its input
    i = sel[-1]
    x = cases[i][0]
    alone, ra = J.noise_pcm([x], reqs[i], HZ)
    assert same(alone[0], outs[i]) and same_report(ra[0], reps[i])
    three, r3 = J.noise_pcm([cases[5][0], x, x], [reqs[5], None, reqs[i]], HZ)
    assert same(three[0], outs[5]) and same(three[1], x) and same(three[2], outs[i]) and same_report(r3[2], reps[i])
    none16, _ = J.noise_pcm([x, x], [None, reqs[i]], HZ, i16=True)
    assert same(none16[0], quant(x)) and same(none16[1], quant(outs[i]))
    # the cases that do not mix: +INFINITY, a silent bed, a silent input, an empty utterance
    z = np.zeros(2000)
    z[::2] = -0.0
    ys, rs = J.noise_pcm([x, x, z, np.zeros(0)],
                         [J.noise(bed(100), HZ, snr_db=math.inf), J.noise(np.zeros(9), HZ, snr_db=3.0),
                          J.noise(None, HZ, snr_db=3.0, seed=5), J.noise(None, HZ, snr_db=3.0)], HZ)
    assert same(ys[0], x) and same(ys[1], x) and same(ys[2], z) and ys[3].size == 0
    assert [r.gain for r in rs] == [0.0] * 4


# ---- 2. the batch path ----------------------------------------------------------------------------------------------
FRAMES = (700, 2500, 1300, 400)


@pytest.fixture(scope="module")
def batch_utts(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 3 + t) for t in FRAMES]


@pytest.fixture(scope="module")
def plain_pcm(batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.run()
        return [b.pcm(i) for i in range(len(utts))]


def batch_noise(hz):
    """A bed at 10 dB, white at 20 dB against the active tiles, none, and a 7-sample bed at 0 dB."""
    return [J.noise(bed(30000), hz, snr_db=10.0, offset=12345),
            J.noise(None, hz, snr_db=20.0, seed=99, reference="active", gate_db=20.0), None,
            J.noise(bed(7), hz, snr_db=0.0, offset=6)]


def test_batch_is_the_seam_bit_for_bit(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    reqs = batch_noise(hz)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="the batch has not run"):
            b.set_noise(reqs)
            b.noise_report(0)
        b.run()
        native = [b.pcm_native(i) for i in range(4)]
        want, reps = J.noise_pcm(native, reqs, hz)
        for i in range(4):
            assert same(native[i], plain_pcm[i])  # the native read stays the vocoder's PCM
            assert same(b.pcm(i), want[i]), i
            if reqs[i] is not None:
                assert same_report(b.noise_report(i), reps[i]), i
        assert same(b.pcm(2), native[2]) and not same(b.pcm(0), native[0])
        with pytest.raises(J.JbError, match="utterance 2 has no noise request"):
            b.noise_report(2)
        r0, r1 = b.noise_report(0), b.noise_report(1)
        assert abs(10 * math.log10(r0.speech_power / (r0.gain ** 2 * r0.noise_power)) - 10.0) < 1e-9
        assert 0 < r1.active_samples < native[1].size  # the silence around the speech is not counted
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_noise(reqs)
    # one request for the whole batch
    with J.Batch(vi, utts) as b:
        b.set_noise(reqs[3])
        b.run()
        assert same(b.pcm(1), J.noise_pcm([plain_pcm[1]], reqs[3], hz)[0][0])
    # the refusals of the setter, before anything runs
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one request, or one per utterance"):
            b.set_noise(reqs[:2])
        with pytest.raises(J.JbError, match="utterance 1: offset must be below bed_len"):
            b.set_noise([None, J.noise([1.0, 2.0], hz, snr_db=3.0, offset=2), None, None])
        with pytest.raises(J.JbError, match="utterance 3: hz differs"):
            b.set_noise([None, None, None, J.noise([1.0, 2.0], hz + 1, snr_db=3.0)])
        with pytest.raises(J.JbError, match="utterance 0: flags: JB_NOISE_VARY"):
            b.set_noise([J.noise(None, hz, snr_db=3.0, vary=True), None, None, None])
        with pytest.raises(J.JbError, match="jb_batch_set_noise was not called"):
            b.run()
            b.noise_report(0)


def test_without_a_request_the_bytes_are_the_batch_of_today(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    for req in ("withdrawn", "no bed"):
        with J.Batch(vi, utts) as b:
            b.set_noise(batch_noise(hz))
            b.set_noise(None if req == "withdrawn" else [None, J.Noise(), None, None])
            b.run()
            assert all(same(b.pcm(i), plain_pcm[i]) for i in range(4)), req


# ---- 3. order -------------------------------------------------------------------------------------------------------
def test_response_then_noise_then_sections(batch_utts, plain_pcm):
    """Every subset of (response, noise, section) on utterance 0, the others carrying other mixes: the batch is
    filter_pcm(noise_pcm(fir_pcm(x))) with the absent ones left out, bit for bit."""
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    f, nz, hp = J.fir(response(300), hz, 10), J.noise(bed(5000), hz, snr_db=5.0, offset=77), J.highpass(70.0)
    other_f = [J.fir(response(64), hz, 0), None, J.fir(response(1500), hz, 3)]
    other_n = [None, J.noise(None, hz, snr_db=12.0, seed=4), J.noise(bed(7), hz, snr_db=30.0)]
    other_s = [J.highpass(120.0), J.peaking(3000.0, 6.0, 2.0), None]

    def chain(x, fir, noise, filt):
        if fir is not None:
            x = J.fir_pcm([x], fir, hz)[0]
        if noise is not None:
            x = J.noise_pcm([x], noise, hz)[0][0]
        if filt is not None:
            x = J.filter_pcm([x], filt, hz)[0]
        return x

    for mask in range(1, 8):
        firs = [f if mask & 1 else None] + other_f
        noises = [nz if mask & 2 else None] + other_n
        filts = [hp if mask & 4 else None] + other_s
        with J.Batch(vi, utts) as b:
            b.set_filter(filts)
            b.set_noise(noises)
            b.set_fir(firs)  # (the setters come in any order)
            b.run()
            for i in range(4):
                assert same(b.pcm(i), chain(plain_pcm[i], firs[i], noises[i], filts[i])), (mask, i)


def test_i16_is_the_quantised_f64(batch_utts):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    reqs = batch_noise(hz)
    firs = [J.fir(response(64), hz, 5), None, None, J.fir(response(700), hz, 0)]
    filts = [J.highpass(70.0), None, J.highpass(70.0), None]
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_noise(reqs)
        b.set_filter(filts)
        b.run()
        f64 = [b.pcm(i) for i in range(4)]
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_fir(firs)
        b.set_noise(reqs)
        b.set_filter(filts)
        b.run()
        for i in range(4):
            assert same(b.pcm_i16(i), quant(f64[i])), i


# ---- 4. other requests in the chain ---------------------------------------------------------------------------------
def test_behind_the_converter_at_16_khz(batch_utts):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    with J.Batch(vi, utts) as b:
        b.set_output_rate(16000)
        b.run()
        conv = [b.pcm(i) for i in range(4)]
    reqs = batch_noise(16000)
    with J.Batch(vi, utts) as b:
        # a bed at the voice's rate is accepted now and refused by the later rate request, which changes nothing
        b.set_noise(J.noise(bed(100), hz, snr_db=10.0))
        with pytest.raises(J.JbError, match="utterance 0: hz of its noise bed differs"):
            b.set_output_rate(16000)
        assert [b.output_rate(i) for i in range(4)] == [hz] * 4
        b.set_noise(None)
        b.set_output_rate(16000)
        with pytest.raises(J.JbError, match="utterance 0: hz differs"):
            b.set_noise(J.noise(bed(100), hz, snr_db=10.0))
        b.set_noise(reqs)
        b.run()
        want, _ = J.noise_pcm(conv, reqs, 16000)
        for i in range(4):
            assert same(b.pcm(i), want[i]), i


def test_loudness_join_and_fbank_read_the_noisy_pcm(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    reqs = batch_noise(hz)
    noisy, _ = J.noise_pcm(plain_pcm, reqs, hz)
    with J.Batch(vi, utts) as b:
        b.set_noise(reqs)
        b.set_loudness_target([-20.0, -26.0, -16.0, -23.0], math.inf)
        b.run()
        for i, (L, _) in enumerate(J.loudness(noisy, hz)):
            lufs, _, gain = b.loudness(i)
            assert abs(lufs - L) <= 1e-8  # (the tolerance of tests/test_gpu_loudness.py for the same comparison)
            np.testing.assert_allclose(b.pcm(i), noisy[i] * 10.0 ** (gain / 20.0), rtol=1e-15, atol=0)
    req = [(0, 100, 3, 48, 48), (None, 1, 1, 0, 0), (0, 7, 2400, 48, 48), (None, 0, 0, 0, 0)]
    with J.Batch(vi, utts) as b:
        b.set_noise(reqs)
        b.set_join(req)
        b.run()
        pcms = [b.pcm(i) for i in range(4)]
        assert all(same(p, c) for p, c in zip(pcms, noisy))
        progs, _, _ = join_ref.join(pcms, req)
        for p, w in enumerate(progs):
            assert same(b.programme_pcm(p), w.astype(np.float64)), p
    opts = J.fbank(n_mels=40)
    with J.Batch(vi, utts) as b:
        b.set_noise(reqs)
        b.set_fbank(opts)
        b.run()
        want = J.fbank_pcm(noisy, hz, opts)
        for i in range(4):
            assert same(np.asarray(b.read_fbank(i)), np.asarray(want[i])), i


def test_vary_gives_each_utterance_its_own_noise(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    for b_ in (bed(5000), None):
        lb = 0 if b_ is None else b_.size
        with J.Batch(vi, utts) as b:
            b.set_noise(J.noise(b_, hz, snr_db=8.0, seed=31, offset=3, vary=True))
            b.run()
            got = [b.pcm(k) for k in range(4)]
            reps = [b.noise_report(k) for k in range(4)]
        for k in range(4):
            s, o = J.noise_vary(31, k, lb)
            assert (reps[k].seed, reps[k].offset) == (s, o) == R.vary(31, k, lb)
            want, _ = J.noise_pcm([plain_pcm[k]], J.noise(b_, hz, snr_db=8.0, seed=s, offset=o), hz)
            assert same(got[k], want[0]), k


# ---- 5. redo rounds, invariance, the engine -------------------------------------------------------------------------
def test_redo_rounds_add_noise_to_the_final_pcm(eng, tab):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12), as in tests/test_gpu_chain_redo.py: redo rounds
    rewrite most chunks after run() has mixed the first PCM; the touched utterances run again whole."""
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    utts = [synth.synth_utterance(tab, t, 40 + t) for t in (600, 1100)]
    firs = [J.fir(response(200), hz, 99), None]
    reqs = [J.noise(bed(9000), hz, snr_db=6.0, offset=8000, reference="active", gate_db=25.0),
            J.noise(None, hz, snr_db=14.0, seed=8)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_fir(firs)
        b.set_noise(reqs)
        b.set_filter([J.highpass(50.0), None])
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        native = [b.pcm_native(i) for i in range(2)]
        conv = J.fir_pcm(native, firs, hz)
        noisy, reps = J.noise_pcm(conv, reqs, hz)
        assert same(b.pcm(0), J.filter_pcm([noisy[0]], J.highpass(50.0), hz)[0])
        assert same(b.pcm(1), noisy[1])
        assert all(same_report(b.noise_report(i), reps[i]) for i in range(2))


def test_invariance_alone_and_in_a_batch(eng, tab):
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(15)]
    pn = J.noise(bed(4000), hz, snr_db=9.0, offset=3999, reference="active", gate_db=20.0)
    on = [[J.noise(bed(50 + k), hz, snr_db=float(k)), J.noise(None, hz, snr_db=20.0, seed=k), None][k % 3]
          for k in range(15)]
    res = []
    for utts, reqs, pos in (([probe], [pn], 0), (others[:6] + [probe] + others[6:], on[:6] + [pn] + on[6:], 6)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_noise(reqs)
            b.run()
            res.append(b.pcm(pos).tobytes())
    assert res[0] == res[1] and len(res[0]) == 8 * 900 * vi.fperiod


def test_engine_entries(eng):
    hz = eng._out_hz()
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    plain = [np.array(x) for x in eng.synthesize_batch(sents)]
    nz = J.noise(bed(20000), hz, snr_db=15.0, offset=19999)
    en = eng.clone()
    en.set_noise(nz)
    want, _ = J.noise_pcm(plain, nz, hz)
    assert same(en.synthesize(SAMPLE_SENTENCE_1), want[0])
    assert all(same(np.array(g), w) for g, w in zip(en.synthesize_batch(sents), want))
    assert all(same(np.array(g), quant(w)) for g, w in zip(en.synthesize_batch(sents, i16=True), want))
    assert same(en.clone().synthesize(SAMPLE_SENTENCE_1), want[0])  # copied with the Condition, bed and all
    each = J.synthesize_batch_each([eng, en], sents)
    assert same(np.array(each[0]), plain[0]) and same(np.array(each[1]), want[1])
    assert same(en.generator(SAMPLE_SENTENCE_1).generate_all(), want[0])
    # JB_NOISE_VARY: the utterance of index k in the call
    en.set_noise(J.noise(None, hz, snr_db=15.0, seed=5, vary=True))
    got = [np.array(g) for g in en.synthesize_batch(sents)]
    for k in range(2):
        s, _ = J.noise_vary(5, k, 0)
        assert same(got[k], J.noise_pcm([plain[k]], J.noise(None, hz, snr_db=15.0, seed=s), hz)[0][0]), k
    with pytest.raises(J.JbError, match="hz differs"):
        en.set_noise(J.noise([1.0], hz + 1, snr_db=3.0))
    en.set_noise(None)
    assert all(same(np.array(g), w) for g, w in zip(en.synthesize_batch(sents), plain))
