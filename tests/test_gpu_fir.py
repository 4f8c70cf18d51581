"""The convolution stage on the GPU (jb_fir.hip): the device seam over tap counts, lengths and delays around every edge
of the two modes -- direct mode against the host rule bit for bit, partitioned mode under the error gate against the
long-double sum -- then the stage in a batch: bit for bit the seam applied to the PCM in front of it, with different
responses side by side, in front of the filter's sections, through the 16-bit sink, behind the converter, with loudness,
the join and the filterbank features reading the convolved PCM; redo rounds; the fast invariant mode; the engine; and a
batch without the request.

The error gate of partitioned mode.  e = max|y - y_ld| / (||h||_1 max|x|) against the long-double sum; the yardstick
e_np is the same metric of float64 numpy.fft.irfft(rfft(x, n) rfft(h, n)) over the whole signal; the device gets
8 e_np (it differs from numpy in FMA contraction and summation order, not in algorithm class).  Where the float64
model of the same partitioned algorithm (tests/fir_ref.py: model_partitioned) alone exceeds 4 e_np, the gate of that
shape is twice the model's ratio.  Measured with numpy 1.26 over the shapes below: the model stays at or below 4 e_np
everywhere but at three shapes of ONE sample, where e_np is the luck of a single rounding (1e-19 .. 2e-20 of the
scale): (K, N, d) = (1025, 1, 1024): 6.65, (2048, 1, 1023): 17.70, (2049, 1, 1): 25.09.
The device's ratios per shape are in profiles/r21_fir.txt."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import fir_ref as R
from tests import join_ref
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

HZ = 48000
DIRECT_K = (1, 2, 255, 256)
PART_K = (257, 1024, 1025, 2 * 1024 + 3, 2048, 2049, 2 * 2048 + 3, 5000)  # Bk, Bk + 1, 2 Bk + 3 of both block sizes


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


def signal(n, seed=1):
    rng = np.random.default_rng(seed)
    return np.round(rng.standard_normal(n) * 6000.0, 3)


def response(k, seed=2):
    rng = np.random.default_rng(seed + k)
    return rng.standard_normal(k) * np.exp(-np.arange(k) / max(1.0, k / 4.0))


def lengths(k):
    _, block, _ = J.fir_geometry(k)
    return sorted({1, block - 1, block, block + 1, 3 * block + 17} | ({k - 1} if k > 1 else set()))


def shapes(ks):
    return [(k, n, d) for k in ks for n in lengths(k) for d in R.delays(k)]


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
def test_direct_mode_is_the_host_rule_bit_for_bit():
    cases = shapes(DIRECT_K)
    assert all(J.fir_geometry(k)[0] == J.FIR_DIRECT for k in DIRECT_K)
    pcms = [signal(n) for _, n, _ in cases]
    for x in pcms:
        x[::7] = -0.0
    firs = [J.fir(response(k), HZ, d) for k, _, d in cases]
    got = J.fir_pcm(pcms, firs, HZ)
    for (k, n, d), x, f, y in zip(cases, pcms, firs, got):
        assert y.dtype == np.float64 and same(y, J.fir_host(x, f)), (k, n, d)
    # the one-tap identity, and an utterance without a response among the others
    x = pcms[-1]
    three = J.fir_pcm([x, x, x], [J.fir([1.0], HZ), None, firs[-1]], HZ)
    assert same(three[0], x) and same(three[1], x) and same(three[2], J.fir_host(x, firs[-1]))
    # the 16-bit seam is the 16-bit sink's rule on the same y
    sel = [i for i, (k, n, d) in enumerate(cases) if n > 2048]
    got16 = J.fir_pcm([pcms[i] for i in sel], [firs[i] for i in sel], HZ, i16=True)
    for i, y16 in zip(sel, got16):
        assert same(y16, quant(got[i])), cases[i]


@pytest.fixture(scope="module")
def partitioned():
    """One launch with every partitioned shape; the references once: (cases, inputs, device outputs, e, e_np, gate)."""
    cases = shapes(PART_K)
    assert all(J.fir_geometry(k)[0] == J.FIR_PARTITIONED for k in PART_K)
    hs = {k: response(k) for k in PART_K}
    xs = {n: signal(n) for _, n, _ in cases}
    got = J.fir_pcm([xs[n] for _, n, _ in cases], [J.fir(hs[k], HZ, d) for k, _, d in cases], HZ)
    full = {}
    rows = []
    for (k, n, d), y in zip(cases, got):
        x, h = xs[n], hs[k]
        if (k, n) not in full:
            full[(k, n)] = np.convolve(x.astype(np.longdouble), h.astype(np.longdouble))
        y_ld = full[(k, n)][d:d + n]
        _, block, parts = J.fir_geometry(k)
        e_np = R.rel_err(R.fft_whole(x, h, d), y_ld, x, h)
        e_model = R.rel_err(R.model_partitioned(x, h, d, block, parts), y_ld, x, h)
        ratio = 8.0 if e_model <= 4.0 * e_np else 2.0 * e_model / e_np
        rows.append(((k, n, d), y, R.rel_err(y, y_ld, x, h), e_np, ratio * e_np))
    return cases, xs, hs, got, rows


def test_partitioned_mode_holds_the_error_gate(partitioned):
    cases, xs, hs, got, rows = partitioned
    worst = 0.0
    for (k, n, d), y, e, e_np, gate in rows:
        assert y.dtype == np.float64 and y.size == n
        print(f"K {k:5d} N {n:5d} d {d:5d}  e {e:.3e}  e_np {e_np:.3e}  e / e_np {e / e_np:6.2f}  gate {gate / e_np:6.2f}")
        worst = max(worst, e / e_np)
    print(f"largest e / e_np {worst:.2f}")
    for (k, n, d), y, e, e_np, gate in rows:
        assert e <= gate, (k, n, d, e, e_np, gate)


def test_partitioned_sixteen_bit_seam_and_same_bits_in_any_company(partitioned):
    cases, xs, hs, got, _ = partitioned
    sel = [i for i, (k, n, d) in enumerate(cases) if k in (1025, 5000) and n > 1]
    firs = [J.fir(hs[cases[i][0]], HZ, cases[i][2]) for i in sel]
    got16 = J.fir_pcm([xs[cases[i][1]] for i in sel], firs, HZ, i16=True)
    for i, y16 in zip(sel, got16):
        assert same(y16, quant(got[i])), cases[i]
    # an utterance's bits do not depend on the launch it is in: alone, and behind a direct one
    i = sel[-1]
    alone = J.fir_pcm([xs[cases[i][1]]], firs[-1], HZ)
    assert same(alone[0], got[i])
    pair = J.fir_pcm([signal(300), xs[cases[i][1]]], [J.fir(response(7), HZ, 3), firs[-1]], HZ)
    assert same(pair[1], got[i])


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


def batch_firs(hz):
    """Three different responses -- direct, the small transform, the large one -- and an utterance without one."""
    return [J.fir(response(64), hz, 5), J.fir(response(1500), hz, 749), None, J.fir(response(5000), hz, 40)]


def test_batch_is_the_seam_bit_for_bit(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    firs = batch_firs(hz)
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        assert b.fir_geometry(0) == J.fir_geometry(64) and b.fir_geometry(1) == J.fir_geometry(1500)
        assert b.fir_geometry(3) == J.fir_geometry(5000) == (J.FIR_PARTITIONED, 2048, 3)
        with pytest.raises(J.JbError, match="utterance 2 has no impulse response"):
            b.fir_geometry(2)
        b.run()
        native = [b.pcm_native(i) for i in range(4)]
        want = J.fir_pcm(native, firs, hz)
        for i in range(4):
            assert same(native[i], plain_pcm[i])  # the native read stays the vocoder's PCM
            assert same(b.pcm(i), want[i]), i
        assert same(b.pcm(2), native[2]) and not same(b.pcm(0), native[0])
        assert same(want[0], J.fir_host(native[0], firs[0]))  # direct mode: the host rule itself
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_fir(firs)
    # one response for the whole batch
    with J.Batch(vi, utts) as b:
        b.set_fir(firs[1])
        b.run()
        assert same(b.pcm(3), J.fir_pcm([plain_pcm[3]], firs[1], hz)[0])
    # the refusals of the setter, before anything runs
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one response, or one per utterance"):
            b.set_fir(firs[:2])
        with pytest.raises(J.JbError, match="utterance 1: delay must be below n_taps"):
            b.set_fir([None, J.fir([1.0, 2.0], hz, 2), None, None])
        with pytest.raises(J.JbError, match="utterance 3: hz differs"):
            b.set_fir([None, None, None, J.fir([1.0, 2.0], hz + 1, 0)])


def test_without_a_request_the_bytes_are_the_batch_of_today(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    for req in ("withdrawn", "no taps"):
        with J.Batch(vi, utts) as b:
            b.set_fir(batch_firs(hz))
            b.set_fir(None if req == "withdrawn" else [None, J.fir(None, hz), None, None])
            b.run()
            assert all(same(b.pcm(i), plain_pcm[i]) for i in range(4)), req


def test_in_front_of_the_sections(batch_utts, plain_pcm):
    """Utterance 0: a response and a section; 1: a response only; 2: a section only; 3: neither."""
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    hp = J.highpass(70.0) + J.peaking(3000.0, 6.0, 2.0)
    firs = [J.fir(response(1500), hz, 10), J.fir(response(64), hz, 0), None, None]
    filts = [hp, None, J.highpass(120.0), None]
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_filter(filts)
        b.run()
        got = [b.pcm(i) for i in range(4)]
    conv = J.fir_pcm(plain_pcm, firs, hz)
    assert same(got[0], J.filter_pcm([conv[0]], hp, hz)[0])  # convolution first, then the cascade
    assert same(got[1], conv[1]) and same(conv[1], J.fir_host(plain_pcm[1], firs[1]))
    assert same(got[2], J.filter_pcm([plain_pcm[2]], filts[2], hz)[0])
    assert same(got[3], plain_pcm[3])
    # against the host alone: the host rule, then jb_filter_pcm_host.  The convolution (direct mode) is the host's bit
    # for bit, so what is left is the filter stage's own distance from its serial recursion: tests/filter_ref.py's gate
    # (8 times scipy's sosfilt's error against the long-double cascade), of the output's largest sample
    from tests import filter_ref
    want = J.filter_pcm_host(J.fir_host(plain_pcm[1], firs[1]), J.highpass(70.0), hz)
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_filter([None, J.highpass(70.0), None, None])
        b.run()
        y = b.pcm(1)
    assert np.max(np.abs(y - want)) <= filter_ref.gate() * np.max(np.abs(want))


def test_i16_is_the_quantised_f64(batch_utts):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    firs = batch_firs(hz)
    filts = [J.highpass(70.0), None, None, None]
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_filter(filts)
        b.run()
        f64 = [b.pcm(i) for i in range(4)]
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_fir(firs)
        b.set_filter(filts)
        b.run()
        for i in range(4):
            assert same(b.pcm_i16(i), quant(f64[i])), i


def test_behind_the_converter_at_16_khz(batch_utts):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    with J.Batch(vi, utts) as b:
        b.set_output_rate(16000)
        b.run()
        conv = [b.pcm(i) for i in range(4)]
    firs = batch_firs(16000)
    with J.Batch(vi, utts) as b:
        # a response at the voice's rate is accepted now and refused by the later rate request, which changes nothing
        b.set_fir(J.fir(response(64), hz, 5))
        with pytest.raises(J.JbError, match="utterance 0: hz of its impulse response differs"):
            b.set_output_rate(16000)
        assert [b.output_rate(i) for i in range(4)] == [hz] * 4
        b.set_fir(None)
        b.set_output_rate(16000)
        with pytest.raises(J.JbError, match="utterance 0: hz differs"):
            b.set_fir(J.fir(response(64), hz, 5))
        b.set_fir(firs)
        b.run()
        want = J.fir_pcm(conv, firs, 16000)
        for i in range(4):
            assert same(b.pcm(i), want[i]), i


def test_loudness_join_and_fbank_read_the_convolved_pcm(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    firs = batch_firs(hz)
    conv = J.fir_pcm(plain_pcm, firs, hz)
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_loudness_target([-20.0, -26.0, -16.0, -23.0], math.inf)
        b.run()
        for i, (L, _) in enumerate(J.loudness(conv, hz)):
            lufs, _, gain = b.loudness(i)
            assert abs(lufs - L) <= 1e-8  # (the tolerance of tests/test_gpu_loudness.py for the same comparison)
            np.testing.assert_allclose(b.pcm(i), conv[i] * 10.0 ** (gain / 20.0), rtol=1e-15, atol=0)
    req = [(0, 100, 3, 48, 48), (None, 1, 1, 0, 0), (0, 7, 2400, 48, 48), (None, 0, 0, 0, 0)]
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_join(req)
        b.run()
        pcms = [b.pcm(i) for i in range(4)]
        assert all(same(p, c) for p, c in zip(pcms, conv))
        progs, _, _ = join_ref.join(pcms, req)
        seam = J.join_pcm(conv, req)  # the join's own seam, fed the convolved PCM
        for p, w in enumerate(progs):
            assert same(b.programme_pcm(p), w.astype(np.float64)), p
            assert same(b.programme_pcm(p), np.asarray(seam[p])), p
    opts = J.fbank(n_mels=40)
    with J.Batch(vi, utts) as b:
        b.set_fir(firs)
        b.set_fbank(opts)
        b.run()
        want = J.fbank_pcm(conv, hz, opts)
        for i in range(4):
            assert same(np.asarray(b.read_fbank(i)), np.asarray(want[i])), i


# ---- 3. redo rounds, invariance -------------------------------------------------------------------------------------
def test_redo_rounds_convolve_the_final_pcm(eng, tab):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12), as in tests/test_gpu_chain_redo.py: redo rounds
    rewrite most chunks after run() has convolved the first PCM; the touched utterances run again whole."""
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    utts = [synth.synth_utterance(tab, t, 40 + t) for t in (600, 1100)]
    firs = [J.fir(response(200), hz, 99), J.fir(response(2500), hz, 17)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_fir(firs)
        b.set_filter([J.highpass(50.0), None])
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        native = [b.pcm_native(i) for i in range(2)]
        conv = J.fir_pcm(native, firs, hz)
        assert same(b.pcm(0), J.filter_pcm([conv[0]], J.highpass(50.0), hz)[0])
        assert same(b.pcm(1), conv[1])


def test_invariance_alone_and_in_a_batch(eng, tab):
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(15)]
    pf = J.fir(response(3000), hz, 1499)
    of = [[J.fir(response(40 + k), hz, k), J.fir(response(600 + k), hz, 0), None][k % 3] for k in range(15)]
    res = []
    for utts, firs, pos in (([probe], [pf], 0), (others[:6] + [probe] + others[6:], of[:6] + [pf] + of[6:], 6)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_fir(firs)
            b.run()
            res.append(b.pcm(pos).tobytes())
    assert res[0] == res[1] and len(res[0]) == 8 * 900 * vi.fperiod


# ---- 4. the engine entries ------------------------------------------------------------------------------------------
def test_engine_entries(eng):
    hz = eng._out_hz()
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    plain = [np.array(x) for x in eng.synthesize_batch(sents)]
    f = J.fir(response(1200), hz, 3)
    ef = eng.clone()
    ef.set_fir(f)
    want = J.fir_pcm(plain, f, hz)
    assert same(ef.synthesize(SAMPLE_SENTENCE_1), want[0])
    assert all(same(np.array(g), w) for g, w in zip(ef.synthesize_batch(sents), want))
    assert all(same(np.array(g), quant(w)) for g, w in zip(ef.synthesize_batch(sents, i16=True), want))
    assert same(ef.clone().synthesize(SAMPLE_SENTENCE_1), want[0])  # copied with the Condition, taps and all
    each = J.synthesize_batch_each([eng, ef], sents)
    assert same(np.array(each[0]), plain[0]) and same(np.array(each[1]), want[1])
    assert same(ef.generator(SAMPLE_SENTENCE_1).generate_all(), want[0])
    with pytest.raises(J.JbError, match="hz differs"):
        ef.set_fir(J.fir([1.0], hz + 1))
    ef.set_fir(None)
    assert all(same(np.array(g), w) for g, w in zip(ef.synthesize_batch(sents), plain))
