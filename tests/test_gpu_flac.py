"""FLAC output on the GPU (jb_flac.hip): streams of crafted signals decoded back exactly by the strict test decoder
(tests/flac_ref.py), then every entry -- batches with output rates, loudness targets, redo rounds and a gang
timeout, the fast invariant mode, the engine entries and their rules -- against the 16-bit PCM the same batch
hands out and against jb_flac_encode_pcm_batch of that PCM."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests.conftest import VOICE
from tests.flac_ref import decode, verbatim_frame_bound
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def signals(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    sq = np.where((t // 37) % 2 == 0, 32767, -32768)
    alt = np.where(t % 2 == 0, 32767, -32768)
    sine = np.round(12000 * np.sin(2 * np.pi * 440 * t / 48000) + 3000 * np.sin(2 * np.pi * 3100 * t / 48000))
    chirp = np.round(20000 * np.sin(2 * np.pi * (100 + 4000 * t / max(n, 1)) * t / 48000))
    return {"silence": np.zeros(n), "dc": np.full(n, -1234), "square": sq, "alternating": alt,
            "noise": rng.integers(-32768, 32768, n), "sine": sine, "chirp": chirp}


def check_stream(data, pcm, hz, bs):
    got, info = decode(data)
    assert got.tobytes() == np.asarray(pcm, dtype=np.int16).tobytes()
    assert info["rate"] == hz and info["block_size"] == bs and info["total"] == len(pcm)
    for f, size in enumerate(info["frame_sizes"]):
        n = min(bs, len(pcm) - f * bs)
        assert size <= verbatim_frame_bound(n, f, hz), (f, size)
    return info


@pytest.mark.parametrize("bs,order", [(16, 0), (1152, 8), (4096, 12), (4096, 8)])
def test_crafted_signals_round_trip(eng, bs, order):
    lengths = sorted({0, 1, 15, 16, 17, bs - 1, bs, bs + 1, 3 * bs})
    pcms, names = [], []
    for n in lengths:
        for name, x in signals(n, seed=n).items():
            pcms.append(np.asarray(x, dtype=np.int16))
            names.append((name, n))
    for hz in (8000, 11025, 22050, 48000, 96000):
        streams = J.flac_encode(pcms, hz, block_size=bs, max_lpc_order=order)
        assert len(streams) == len(pcms)
        for (name, n), data, x in zip(names, streams, pcms):
            if hz != 48000 and n > bs + 1:
                continue  # the long ones are decoded at 48 kHz; other rates differ only in the header
            info = check_stream(data, x, hz, bs)
            if name in ("silence", "dc") and n:
                assert set(info["types"]) == {"constant"}, (name, n)
            if n == 0:
                assert len(data) == 42 and info["min_frame"] == info["max_frame"] == 0


def test_over_128_frames_and_silence_sizes(eng):
    bs = 16
    x = signals(130 * bs + 5, seed=3)
    pcms = [np.asarray(x["chirp"], dtype=np.int16), np.asarray(x["noise"], dtype=np.int16)]
    for data, p in zip(J.flac_encode(pcms, 48000, block_size=bs, max_lpc_order=8), pcms):
        info = check_stream(data, p, 48000, bs)
        assert info["frames"] == 131  # frame numbers 128.. take two bytes
    for k in (1, 2, 5, 127):
        (data,) = J.flac_encode([np.zeros(k * 4096, dtype=np.int16)], 48000)
        assert len(data) == 42 + 11 * k  # 6-byte headers, 3-byte CONSTANT subframes, CRC-16


def test_full_scale_noise_stays_verbatim_bound(eng):
    x = np.random.default_rng(9).integers(-32768, 32768, 4096 * 3).astype(np.int16)
    (data,) = J.flac_encode([x], 48000)
    info = check_stream(data, x, 48000, 4096)
    assert len(data) <= 42 + 3 * verbatim_frame_bound(4096, 0, 48000)
    assert set(info["types"]) <= {"verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"} | {
        f"lpc{o}" for o in range(1, 13)}


def test_unsupported_rate_and_bad_options(eng):
    x = [np.zeros(100, dtype=np.int16)]
    with pytest.raises(J.JbError):
        J.flac_encode(x, 65537)  # no kHz, 16-bit-Hz or tens-of-Hz form
    for hz in (65535, 88200, 176400, 192000, 12345, 655350):
        (data,) = J.flac_encode(x, hz)
        assert decode(data)[1]["rate"] == hz


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, T, seed + T) for T in frames]


def batch_streams(b, decode_all=True, opts=None):
    """Every utterance: decode(read_flac(u)) == read_pcm_i16(u), and the bytes equal jb_flac_encode_pcm_batch's."""
    opts = opts or {}
    streams = b.flac_all()
    pcms = [b.pcm_i16(i) for i in range(len(b))]
    for i in range(len(b)):
        hz = b.output_rate(i)
        assert b.flac(i) == streams[i]
        (ref,) = J.flac_encode([pcms[i]], hz, **opts)
        assert ref == streams[i], i
        if decode_all or i < 2:
            check_stream(streams[i], pcms[i], hz, opts.get("block_size") or 4096)
    return streams, pcms


def test_ragged_batch(eng):
    vi, utts = _utts(eng, (300, 1, 777, 60, 1500), 11)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_flac()
        b.run()
        streams, pcms = batch_streams(b)
    assert sum(len(s) for s in streams) < 2 * sum(p.size for p in pcms)


@pytest.mark.parametrize("rates,target", [((16000,), None), ((22050, 16000, 48000), None), ((0,), -20.0),
                                          ((22050, 16000, 0), -23.0)])
def test_rates_and_targets(eng, rates, target):
    vi, utts = _utts(eng, (500, 900, 240), 5)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        if rates != (0,):
            b.set_output_rate(list(rates) if len(rates) > 1 else rates[0])
        if target is not None:
            b.set_loudness_target(target, 0.0)
        b.set_flac(block_size=1152, max_lpc_order=12)
        b.run()
        batch_streams(b, opts={"block_size": 1152, "max_lpc_order": 12})


def test_redo_rounds_encode_the_final_pcm(eng):
    vi, utts = _utts(eng, (600, 1100), 40)
    with J.Batch(vi, utts, pcm_i16=True, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target(-20.0, math.inf)
        b.set_flac()
        b.run()
        b.sync()
        assert b.info()["n_redo"] > 0
        batch_streams(b)


def test_gang_timeout(eng):
    vi, utts = _utts(eng, (400, 700, 90), 21)
    with J.Batch(vi, utts, pcm_i16=True, test_gang_timeout=True) as b:
        b.set_flac()
        b.run()
        batch_streams(b)


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20), (others + [probe], 63)):
        with J.Batch(vi, utts, pcm_i16=True, fast_invariant=True) as b:
            b.set_flac()
            b.run()
            res.append(b.flac(pos))
    assert res[0] == res[1] == res[2]


def test_engine_entries(eng):
    data = eng.synthesize_flac(SAMPLE_SENTENCE_1)
    (pcm,) = eng.synthesize_batch([SAMPLE_SENTENCE_1], i16=True)
    info = check_stream(data, pcm, 48000, 4096)
    assert len(data) < 2 * pcm.size
    e2 = eng.clone()
    e2.condition.set_output_sampling_frequency(22050)
    e2.condition.set_loudness_target(-18.0)
    out = J.synthesize_batch_each_flac([eng, e2], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], block_size=2304)
    ref = J.synthesize_batch_each([eng, e2], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], i16=True)
    for data, p, hz in zip(out, ref, (48000, 22050)):
        check_stream(data, p, hz, 2304)
    (b2,) = e2.synthesize_batch_flac([SAMPLE_SENTENCE_2])
    check_stream(b2, ref[1], 22050, 4096)
    assert info["rate"] == 48000


def test_rules(eng):
    vi, utts = _utts(eng, (100,), 1)
    with J.Batch(vi, utts) as b:  # f64 batch
        with pytest.raises(J.JbError):
            b.set_flac()
    with J.Batch(vi, utts, pcm_i16=True, mlpg_only=True) as b:
        with pytest.raises(J.JbError):
            b.set_flac()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.run()
        with pytest.raises(J.JbError):
            b.set_flac()
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_output_rate(65875)  # 48000 * 527 / 384: the converter takes it, FLAC has no code
        b.set_flac()
        with pytest.raises(J.JbError):
            b.run()
    e = eng.clone()
    e.condition.set_output_sampling_frequency(65875)
    with pytest.raises(J.JbError):
        e.synthesize_flac(SAMPLE_SENTENCE_1)


def test_speech_compresses(eng):
    vi, utts = _utts(eng, (2000, 1200, 800), 2)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_flac()
        b.run()
        streams, pcms = batch_streams(b, decode_all=False)
    nb, ns = sum(len(s) for s in streams), sum(p.size for p in pcms)
    assert nb < 2 * ns
    print(f"speech: {nb / ns:.3f} bytes per sample")
