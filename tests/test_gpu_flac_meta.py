"""FLAC metadata on the GPU (jb_flac.hip k_flac_md5, k_flac_header, k_flac_seektable): the STREAMINFO MD5 against
hashlib over the padding and alignment cases and over batches that fill lanes and waves unevenly, the SEEKTABLE
against the frames the strict decoder finds (tests/flac_meta_ref.py), then every entry -- batches with output rates,
loudness targets, redo rounds and a gang timeout, the fast invariant mode, the engine entries and their rules -- with
both requests on, against the 16-bit PCM the same batch hands out."""
import hashlib
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests.conftest import VOICE
from tests.flac_meta_ref import check, split
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

SEEK_MS = 100  # with both requests on: a point every 100 ms


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def md5_of(pcm):
    return hashlib.md5(np.asarray(pcm).astype("<i2").tobytes()).digest()


def odd_views(lengths, seed):
    """int16 arrays of the lengths, each a view that starts at an odd sample of a larger buffer."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        buf = rng.integers(-32768, 32768, n + 3).astype(np.int16)
        out.append(buf[1:1 + n])
        assert out[-1].size == n and (n == 0 or out[-1].ctypes.data % 4 == 2)
    return out


PAD_LENGTHS = [0, 1, 2, 27, 28, 29, 31, 32, 33, 59, 60, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5]


def test_padding_and_alignment(eng):
    pcms = odd_views(PAD_LENGTHS, 7)
    plain = J.flac_encode(pcms, 48000)
    streams = J.flac_encode(pcms, 48000, md5=True)
    digests = J.flac_md5(pcms)
    for n, x, p, s, d in zip(PAD_LENGTHS, pcms, plain, streams, digests):
        want = md5_of(x)
        meta, plain_form = split(s)
        assert meta["md5"] == want, n
        assert d == want, n
        assert plain_form == p, n
        assert meta["streaminfo_last"] and meta["points"] is None and len(s) == len(p)
        got, _, _ = check(s)
        assert got.tobytes() == x.tobytes(), n
    # the same lengths the other way round: every utterance at another offset of the device slab
    rev = J.flac_md5(pcms[::-1])
    assert rev == [md5_of(x) for x in pcms[::-1]]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_lanes_and_waves(eng, count):
    rng = np.random.default_rng(count)
    lengths = [int(v) for v in rng.integers(0, 20001, count)]
    lengths[rng.integers(0, count)] = 0
    lengths[rng.integers(0, count)] = 20000
    pcms = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lengths]
    want = [md5_of(x) for x in pcms]
    assert J.flac_md5(pcms) == want
    streams = J.flac_encode(pcms, 22050, block_size=1152, max_lpc_order=0, md5=True)
    assert [split(s)[0]["md5"] for s in streams] == want


@pytest.mark.parametrize("bs,frames,hz", [(16, 131, 8000), (4096, 5, 48000)])
def test_seek_table(eng, bs, frames, hz):
    n = (frames - 1) * bs + 5  # (at 8 kHz a block of 16 is 2 ms: an interval of 1 ms rounds to a step of 1)
    t = np.arange(n)
    x = np.round(9000 * np.sin(2 * np.pi * 313 * t / hz) + 2000 * np.sin(2 * np.pi * 5100 * t / hz)).astype(np.int16)
    (plain,) = J.flac_encode([x], hz, block_size=bs, max_lpc_order=8)
    block_ms = 1000.0 * bs / hz
    seen = set()
    for ms in (1, max(2, round(3 * block_ms)), 10 ** 7):  # a step of 1, a step above 1, one point only
        step, points, hdr = J.flac_seek_geometry(n, bs, hz, ms)
        seen.add("one" if points == 1 else "step1" if step == 1 else "above")
        for md5 in (False, True):
            (s,) = J.flac_encode([x], hz, block_size=bs, max_lpc_order=8, md5=md5, seek_interval_ms=ms)
            got, info, meta = check(s)  # every point against the decoded frames; sync and frame number at its offset
            assert got.tobytes() == x.tobytes() and info["frames"] == frames
            assert len(meta["points"]) == points and meta["header_bytes"] == hdr
            assert [p[0] for p in meta["points"]] == [f * bs for f in range(0, frames, step)]
            assert not meta["streaminfo_last"] and meta["seektable_last"]
            assert meta["md5"] == (md5_of(x) if md5 else bytes(16))
            assert s[hdr:] == plain[42:]  # the frames do not change
            assert split(s)[1] == plain
    assert seen == {"one", "step1", "above"}
    # no frames: no table, STREAMINFO stays last
    (e,) = J.flac_encode([np.zeros(0, dtype=np.int16)], hz, block_size=bs, md5=True, seek_interval_ms=100)
    meta, _ = split(e)
    assert len(e) == 42 and meta["streaminfo_last"] and meta["points"] is None and meta["md5"] == md5_of([])


def _utts(eng, frames, seed):
    tab = synth.VoiceTables(eng)
    return eng.voice_info(), [synth.synth_utterance(tab, T, seed + T) for T in frames]


def batch_streams(b, opts=None):
    """Every utterance, both requests on: the digest is hashlib's of pcm_i16(u), the stream is the seam's on that PCM
    and verifies against it in the test decoder."""
    opts = opts or {}
    streams = b.flac_all()
    for i in range(len(b)):
        pcm, hz = b.pcm_i16(i), b.output_rate(i)
        assert b.flac(i) == streams[i]
        meta, _ = split(streams[i])
        assert meta["md5"] == md5_of(pcm), i
        (ref,) = J.flac_encode([pcm], hz, md5=True, seek_interval_ms=SEEK_MS, **opts)
        assert ref == streams[i], i
        got, info, meta = check(streams[i])
        assert got.tobytes() == pcm.tobytes() and info["rate"] == hz
        step, points, hdr = J.flac_seek_geometry(pcm.size, opts.get("block_size") or 4096, hz, SEEK_MS)
        assert len(meta["points"] or []) == points and meta["header_bytes"] == hdr
    return streams


def test_ragged_batch(eng):
    vi, utts = _utts(eng, (300, 1, 777, 60, 1500), 11)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_flac(md5=True, seek_interval_ms=SEEK_MS)
        b.run()
        batch_streams(b)


@pytest.mark.parametrize("rates,target", [((22050, 16000, 0), -23.0)])
def test_rates_and_targets(eng, rates, target):
    vi, utts = _utts(eng, (500, 900, 240), 5)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_output_rate(list(rates))
        b.set_loudness_target(target, 0.0)
        b.set_flac(block_size=1152, max_lpc_order=12)
        b.set_flac_meta(md5=True, seek_interval_ms=SEEK_MS)
        b.run()
        batch_streams(b, opts={"block_size": 1152, "max_lpc_order": 12})
        assert any(b.pcm_i16(i).size % 2 for i in range(len(b)))  # odd lengths: later utterances start on odd samples


def test_redo_rounds_hash_the_final_pcm(eng):
    vi, utts = _utts(eng, (600, 1100), 40)
    with J.Batch(vi, utts, pcm_i16=True, chunk_frames=96, warmup_frames=2, verify_tol=1e-12) as b:
        b.set_loudness_target(-20.0, math.inf)
        b.set_flac(md5=True, seek_interval_ms=SEEK_MS)
        b.run()
        b.sync()
        assert b.info()["n_redo"] > 0
        batch_streams(b)


def test_gang_timeout(eng):
    vi, utts = _utts(eng, (400, 700, 90), 21)
    with J.Batch(vi, utts, pcm_i16=True, test_gang_timeout=True) as b:
        b.set_flac(md5=True, seek_interval_ms=SEEK_MS)
        b.run()
        batch_streams(b)


def test_invariance_alone_and_among_64(eng):
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    res = []
    for utts, pos in (([probe], 0), (others[:20] + [probe] + others[20:], 20), (others + [probe], 63)):
        with J.Batch(vi, utts, pcm_i16=True, fast_invariant=True) as b:
            b.set_flac(md5=True, seek_interval_ms=SEEK_MS)
            b.run()
            res.append(b.flac(pos))
            if pos == 63:
                assert split(res[-1])[0]["md5"] == md5_of(b.pcm_i16(pos))
    assert res[0] == res[1] == res[2]
    assert split(res[0])[0]["points"]


def test_engine_entries(eng):
    kw = {"md5": True, "seek_interval_ms": SEEK_MS}
    data = eng.synthesize_flac(SAMPLE_SENTENCE_1, **kw)
    (pcm,) = eng.synthesize_batch([SAMPLE_SENTENCE_1], i16=True)
    got, info, meta = check(data)
    assert got.tobytes() == pcm.tobytes() and meta["md5"] == md5_of(pcm) and meta["points"]
    assert split(data)[1] == eng.synthesize_flac(SAMPLE_SENTENCE_1)
    e2 = eng.clone()
    e2.condition.set_output_sampling_frequency(22050)
    e2.condition.set_loudness_target(-18.0)
    out = J.synthesize_batch_each_flac([eng, e2], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], block_size=2304, **kw)
    ref = J.synthesize_batch_each([eng, e2], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2], i16=True)
    for data, p, hz in zip(out, ref, (48000, 22050)):
        got, info, meta = check(data)
        assert got.tobytes() == p.tobytes() and info["rate"] == hz and info["block_size"] == 2304
        assert meta["md5"] == md5_of(p)
        assert len(meta["points"]) == J.flac_seek_geometry(p.size, 2304, hz, SEEK_MS)[1]
    (b2,) = e2.synthesize_batch_flac([SAMPLE_SENTENCE_2], **kw)
    got, info, meta = check(b2)
    assert got.tobytes() == ref[1].tobytes() and meta["md5"] == md5_of(ref[1]) and info["rate"] == 22050


def test_rules(eng):
    vi, utts = _utts(eng, (100,), 1)
    with J.Batch(vi, utts, pcm_i16=True) as b:
        with pytest.raises(J.JbError):
            b.set_flac_meta(md5=True)  # before set_flac
        b.set_flac()
        b.set_flac_meta(md5=True, seek_interval_ms=SEEK_MS)
        b.run()
        with pytest.raises(J.JbError):
            b.set_flac_meta(md5=True)  # after a run
        assert split(b.flac(0))[0]["md5"] == md5_of(b.pcm_i16(0))
    with J.Batch(vi, utts, pcm_i16=True) as b:  # without the request: today's stream
        b.set_flac()
        b.run()
        meta, plain = split(b.flac(0))
        assert plain == b.flac(0) and meta["md5"] == bytes(16) and meta["streaminfo_last"]
