"""The mix stage on the GPU (jb_mix.hip): the device seam against the host seam bit for bit (the host seam is held to
the numpy statement of the rule by tests/test_mix_abi.py) over join-shaped requests, every misalignment of source
against destination under overlap, depths, segment boundaries around tile edges, fades, gains and the fit; then the
stage in a batch -- from f64 and from the 16-bit sink, behind the converter and the loudness apply pass -- with FLAC, the
sample format, IMA ADPCM and the feature stages encoding mixtures; redo rounds; the fast invariant mode; the engine
path; the example; and the batch without a request.  Every comparison is bit-exact unless it says otherwise."""
import hashlib
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi, synth
from tests import join_ref as R
from tests import mix_ref as M
from tests.conftest import VOICE
from tests.flac_meta_ref import check as flac_check
from tests.flac_meta_ref import split as flac_split
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE = {np.dtype(np.float64): 2048, np.dtype(np.int16): 8192}  # samples of a workgroup's tile (16 KiB)
NINF = -math.inf
LENGTHS = [0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097]  # tests/test_gpu_join.py's
PADS = [0, 1, 3, 4097]


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


def pcm_of(n, seed, dtype):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 9000.0 + 0.25
    if n > 6:
        x[:3] = [32767.0, -32768.0, 12345.678]
        x[-3:] = [-1.0, 1.0, -32768.0]
    return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) if dtype == np.int16 else x


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def ceiling(db):
    return 32768.0 * math.pow(10.0, db / 20.0)


def check_seam(pcms, req, fit=False, ceiling_db=0.0):
    """The device against jb_mix_host: the programmes, the geometry's counts, and the peak (a maximum: the same bits).
    With fit the output is the host rule under the device's scale, and the device's scale is the host's within 2^-50
    relative (the deviation is returned)."""
    opts = _ffi.mix_opts(fit, ceiling_db)
    got, reps = J.mix_pcm(pcms, req, opts)
    want, wreps = J.mix_host(pcms, req, opts, [r.scale for r in reps] if fit else None)
    assert len(got) == len(want)
    dev = 0.0
    for p, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (p, g.size, w.size, np.flatnonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[:8])
        assert (reps[p].peak, reps[p].depth, reps[p].overlap) == (wreps[p].peak, wreps[p].depth, wreps[p].overlap), p
    if fit:
        _, hreps = J.mix_host(pcms, req, opts)
        for r, h in zip(reps, hreps):
            assert (r.scale == 1.0) == (h.scale == 1.0)
            dev = max(dev, abs(r.scale - h.scale) / h.scale)
        print("largest relative deviation of the device's scale from the host's:", dev)
        assert dev <= 2.0 ** -50
    else:
        assert all(r.scale == 1.0 for r in reps)
    return got, reps


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_join_shaped_requests_equal_the_join(dtype):
    lengths = LENGTHS + LENGTHS[::-1]
    pcms = [pcm_of(n, 31 * u + n, dtype) for u, n in enumerate(lengths)]

    def fades(n):
        return [0, 1, 2, n, n + 5]
    req = [(0, PADS[u % 4], PADS[(u // 4) % 4], fades(n)[u % 5], fades(n)[(u + 2) % 5]) for u, n in enumerate(lengths)]
    for r in (req, [(None,) + q[1:] for q in req]):
        want = J.join_pcm(pcms, r)
        got, reps = check_seam(pcms, M.from_join(r, lengths))
        assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
        assert all(rep.depth <= 1 for rep in reps)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_every_source_offset_against_every_destination_offset_of_an_overlapping_pair(dtype):
    """The seam packs its inputs one after the other.  A member of d samples in front shifts the source of the first of
    the pair to offset d, its start d + k its destination to d + k; the second's source lies at d + k, its start,
    inside the first, at 2 d + k: over all k and d each of the two meets every source offset against every
    destination offset within 16 bytes (asserted from the geometry).  A filler behind each triple keeps the next
    triple's sources on a 16-byte boundary."""
    per = 16 // np.dtype(dtype).itemsize
    pcms, req = [], []
    for k in range(per):
        for d in range(per):
            p = len(req) // 4
            triple = [pcm_of(d, d, dtype), pcm_of(k + 4 * per, k, dtype), pcm_of(3 * per + 5, 100 + 8 * k + d, dtype)]
            pcms += triple + [pcm_of(-sum(x.size for x in triple) % per, 7, dtype)]
            req += [(p, 0, 0.0), (p, d + k, 0.0, 0, 2, 3), (p, d + k + per + d, -6.5, 2, 3, 4), (None, 0)]
    check_seam(pcms, req)
    lengths = [x.size for x in pcms]
    src = np.cumsum([0] + lengths[:-1])
    for m in (1, 2):
        pairs = {(int(src[i] % per), int(req[i][1] % per)) for i in range(m, len(req), 4)}
        assert len(pairs) == per * per


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_depths_starts_and_containment(dtype):
    per = 16 // np.dtype(dtype).itemsize
    t = TILE[np.dtype(dtype)]
    for depth in (1, 2, 3, 9):  # nine: more than anything unrolled
        pcms = [pcm_of(t + 100 + 7 * u, 50 + u, dtype) for u in range(depth)]
        _, reps = check_seam(pcms, [(0, 3 * u, -3.0 * u, 0, 5 * u, 9) for u in range(depth)])
        assert reps[0].depth == depth
    # identical starts
    pcms = [pcm_of(500 + u, u, dtype) for u in range(4)]
    _, reps = check_seam(pcms, [(0, 77, 0.0), (0, 77, -6.5), (0, 77, 12.0, 0, 40, 40), (0, 77)])
    assert reps[0].depth == 4 and reps[0].overlap == 502  # (the second longest ends the overlap)
    # a member wholly inside another, and members of 0, 1 and one group minus 1 samples inside an overlap
    for inner in (0, 1, per - 1, 300):
        pcms = [pcm_of(1000, 1, dtype), pcm_of(inner, 2, dtype), pcm_of(600, 3, dtype)]
        _, reps = check_seam(pcms, [(0, 5, 0.0), (0, 333, -6.5, 0, 2, 2), (0, 200, 12.0)])
        assert reps[0].depth == (3 if inner else 2)
    # out of start order: the sum's order is the utterance index, not the start
    pcms = [pcm_of(900, 1, dtype) * 3, pcm_of(900, 2, dtype), pcm_of(900, 3, dtype) * 5]
    check_seam(pcms, [(0, 600, -0.1), (0, 0, 0.1), (0, 300, -0.2)])


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_segment_boundaries_around_a_tile_edge(dtype):
    t = TILE[np.dtype(dtype)]
    per = 16 // np.dtype(dtype).itemsize
    # a second member starting, and a first one ending, exactly on the tile edge and one sample to either side
    for edge in (t, t - 1, t + 1, 2 * t, t - per, t + per):
        pcms = [pcm_of(edge, 5, dtype), pcm_of(t // 2 + 3, 6, dtype), pcm_of(2 * t + 9, 7, dtype)]
        check_seam(pcms, [(0, 0, 0.0, 0, 5, 5), (0, edge - 7, -6.5, 0, 9, 9), (0, edge, 12.0)])
        check_seam(pcms, [(0, 0, 0.0, 0, 5, 5), (0, edge, -6.5, 0, 9, 9), (0, 3, 12.0)])
    # a programme's last partial group under depth 2
    for tail in range(1, per):
        pcms = [pcm_of(t + tail, 8, dtype), pcm_of(4 * per + tail, 9, dtype)]
        check_seam(pcms, [(0, 0, 0.0), (0, t - 4 * per, -6.5)])
    # fades longer than a tile under overlap
    pcms = [pcm_of(3 * t + 1, 8, dtype), pcm_of(3 * t - 5, 9, dtype)]
    check_seam(pcms, [(0, 1, 0.0, 1, 2 * t + 3, t + 9), (0, 40, -6.5, 0, t + 9, 2 * t + 3)])


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_crossfade_muted_members_gains_and_shapes(dtype):
    # two fades crossing, with fade_in + fade_out > n
    n = 700
    pcms = [pcm_of(n, 1, dtype), pcm_of(n, 2, dtype)]
    _, reps = check_seam(pcms, [(0, 0, 0.0, 0, 400, 400), (0, n - 400, 0.0, 0, 400, 400)])
    assert reps[0].overlap == 400
    # a muted member extending the length; gains of 0, -6.5 and +12 dB
    pcms = [pcm_of(300, 3, dtype), pcm_of(5000, 4, dtype), pcm_of(200, 5, dtype), pcm_of(250, 6, dtype)]
    (got,), reps = check_seam(pcms, [(0, 10, 0.0), (0, 0, NINF, 11), (0, 100, -6.5), (0, 150, 12.0)])
    assert got.size == 5011 and reps[0].depth == 3 and not got[400:].any()
    # 64 programmes of one, one programme of 64, an empty call
    pcms = [pcm_of(50 + 13 * u, u, dtype) for u in range(64)]
    assert len(check_seam(pcms, [(None, u % 3, -0.5 * (u % 4), u % 5, 4, 4) for u in range(64)])[0]) == 64
    got, reps = check_seam(pcms, [(7, 11 * u, -0.5 * (u % 4), u % 5, 4, 4) for u in range(64)])
    assert len(got) == 1 and reps[0].depth > 3
    assert check_seam([], []) == ([], [])
    # a programme of empty members and pads alone
    (z,), _ = check_seam([np.zeros(0, dtype)] * 3, [(0, 2, 0.0, 3)] * 3)
    assert z.size == 5 and not z.any()


def test_seam_keeps_the_bits_of_a_copied_f64_sample():
    x = np.arange(64, dtype=np.float64)
    x[5] = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
    x[6], x[7], x[8] = -0.0, 5e-324, -np.inf
    (got,), _ = check_seam([x], [(None, 3, 0.0, 0, 2, 2)])
    assert got[3 + 2:3 + 62].tobytes() == x[2:62].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_fit(dtype):
    t = TILE[np.dtype(dtype)]
    loud = [pcm_of(2 * t + 77, 1, dtype), pcm_of(t + 5, 2, dtype), pcm_of(900, 3, dtype)]
    quiet = [pcm_of(400, 4, dtype), pcm_of(300, 5, dtype)]
    req = [(0, 0, 6.0, 0, 10, 10), (0, t - 3, 3.0), (0, 50, 0.0), (1, 0, -30.0), (1, 10, -30.0, 3)]
    for db in (-1.0, -6.0):
        got, reps = check_seam(loud + quiet, req, True, db)
        plain, preps = check_seam(loud + quiet, req)
        c = ceiling(db)
        assert reps[0].peak > c and reps[0].scale < 1.0  # driven over the ceiling
        assert np.max(np.abs(got[0].astype(np.float64))) <= c
        assert reps[1].scale == 1.0 and same(got[1], plain[1])  # under the ceiling: the no-fit bytes
        # the reported peak is the largest |sum| of the unscaled f64 sum, with and without the flag
        _, sums, _, _, _ = M.mix(loud + quiet, req, [J.mix_gain(r[2]) for r in M.norm(req)])
        for p in range(2):
            assert reps[p].peak == preps[p].peak == np.max(np.abs(sums[p]))
    if dtype == np.int16:  # the 16-bit form scales in front of the sink: 2 x 30000 under -6 dBFS, not the clamp's 32767
        big = np.full(t + 9, 30000, dtype=np.int16)
        (got,), (rep,) = check_seam([big, big], [(0, 0), (0, 0)], True, -6.0)
        assert rep.peak == 60000.0 and got.tolist() == [int(min(60000.0 * rep.scale, ceiling(-6.0)))] * big.size


# ---- 2. the batch path ----------------------------------------------------------------------------------------------
FRAMES6 = (7, 1, 40, 3, 12, 5)
# (programme, start, gain_db, pad_after, fade_in, fade_out): programme 0 = {0, 2, 4} three deep, programme 1 = {1, 3}
MIX6 = [(0, 4097, 0.0, 3, 240, 240), (1, 1, -6.5, 0, 0, 7), (0, 0, -3.0, 5), (1, 100, 0.0, 9, 3, 0),
        (0, 5000, 2.0, 11, 5, 99999), (None, 2, 0.0, 4, 1, 1)]


@pytest.fixture(scope="module")
def utts6(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 3 + t) for t in FRAMES6]


def member_pcm(b, i16):
    return [b.pcm_i16(u) if i16 else b.pcm(u) for u in range(len(b))]


def gains_of(req):
    return [J.mix_gain(r[2]) for r in M.norm(req)]


def check_programmes(b, i16, req, fit=False, ceiling_db=0.0):
    """programme_pcm(p) is mix_ref of the PCM the same batch hands out (with fit: under the device's scale, which is
    the rule's within 2^-50 relative); the layout entries and the report agree."""
    pcms = member_pcm(b, i16)
    gains = gains_of(req)
    reps = [b.mix_report(p) for p in range(b.num_outputs())]
    want, sums, peaks, scales, prog_of = M.mix(pcms, req, gains, fit, ceiling(ceiling_db),
                                               [r.scale for r in reps] if fit else None)
    _, _, ns, depth, overlap = M.geometry([x.size for x in pcms], req, gains)
    assert b.num_outputs() == len(want)
    assert [b.programme_of(u) for u in range(len(b))] == prog_of
    assert [b.member_start(u) for u in range(len(b))] == [r[1] for r in M.norm(req)]
    got = []
    for p, w in enumerate(want):
        members = [u for u in range(len(b)) if prog_of[u] == p]
        assert b.programme_layout(p) == (len(members), w.size, b.output_rate(members[0]))
        got.append(b.programme_pcm(p))
        assert same(got[p], w.astype(np.int16 if i16 else np.float64)), p
        assert (reps[p].peak, reps[p].depth, reps[p].overlap) == (peaks[p], depth[p], overlap[p]), p
        rule = ceiling(ceiling_db) / peaks[p] if fit and peaks[p] > ceiling(ceiling_db) else 1.0
        assert (reps[p].scale == 1.0) == (rule == 1.0) and abs(reps[p].scale - rule) / rule <= 2.0 ** -50, p
    return got


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("chain", ["native", "rate", "loudness", "both"])
def test_batch_programmes_are_the_mix_of_the_batch_pcm(eng, utts6, i16, chain):
    vi, utts = utts6
    with J.Batch(vi, utts, pcm_i16=i16) as b:
        if chain in ("rate", "both"):
            b.set_output_rate(44100)  # 48 kHz -> 44.1 kHz: odd lengths
        if chain in ("loudness", "both"):
            b.set_loudness_target(-20.0, -1.0)
        b.set_mix(MIX6, fit=True, ceiling_db=-3.0)
        # the geometry answers before the run
        assert b.num_outputs() == 3 and b.programme_of(4) == 0 and b.member_start(0) == 4097
        assert b.programme_layout(2)[:2] == (1, 2 + b.num_samples(5) + 4)
        with pytest.raises(J.JbError, match="has not run"):
            b.programme_pcm(0)
        with pytest.raises(J.JbError, match="has not run"):
            b.mix_report(0)
        b.run()
        if chain in ("rate", "both"):
            assert any(b.num_samples(u) % 2 for u in range(6))
        check_programmes(b, i16, MIX6, True, -3.0)
        assert b.mix_report(0).depth == 3 and b.mix_report(1).depth == 2


# ---- 3. the encoders and the feature stages take mixtures -----------------------------------------------------------
def md5_of(pcm):
    return hashlib.md5(np.ascontiguousarray(pcm, dtype="<i2").tobytes()).digest()


def check_flac(b, progs, hz, decode=True, **opts):
    streams = J.flac_encode(progs, hz, **opts)
    every = b.flac_all()
    assert len(every) == len(progs)
    for p, x in enumerate(progs):
        s = b.flac(p)
        assert s == every[p] == streams[p], p  # byte for byte the seam's stream of those samples
        if not decode:
            assert flac_split(s)[0]["md5"] == md5_of(x) and flac_split(s)[0]["total"] == x.size
            continue
        dec, _, meta = flac_check(s)  # decodes, and every seek point verifies
        assert np.array_equal(dec, x) and meta["total"] == x.size and meta["rate"] == hz
        assert meta["md5"] == md5_of(x)


def test_flac_streams_of_mixtures(eng, utts6):
    vi, utts = utts6
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_mix(MIX6)
        b.set_flac(block_size=1152, md5=True, seek_interval_ms=20)
        b.run()
        progs = check_programmes(b, True, MIX6)
        check_flac(b, progs, vi.sampling_frequency, block_size=1152, md5=True, seek_interval_ms=20)
        assert len(b.pcm_all()) == 6  # the per-utterance PCM entries keep handing out utterances: the stems


def test_formatted_adpcm_and_features_of_mixtures(eng, utts6):
    vi, utts = utts6
    hz = vi.sampling_frequency
    fo, mo = J.fbank(center=True), J.mfcc(delta_order=2, cmvn="mean_var")
    ml = J.melspec(n_fft=1200, hop=480, log="log10", range=8.0, f64=True)
    with J.Batch(vi, utts) as b:
        b.set_mix(MIX6)
        b.set_format("s16", dither=True, seed=77)  # TPDF: the dither index runs over the mixture
        b.set_adpcm()
        b.set_fbank(fo)
        b.set_mfcc(mo, fbank=fo)
        b.set_melspec(ml)
        b.run()
        progs = check_programmes(b, False, MIX6)
        for p, x in enumerate(progs):
            assert b.formatted(p) == J.format_pcm_host(x, "s16", True, 77), p
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, hz), p
            assert np.array_equal(b.read_fbank(p), J.fbank_pcm(x, hz, fo)), p
            assert np.array_equal(b.read_mfcc(p), J.mfcc_pcm(x, hz, fo, mo)), p  # the CMVN runs over the mixture
            assert np.array_equal(b.read_melspec(p), J.melspec_pcm(x, hz, ml)), p  # ... and so does the clamp


# ---- 4. redo rounds -------------------------------------------------------------------------------------------------
REDO_MIX = [(0, 100, 0.0, 0, 48, 48), (1, 3, -2.0, 5, 48, 48), (0, 2400, 3.0, 7, 48, 48), (1, 1000, 0.0, 0, 48, 48)]


@pytest.mark.parametrize("i16", [False, True])
def test_redo_rounds_leave_no_stale_mixture(eng, tab, i16):
    """tests/test_gpu_join.py's recipe: every hand-off of the long members fails, so redo rounds rewrite them behind the
    first mix; the loudness group {1, 2} spans both programmes, so utterance 1 changes its gain with utterance 2's redo.
    A touched programme runs again whole, the peak and the fit included."""
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (400, 90, 600, 30)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        b.set_loudness_target(-21.0, math.inf)
        b.set_loudness_groups([None, 0, 0, None])
        b.set_mix(REDO_MIX, fit=True, ceiling_db=-12.0)
        if i16:
            b.set_flac(md5=True, seek_interval_ms=50)
        else:
            b.set_format("s24", dither=True, seed=5)
        b.set_adpcm()
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 1 and sum(b.redo_stats()) >= 1
        progs = check_programmes(b, i16, REDO_MIX, True, -12.0)  # recomputed from the final per-utterance PCM
        assert any(b.mix_report(p).scale < 1.0 for p in range(2))
        hz = vi.sampling_frequency
        for p, x in enumerate(progs):
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, hz), p
            if not i16:
                assert b.formatted(p) == J.format_pcm_host(x, "s24", True, 5), p
        if i16:
            check_flac(b, progs, hz, decode=False, md5=True, seek_interval_ms=50)


# ---- 5. invariance --------------------------------------------------------------------------------------------------
def test_mixture_alone_and_among_64(eng, tab):
    vi = eng.voice_info()
    probe = [synth.synth_utterance(tab, T, 77 + T) for T in (300, 40, 210)]
    others = [synth.synth_utterance(tab, 50 + 7 * k, 1000 + k) for k in range(64)]
    req = [(0, 1000, 0.0, 3, 100, 100), (0, 30000, -6.5, 2401, 100, 100), (0, 5, 3.0, 7, 100, 100)]
    one = (None, 1, 0.0, 1)
    res = []
    for utts, r, p in ((probe, req, 0),
                       (others[:20] + probe[:1] + others[20:50] + probe[1:] + others[50:],
                        [one] * 20 + req[:1] + [one] * 30 + req[1:] + [one] * 14, 20)):
        with J.Batch(vi, utts, fast_invariant=True, pcm_i16=True) as b:
            b.set_mix(r, fit=True, ceiling_db=-9.0)
            b.set_flac(md5=True)
            b.run()
            assert b.programme_layout(p)[0] == 3
            rep = b.mix_report(p)
            res.append((b.programme_pcm(p).tobytes(), b.flac(p), rep.peak, rep.scale, rep.depth, rep.overlap))
    assert res[0] == res[1] and res[0][4] == 3


# ---- 6. the engine path ---------------------------------------------------------------------------------------------
SENTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
PLACE = [(0.0, 0.0), (350.0, -6.5), (120.25, 3.0)]
OPTS = dict(lead_ms=12.5, trail_ms=3.3, fade_ms=5.0)


def engine_request(lengths, hz):
    f = R.ms_to_samples(OPTS["fade_ms"], hz)
    return [(0, R.ms_to_samples(OPTS["lead_ms"] + ms, hz), db, R.ms_to_samples(OPTS["trail_ms"], hz), f, f)
            for (ms, db), _ in zip(PLACE, lengths)]


def test_engine_programme_mix(eng):
    e = eng.clone()
    hz = e._out_hz()
    parts = e.synthesize_batch(SENTS)
    parts16 = e.synthesize_batch(SENTS, i16=True)
    req = engine_request(parts, hz)
    gains = gains_of(req)
    e.set_programme_mix(PLACE, fit=True, ceiling_db=-2.0)
    place, fit, cdb = e.get_programme_mix()
    assert place == PLACE and fit and cdb == -2.0
    (want,), _, peaks, scales, _ = M.mix(parts, req, gains, True, ceiling(-2.0))
    (want16,), _, _, _, _ = M.mix(parts16, req, gains, True, ceiling(-2.0))
    got, starts = e.synthesize_programme(SENTS, **OPTS)
    assert same(got, want) and starts == [r[1] for r in req]
    got16, starts16 = e.synthesize_programme(SENTS, sink="i16", **OPTS)
    assert same(got16, want16) and starts16 == starts
    stream, _ = e.synthesize_programme(SENTS, sink="flac", md5=True, seek_interval_ms=100, **OPTS)
    dec, _, meta = flac_check(stream)
    assert np.array_equal(dec, want16) and meta["md5"] == md5_of(want16) and meta["rate"] == hz
    ml = J.melspec(n_fft=1200, hop=480, log="log10", range=8.0, f64=True)
    feats, _ = e.synthesize_programme(SENTS, sink="melspec", opts=ml, **OPTS)
    assert np.array_equal(feats, J.melspec_pcm(want, hz, ml))
    # another utterance count, a gap, a bad place
    with pytest.raises(J.JbError, match="places 3 utterances, the call has 2"):
        e.synthesize_programme(SENTS[:2], **OPTS)
    with pytest.raises(J.JbError, match="gap_ms must be 0"):
        e.synthesize_programme(SENTS, gap_ms=1.0, **OPTS)
    for bad in ([(-1.0, 0.0)], [(math.nan, 0.0)], [(0.0, 41.0)]):
        with pytest.raises(J.JbError):
            e.set_programme_mix(bad)
    assert e.get_programme_mix()[0] == PLACE  # a refused call changes nothing
    # withdrawn: the join of today; the convenience form sets and puts back
    e.set_programme_mix(None)
    assert e.get_programme_mix() == (None, False, 0.0)
    joined, _ = e.synthesize_programme(SENTS, **OPTS)
    (jwant,), _, _ = R.join(parts, R.chapter([x.size for x in parts], hz, **OPTS))
    assert same(joined, jwant)
    again, _ = e.synthesize_programme(SENTS, mix=PLACE, fit=True, ceiling_db=-2.0, **OPTS)
    assert same(again, want) and e.get_programme_mix()[0] is None


def test_mixture_example(tmp_path):
    out = tmp_path / "mixture.flac"
    labs = []
    for k, s in enumerate(SENTS):
        p = tmp_path / f"s{k}.lab"
        p.write_text("\n".join(s) + "\n")
        labs.append(str(p))
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "mixture.py"), str(VOICE), *labs, "-o", str(out),
                        "--start-ms", "0,400,150", "--gain-db", "0,-6,-3", "--fit"], capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    dec, _, meta = flac_check(out.read_bytes())
    assert dec.size == meta["total"] > 0 and meta["md5"] == md5_of(dec)
    cues = [ln for ln in r.stdout.splitlines() if ln.startswith("cue ")]
    assert len(cues) == 3 and cues[0].split()[2] == "0"
    assert any(ln.startswith("report ") for ln in r.stdout.splitlines())


# ---- 7. without the request, and the two requests side by side ------------------------------------------------------
def test_default_unchanged_and_rules(eng, utts6):
    vi, utts = utts6
    join6 = [(0, 4097, 3, 240, 240), (1, 1, 0, 0, 7), (0, 0, 5, 0, 0), (1, 7, 9, 3, 0), (0, 0, 11, 5, 99999), (None, 2, 4, 1, 1)]
    with J.Batch(vi, utts) as b:
        b.run()
        plain, info, kinfo = [x.tobytes() for x in member_pcm(b, False)], b.info(), b.kernel_info()
        with pytest.raises(J.JbError, match="was not called"):
            b.mix_report(0)
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_mix(MIX6)
    with J.Batch(vi, utts) as b:  # a request made and withdrawn: the batch of today, the encoders by utterance
        b.set_mix(MIX6, fit=True, ceiling_db=-1.0)
        b.set_mix(None)
        b.set_adpcm()
        b.run()
        assert b.num_outputs() == 6 and len(b.read_adpcm_all()) == 6 and b.programme_of(0) == -1
        assert [x.tobytes() for x in member_pcm(b, False)] == plain and b.info() == info and b.kernel_info() == kinfo
        with pytest.raises(J.JbError, match="was not called"):
            b.mix_report(0)
    with J.Batch(vi, utts) as b:  # with the request the members' PCM and the vocoder's work items stay as they were
        b.set_mix(MIX6)
        b.run()
        assert [x.tobytes() for x in member_pcm(b, False)] == plain and b.info() == info and b.kernel_info() == kinfo
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError, match="no PCM"):
            b.set_mix(MIX6)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one request per utterance"):
            b.set_mix(MIX6[:5])
        with pytest.raises(J.JbError, match="programme id 6"):
            b.set_mix([(6,)] + MIX6[1:])
        with pytest.raises(J.JbError, match="gain_db.*utterance 2"):
            b.set_mix(MIX6[:2] + [(0, 0, 40.5)] + MIX6[3:])
        with pytest.raises(J.JbError, match="ceiling_db"):
            b.set_mix(MIX6, fit=True, ceiling_db=1.0)
        bad = _ffi.mix_request(MIX6)
        bad[2].reserved2 = 9
        assert J.lib().jb_batch_set_mix(b._h, bad, 6, None) == -1 and b"reserved" in J.lib().jb_last_error()
        assert b.num_outputs() == 6
        # a batch holds a join or a mix request: the second setter is refused and changes nothing
        b.set_join(join6)
        with pytest.raises(J.JbError, match="holds a join request"):
            b.set_mix(MIX6)
        assert b.member_start(2) == 4097 + b.num_samples(0) + 3  # (still the join's geometry)
        b.set_join(None)
        b.set_mix(MIX6)
        with pytest.raises(J.JbError, match="holds a mix request"):
            b.set_join(join6)
        assert b.member_start(2) == 0 and b.num_outputs() == 3
        b.set_mix(None)
        # a programme of mixed rates is refused by whichever setter comes second, and changes nothing
        b.set_output_rate([8000, 0, 16000, 0, 8000, 0])
        with pytest.raises(J.JbError, match="programme 0 would disagree on the output rate"):
            b.set_mix(MIX6)
        assert b.num_outputs() == 6
        b.set_output_rate([8000, 0, 8000, 0, 8000, 0])
        b.set_mix(MIX6)
        with pytest.raises(J.JbError, match="programme 1 would disagree on the output rate"):
            b.set_output_rate([8000, 0, 8000, 16000, 8000, 0])
        assert [b.output_rate(u) for u in range(6)] == [8000, vi.sampling_frequency] * 3
        assert b.programme_layout(0)[2] == 8000 and b.num_outputs() == 3
