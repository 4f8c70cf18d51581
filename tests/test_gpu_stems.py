"""The stems of a mix on the GPU (jb_mix.hip: k_mix's stem form, k_mix_levels and its fold): the device seam against
the host seam bit for bit (the host seam is held to the numpy statement of the rule by tests/test_stems_abi.py), f64 and
16-bit, with and without the fit -- talkers of several utterances with extents around tile edges, every misalignment of
source against destination, a stem of one member at 0 dB, a stem of muted members alone, a member of no stem, depth 9, a
fitted stem above the ceiling -- and the levels' three sums against jb_mix_levels_host; then the request in a batch:
the stems against the seam on the batch's own PCM, every encoder and feature stage over a stem, the programmes' outputs
byte for byte those of the batch without the request, the refusals, redo rounds, the fast invariant mode, and the batch
without the request.  Every comparison is bit-exact unless it says otherwise."""
import hashlib
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi, synth
from tests.conftest import VOICE
from tests.flac_meta_ref import check as flac_check
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.test_gpu_mix import LENGTHS, PADS

pytestmark = pytest.mark.gpu

TILE = {np.dtype(np.float64): 2048, np.dtype(np.int16): 8192}  # samples of a workgroup's tile (16 KiB)
NINF = -math.inf


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


def sums_of(r):
    return (r.e_s, r.d, r.e_p)


def check_levels(units, geo, sreps):
    """The device's three sums are jb_mix_levels_host's of the units it handed out, bit for bit; the dB values follow
    from them; a programme's E_p is the same whichever stem reports it"""
    e_p = {}
    for s, r in enumerate(sreps):
        u = geo["P"] + s
        p = geo["programme"][u]
        want = J.mix_levels_host(units[u], units[p], geo["first"][u], geo["end"][u])
        assert sums_of(r) == want, (s, sums_of(r), want)
        db = (r.level_db, r.sir_db, r.si_sdr_db)
        assert np.array_equal(db, J.mix_levels_db(*want), equal_nan=True), s
        assert e_p.setdefault(p, r.e_p) == r.e_p


def check_seam(pcms, req, stem_of, fit=False, ceiling_db=0.0):
    """The device against jb_mix_stems_host: the P + S units, the peaks (maxima: the same bits), the levels.  With fit
    the host runs under the device's scale (as tests/test_gpu_mix.py's check_seam), which is the rule's within 2^-50
    relative; a stem reports its programme's."""
    opts = _ffi.mix_opts(fit, ceiling_db)
    got, reps, sreps = J.mix_stems_pcm(pcms, req, stem_of, opts, levels=True)
    want, wreps, wsreps = J.mix_stems_host(pcms, req, stem_of, opts, [r.scale for r in reps] if fit else None,
                                           levels=True)
    geo = J.mix_stems_geometry(req, stem_of, [np.asarray(x).size for x in pcms])
    assert len(got) == len(want) == geo["U"] and len(reps) == len(wreps) == geo["P"] and len(sreps) == len(wsreps)
    for p, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (p, g.size, w.size, np.flatnonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[:8])
    for p, (r, w) in enumerate(zip(reps, wreps)):
        assert (r.peak, r.depth, r.overlap) == (w.peak, w.depth, w.overlap), p
    for s, (r, w) in enumerate(zip(sreps, wsreps)):
        assert r.peak == w.peak and r.scale == reps[geo["programme"][geo["P"] + s]].scale, s
        assert sums_of(r) == sums_of(w), s
    check_levels(got, geo, sreps)
    # the programmes are the plain mix's, bit for bit
    plain, preps = J.mix_pcm(pcms, req, opts)
    for p in range(geo["P"]):
        assert same(plain[p], got[p]) and (preps[p].peak, preps[p].scale) == (reps[p].peak, reps[p].scale), p
    if fit:
        _, hreps, _ = J.mix_stems_host(pcms, req, stem_of, opts)
        for r, h in zip(reps, hreps):
            assert (r.scale == 1.0) == (h.scale == 1.0) and abs(r.scale - h.scale) / h.scale <= 2.0 ** -50
    else:
        assert all(r.scale == 1.0 for r in reps)
    return got, reps, sreps


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_talkers_with_extents_around_tile_edges(dtype, fit):
    t = TILE[np.dtype(dtype)]
    # two talkers of two and three utterances: talker 0 begins one sample in front of a tile edge and ends on one,
    # talker 1 begins on one and ends one sample behind one
    pcms = [pcm_of(n, 20 + u, dtype) for u, n in enumerate([t // 2, t, t - 300, 100, t + 1 - 900])]
    req = [(0, t - 1, 0.0, 0, 9, 9), (0, t, -3.0, 5, 0, 40), (0, 2 * t + 300, 2.0), (0, 2 * t - 100, 6.0, 0, 64, 64),
           (0, 3 * t + 900, 1.5, 77)]
    _, _, _ = check_seam(pcms, req, [0, 1, 0, 1, 1], fit, -6.0)
    geo = J.mix_stems_geometry(req, [0, 1, 0, 1, 1], [x.size for x in pcms])
    assert (geo["first"][1], geo["end"][1]) == (t - 1, 3 * t) and (geo["first"][2], geo["end"][2]) == (t, 4 * t + 1)
    # three talkers of three, two and three utterances, over test_gpu_mix's lengths and pads; one utterance alone
    lengths = LENGTHS[1:] + [2 * t + 1]
    pcms = [pcm_of(n, 31 * u + n, dtype) for u, n in enumerate(lengths)]
    req = [(None if u == 9 else 0, (u * 811) % (t + 9) + PADS[u % 4], [0.0, -6.5, 3.0][u % 3], PADS[(u // 4) % 4],
            [0, 1, 2, n, n + 5][u % 5], [0, 1, 2, n, n + 5][(u + 2) % 5]) for u, n in enumerate(lengths)]
    check_seam(pcms, req, [u % 3 for u in range(10)], fit, -3.0)
    # extents that begin and end at a levels tile's edge - 1, 0, + 1
    for d in (-1, 0, 1):
        pcms = [pcm_of(1024 + d, 1, dtype), pcm_of(3000, 2, dtype)]
        check_seam(pcms, [(0, 1024 - d, 0.0), (0, 0, -2.0)], [0, 1], fit, -6.0)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_every_source_offset_against_every_destination_offset_of_a_stem_of_two(dtype):
    """tests/test_gpu_mix.py's construction: a member of d samples in front shifts the sources, the starts the
    destinations; here the overlapping pair is one stem and the member in front another, so the stem's own segments
    meet every source offset against every destination offset within 16 bytes (asserted from the geometry)."""
    per = 16 // np.dtype(dtype).itemsize
    pcms, req, stem_of = [], [], []
    for k in range(per):
        for d in range(per):
            p = len(req) // 4
            triple = [pcm_of(d, d, dtype), pcm_of(k + 4 * per, k, dtype), pcm_of(3 * per + 5, 100 + 8 * k + d, dtype)]
            pcms += triple + [pcm_of(-sum(x.size for x in triple) % per, 7, dtype)]
            req += [(p, 0, 0.0), (p, d + k, 0.0, 0, 2, 3), (p, d + k + per + d, -6.5, 2, 3, 4), (None, 0)]
            stem_of += [0, 1, 1, None]
    check_seam(pcms, req, stem_of)
    lengths = [x.size for x in pcms]
    src = np.cumsum([0] + lengths[:-1])
    for m in (1, 2):
        pairs = {(int(src[i] % per), int(req[i][1] % per)) for i in range(m, len(req), 4)}
        assert len(pairs) == per * per


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_shapes_of_stems(dtype):
    t = TILE[np.dtype(dtype)]
    # a stem that is one member at 0 dB: the member's bits outside its fades (the plain copy), zeros elsewhere
    x, y = pcm_of(t + 500, 1, dtype), pcm_of(2 * t, 2, dtype)
    if dtype == np.float64:
        x[40] = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
        x[41], x[42] = -0.0, 5e-324
    opts = None
    got, _, _ = J.mix_stems_pcm([x, y], [(0, 333, 0.0, 0, 8, 8), (0, 0, -1.0)], [1, 0], opts)
    assert got[1][333 + 8:333 + x.size - 8].tobytes() == x[8:-8].tobytes()
    assert not got[1][:333].any() and not got[1][333 + x.size:].any() and got[1].size == 2 * t
    if dtype == np.int16:
        check_seam([x, y], [(0, 333, 0.0, 0, 8, 8), (0, 0, -1.0)], [1, 0])
    # a stem of muted members only and one of an empty member: they exist, all +0.0, silent levels
    pcms = [pcm_of(900, 3, dtype), pcm_of(5000, 4, dtype), pcm_of(0, 5, dtype), pcm_of(700, 6, dtype)]
    got, _, sreps = check_seam(pcms, [(0, 10, 0.0), (0, 0, NINF, 11), (0, 100, -6.5), (0, 150, NINF)], [0, 1, 2, 1])
    assert len(got) == 4 and got[2].size == got[3].size == 5011 and not got[2].any() and not got[3].any()
    assert not np.signbit(got[2].astype(np.float64)).any()
    assert sums_of(sreps[1])[:2] == (0.0, 0.0) and sreps[1].level_db == -math.inf and sreps[1].peak == 0.0
    # a programme with a member of no stem, and one without any stem beside one with stems
    pcms = [pcm_of(1500 + 7 * u, 10 + u, dtype) for u in range(5)]
    got, _, _ = check_seam(pcms, [(0, 0, 0.0), (0, 500, -2.0), (0, 900, 1.0), (1, 0, 0.0), (1, 9, 0.0)],
                           [0, None, 0, None, None])
    assert len(got) == 3
    # depth 9: more than anything unrolled, as one stem, as two talkers, as nine stems
    pcms = [pcm_of(t + 100 + 7 * u, 50 + u, dtype) for u in range(9)]
    req = [(0, 3 * u, -3.0 * u, 0, 5 * u, 9) for u in range(9)]
    for stem_of in ([4] * 9, [u % 2 for u in range(9)], list(range(9))):
        _, reps, _ = check_seam(pcms, req, stem_of)
        assert reps[0].depth == 9
    assert check_seam([], [], []) == ([], [], [])


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_a_fitted_stem_above_the_ceiling_is_not_clamped(dtype):
    """Two talkers in antiphase under +6 dB: the mixture is quiet but for one sample, so s_p stays large; each scaled
    stem peaks above the ceiling: unclamped in f64, clamped by the 16-bit sink alone"""
    t = TILE[np.dtype(dtype)]
    a = pcm_of(t + 77, 1, np.float64)
    b = -0.9 * a
    a[100] = b[100] = 6000.0
    pcms = [x if dtype == np.float64 else np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) for x in (a, b)]
    db = -6.0
    got, reps, sreps = check_seam(pcms, [(0, 0, 6.0), (0, 0, 6.0)], [0, 1], True, db)
    c = ceiling(db)
    assert reps[0].scale < 1.0 and np.abs(got[0].astype(np.float64)).max() <= c
    assert sreps[0].peak * reps[0].scale > 32767.0
    if dtype == np.float64:
        assert np.abs(got[1]).max() == sreps[0].peak * reps[0].scale  # as it is, above the ceiling and above full scale
    else:
        assert got[1].max() == 32767 and got[1].min() == -32768


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_levels_at_the_host_tests_lengths(dtype):
    for n in (1, 255, 256, 1023, 1024, 1025, 3 * 1024 + 1):
        for a in sorted({0, 1023, 1024, 1025, 2047, 2048, 2049} & set(range(n))):
            pcms = [pcm_of(n, 5, dtype), pcm_of(n - a, 6, dtype)]
            check_seam(pcms, [(0, 0, 0.0), (0, a, -1.0)], [0, 1])


# ---- 2. the request in a batch --------------------------------------------------------------------------------------
# two talkers of two sentences each in one programme, and an utterance of its own
SENTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
# (programme, start, gain_db, pad_after, fade_in, fade_out)
MIX5 = [(0, 0, 0.0, 0, 240, 240), (0, 20001, -4.0, 7, 100, 100), (0, 70000, 1.0, 0, 240, 240),
        (0, 90003, -2.0, 11, 0, 480), (None, 5, 0.0, 3, 1, 1)]
STEM5 = [0, 1, 0, 1, None]


@pytest.fixture(scope="module")
def utts5(eng):
    return eng.voice_info(), [eng.states(s) for s in SENTS]


def member_pcm(b, i16):
    return [b.pcm_i16(u) if i16 else b.pcm(u) for u in range(len(b))]


def check_batch_stems(b, i16, req, stem_of, fit=False, ceiling_db=0.0, levels=True):
    """The batch's units are the seam's on the batch's own final PCM (with fit: the host rule under the device's
    scale), the probes agree with the geometry, and the reports with the seam's"""
    pcms = member_pcm(b, i16)
    geo = J.mix_stems_geometry(req, stem_of, [x.size for x in pcms])
    P, U = geo["P"], geo["U"]
    assert b.num_programmes() == P and b.num_outputs() == U
    assert [b.stem_unit(u) for u in range(len(b))] == geo["stem_unit"]
    reps = [b.mix_report(p) for p in range(P)]
    opts = _ffi.mix_opts(fit, ceiling_db)
    want, _, wsreps = J.mix_stems_host(pcms, req, stem_of, opts, [r.scale for r in reps] if fit else None,
                                       levels=levels)  # (without the flag: no sums, NaN for the dB values)
    got = [b.programme_pcm(u) for u in range(U)]
    for u in range(U):
        assert same(got[u], want[u]), u
        assert b.programme_layout(u)[1] == want[u].size
    for u in range(P, U):
        assert b.stem_layout(u) == (geo["programme"][u], geo["stem_id"][u], geo["members"][u], geo["first"][u],
                                    geo["end"][u])
        r, w = b.stem_report(u), wsreps[u - P]
        assert (r.peak, r.scale) == (w.peak, reps[geo["programme"][u]].scale), u
        assert sums_of(r) == sums_of(w), u
        assert np.array_equal((r.level_db, r.sir_db, r.si_sdr_db), (w.level_db, w.sir_db, w.si_sdr_db), equal_nan=True)
    with pytest.raises(J.JbError, match="no such programme"):
        b.mix_report(P)
    with pytest.raises(J.JbError, match="no such stem"):
        b.stem_report(0)
    return got


@pytest.mark.parametrize("i16", [False, True])
def test_batch_stems_are_the_seam_on_the_batch_pcm(eng, utts5, i16):
    vi, utts = utts5
    with J.Batch(vi, utts, pcm_i16=i16) as b:
        b.set_output_rate(44100)  # behind the converter: odd lengths
        b.set_loudness_target(-20.0, -1.0)
        b.set_mix(MIX5, fit=True, ceiling_db=-9.0)
        b.set_mix_stems(STEM5, levels=True)
        assert b.num_outputs() == 4 and b.num_programmes() == 2 and b.stem_unit(2) == 2 and b.stem_unit(4) == -1
        assert b.stem_layout(3)[:3] == (0, 1, 2)
        with pytest.raises(J.JbError, match="has not run"):
            b.stem_report(2)
        b.run()
        check_batch_stems(b, i16, MIX5, STEM5, True, -9.0)
        assert b.mix_report(0).scale < 1.0 and -30 < b.stem_report(2).si_sdr_db < 30


def md5_of(pcm):
    return hashlib.md5(np.ascontiguousarray(pcm, dtype="<i2").tobytes()).digest()


def test_encoders_take_stems_and_the_programmes_stay_byte_for_byte(eng, utts5):
    vi, utts = utts5
    hz = vi.sampling_frequency
    fo, mo = J.fbank(center=True), J.mfcc(delta_order=2, cmvn="mean_var")
    ml = J.melspec(n_fft=1200, hop=480, log="log10", range=8.0, f64=True)
    res = []
    for stems in (False, True):
        with J.Batch(vi, utts) as b:
            b.set_mix(MIX5)
            if stems:
                b.set_mix_stems(STEM5)
            b.set_format("s16", dither=True, seed=77)
            b.set_adpcm()
            b.set_fbank(fo)
            b.set_mfcc(mo, fbank=fo)
            b.set_melspec(ml)
            b.set_activity(J.activity())
            b.run()
            units = check_batch_stems(b, False, MIX5, STEM5, levels=False) if stems else [b.programme_pcm(p) for p in range(2)]
            for p, x in enumerate(units):
                assert b.formatted(p) == J.format_pcm_host(x, "s16", True, 77), p
                assert b.read_adpcm(p) == J.adpcm_encode_host(x, hz), p
                assert np.array_equal(b.read_fbank(p), J.fbank_pcm(x, hz, fo)), p
                assert np.array_equal(b.read_mfcc(p), J.mfcc_pcm(x, hz, fo, mo)), p  # the CMVN runs over the stem
                assert np.array_equal(b.read_melspec(p), J.melspec_pcm(x, hz, ml)), p  # ... and so does the clamp
            rep = [(r.peak, r.scale, r.depth, r.overlap) for r in (b.mix_report(p) for p in range(2))]
            res.append(([(x.tobytes(), b.formatted(p), b.read_adpcm(p), b.read_fbank(p).tobytes(),
                          b.read_mfcc(p).tobytes(), b.read_melspec(p).tobytes()) for p, x in enumerate(units[:2])],
                        rep, [a.tobytes() for a in b.read_activity_all()], [x.tobytes() for x in member_pcm(b, False)]))
            if stems:  # the activity stage keeps the P programmes as its units
                assert len(b.read_activity_all()) == 2
                with pytest.raises(J.JbError):
                    b.read_activity(2)
    assert res[0] == res[1]


def test_flac_streams_of_stems(eng, utts5):
    vi, utts = utts5
    res = []
    for stems in (False, True):
        with J.Batch(vi, utts, pcm_i16=True) as b:
            b.set_mix(MIX5)
            if stems:
                b.set_mix_stems(STEM5, levels=True)
            b.set_flac(block_size=1152, md5=True, seek_interval_ms=20)
            b.run()
            units = check_batch_stems(b, True, MIX5, STEM5) if stems else [b.programme_pcm(p) for p in range(2)]
            streams = b.flac_all()
            assert len(streams) == len(units)
            for p, x in enumerate(units):
                dec, _, meta = flac_check(streams[p])  # decodes, and every seek point verifies
                assert np.array_equal(dec, x) and meta["total"] == x.size and meta["md5"] == md5_of(x), p
            res.append(streams[:2])
    assert res[0] == res[1]


def test_refusals_leave_the_request_as_it_was(eng, utts5):
    vi, utts = utts5
    join5 = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (None, 0, 0)]
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="holds no mix request"):
            b.set_mix_stems(STEM5)
        b.set_join(join5)
        with pytest.raises(J.JbError, match="holds a join request"):
            b.set_mix_stems(STEM5)
        assert b.num_outputs() == 2
        b.set_join(None)
        b.set_mix(MIX5)
        b.set_mix_stems(STEM5)
        assert b.num_outputs() == 4
        with pytest.raises(J.JbError, match="utterance 3.*stem id"):
            b.set_mix_stems([0, 1, 0, 5, None])
        with pytest.raises(J.JbError, match="one stem id per utterance"):
            b.set_mix_stems(STEM5[:4])
        assert J.lib().jb_batch_set_mix_stems(b._h, _ffi.stem_ids(STEM5), 5, 2) == -1
        assert b"unknown flag" in J.lib().jb_last_error()
        assert b.num_outputs() == 4 and b.stem_unit(1) == 3  # every refusal left the request standing
        b.set_mix_stems(None)  # withdrawn alone: the mix stands
        assert b.num_outputs() == 2 and b.num_programmes() == 2 and b.stem_unit(1) == -1
        b.set_mix_stems([2, 1, 0, 1, 4])  # three stems in the programme, one of the utterance alone
        assert b.num_outputs() == 6
        b.set_mix(None)  # withdrawing the mix withdraws the stems
        assert b.num_outputs() == 5 == len(b) and b.num_programmes() == 5 and b.stem_unit(0) == -1
        b.set_mix(MIX5)
        assert b.num_outputs() == 2
        with pytest.raises(J.JbError, match="no such stem"):
            b.stem_layout(1)
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_mix_stems(STEM5)
        with pytest.raises(J.JbError, match="was not called"):
            b.stem_report(2)


# ---- 3. redo rounds -------------------------------------------------------------------------------------------------
REDO_MIX = [(0, 100, 0.0, 0, 48, 48), (1, 3, -2.0, 5, 48, 48), (0, 2400, 3.0, 7, 48, 48), (1, 1000, 0.0, 0, 48, 48)]


@pytest.mark.parametrize("i16", [False, True])
def test_redo_rounds_leave_no_stale_stem_or_level(eng, tab, i16):
    """tests/test_gpu_mix.py's recipe (test_redo_rounds_leave_no_stale_mixture): every hand-off of the long members
    fails, so redo rounds rewrite them behind the first mix; the loudness group {1, 2} spans both programmes.  A
    touched programme runs again whole, with its stems and their levels"""
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (400, 90, 600, 30)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        b.set_loudness_target(-21.0, math.inf)
        b.set_loudness_groups([None, 0, 0, None])
        b.set_mix(REDO_MIX, fit=True, ceiling_db=-12.0)
        b.set_mix_stems([0, 0, 1, 1], levels=True)
        b.set_adpcm()
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 1 and sum(b.redo_stats()) >= 1
        units = check_batch_stems(b, i16, REDO_MIX, [0, 0, 1, 1], True, -12.0)  # from the final per-utterance PCM
        assert len(units) == 6 and any(b.mix_report(p).scale < 1.0 for p in range(2))
        for p, x in enumerate(units):
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, vi.sampling_frequency), p


# ---- 4. invariance --------------------------------------------------------------------------------------------------
def test_stems_alone_and_among_others(eng, tab):
    vi = eng.voice_info()
    probe = [synth.synth_utterance(tab, T, 77 + T) for T in (300, 40, 210)]
    others = [synth.synth_utterance(tab, 50 + 7 * k, 1000 + k) for k in range(24)]
    req = [(0, 1000, 0.0, 3, 100, 100), (0, 30000, -6.5, 2401, 100, 100), (0, 5, 3.0, 7, 100, 100)]
    one = (None, 1, 0.0, 1)
    res = []
    for utts, r, st, p in ((probe, req, [0, 1, 0], 0),
                           (others[:10] + probe[:1] + others[10:20] + probe[1:] + others[20:],
                            [one] * 10 + req[:1] + [one] * 10 + req[1:] + [one] * 4,
                            [None] * 10 + [20] + [3] * 10 + [1, 20] + [None] * 4, 10)):
        with J.Batch(vi, utts, fast_invariant=True, pcm_i16=True) as b:
            b.set_mix(r, fit=True, ceiling_db=-9.0)
            b.set_mix_stems(st, levels=True)
            b.run()
            us = sorted({b.stem_unit(u) for u in range(len(utts)) if b.programme_of(u) == p})
            assert len(us) == 2
            reps = [b.stem_report(u) for u in us]
            res.append([(b.programme_pcm(u).tobytes(), b.stem_layout(u)[2:], r_.peak, r_.scale, sums_of(r_))
                        for u, r_ in zip(us, reps)])
    assert res[0] == res[1]


# ---- 5. without the request -----------------------------------------------------------------------------------------
def test_without_the_request_the_batch_is_the_mix_of_today(eng, utts5):
    """Held to the seam and the host rule that already exist (jb_mix_pcm_batch, jb_mix_host), not to stored hashes"""
    vi, utts = utts5
    with J.Batch(vi, utts) as b:
        b.set_mix(MIX5, fit=True, ceiling_db=-9.0)
        b.set_adpcm()
        b.run()
        assert b.num_outputs() == b.num_programmes() == 2 and len(b.read_adpcm_all()) == 2
        pcms = member_pcm(b, False)
        opts = _ffi.mix_opts(True, -9.0)
        seam, sreps = J.mix_pcm(pcms, MIX5, opts)
        host, _ = J.mix_host(pcms, MIX5, opts, [r.scale for r in sreps])
        for p in range(2):
            r = b.mix_report(p)
            assert same(b.programme_pcm(p), seam[p]) and same(seam[p], host[p])
            assert (r.peak, r.scale, r.depth, r.overlap) == (sreps[p].peak, sreps[p].scale, sreps[p].depth,
                                                             sreps[p].overlap)
            assert b.read_adpcm(p) == J.adpcm_encode_host(seam[p], vi.sampling_frequency)
        assert [b.stem_unit(u) for u in range(5)] == [-1] * 5
        with pytest.raises(J.JbError, match="was not called"):
            b.stem_report(2)
    with J.Batch(vi, utts) as b:  # no request at all: the utterances
        assert b.num_outputs() == b.num_programmes() == 5


# ---- 6. the engine entries and the example --------------------------------------------------------------------------
ENG_SENTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
ENG_PLACE = [(0.0, 0.0), (350.0, -6.5), (120.25, 3.0)]
ENG_OPTS = dict(lead_ms=12.5, trail_ms=3.3, fade_ms=5.0)
ENG_STEMS = [1, 0, 1]


def test_engine_programme_stems(eng):
    from tests import join_ref as R

    e = eng.clone()
    hz = e._out_hz()
    # without a mix the entries refuse before any device is touched, and other sinks are not theirs
    with pytest.raises(J.JbError, match="holds no mix"):
        e.synthesize_programme(ENG_SENTS, stems=ENG_STEMS, **ENG_OPTS)
    with pytest.raises(ValueError):
        e.synthesize_programme(ENG_SENTS, sink="i16", stems=ENG_STEMS, **ENG_OPTS)
    with pytest.raises(ValueError):
        e.synthesize_programme(ENG_SENTS, sink="adpcm", stems=ENG_STEMS, **ENG_OPTS)
    e.set_programme_mix(ENG_PLACE, fit=True, ceiling_db=-9.0)
    with pytest.raises(J.JbError, match="utterance 2.*stem id"):
        e.synthesize_programme(ENG_SENTS, stems=[0, 1, 3], **ENG_OPTS)
    parts, parts16 = e.synthesize_batch(ENG_SENTS), e.synthesize_batch(ENG_SENTS, i16=True)
    f = R.ms_to_samples(ENG_OPTS["fade_ms"], hz)
    req = [(0, R.ms_to_samples(ENG_OPTS["lead_ms"] + ms, hz), db, R.ms_to_samples(ENG_OPTS["trail_ms"], hz), f, f)
           for ms, db in ENG_PLACE]
    opts = _ffi.mix_opts(True, -9.0)
    # f64: the mixture first (the plain entry's), the S stems behind it, the reports the seam's under the same scale
    mix, starts = e.synthesize_programme(ENG_SENTS, **ENG_OPTS)
    got, gstarts, reps = e.synthesize_programme(ENG_SENTS, stems=ENG_STEMS, levels=True, **ENG_OPTS)
    assert len(got) == 1 + 2 == 1 + len(reps) and gstarts == starts == [r[1] for r in req] and same(got[0], mix)
    assert reps[0].scale < 1.0
    want, _, wreps = J.mix_stems_host(parts, req, ENG_STEMS, opts, [reps[0].scale], levels=True)
    for u in range(3):
        assert same(got[u], want[u]), u
    for r, w in zip(reps, wreps):
        assert (r.peak, r.scale) == (w.peak, w.scale) and sums_of(r) == sums_of(w)
        assert (r.level_db, r.sir_db, r.si_sdr_db) == (w.level_db, w.sir_db, w.si_sdr_db)
    # FLAC with its metadata: every stream verifies and decodes to the 16-bit unit
    streams, fstarts, freps = e.synthesize_programme(ENG_SENTS, sink="flac", md5=True, seek_interval_ms=100,
                                                     stems=ENG_STEMS, levels=True, **ENG_OPTS)
    plain, _ = e.synthesize_programme(ENG_SENTS, sink="flac", md5=True, seek_interval_ms=100, **ENG_OPTS)
    assert len(streams) == 3 and fstarts == starts and streams[0] == plain
    want16, _, wreps16 = J.mix_stems_host(parts16, req, ENG_STEMS, opts, [freps[0].scale], levels=True)
    for u, s in enumerate(streams):
        dec, _, meta = flac_check(s)
        assert np.array_equal(dec, want16[u]) and meta["md5"] == md5_of(want16[u]) and meta["rate"] == hz, u
    assert [sums_of(r) for r in freps] == [sums_of(w) for w in wreps16]
    # without levels: the reports carry the peak and the scale alone
    _, _, nreps = e.synthesize_programme(ENG_SENTS, stems=ENG_STEMS, **ENG_OPTS)
    assert all(sums_of(r) == (0.0, 0.0, 0.0) and math.isnan(r.si_sdr_db) for r in nreps)
    assert [r.peak for r in nreps] == [r.peak for r in reps]
    # the convenience form sets the mix for the call alone
    e.set_programme_mix(None)
    again, _, _ = e.synthesize_programme(ENG_SENTS, mix=ENG_PLACE, fit=True, ceiling_db=-9.0, stems=ENG_STEMS,
                                         **ENG_OPTS)
    assert all(same(a, g) for a, g in zip(again, got)) and e.get_programme_mix()[0] is None


def test_mixture_example_stems(tmp_path):
    import csv
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    out, stems, levels = tmp_path / "mixture.flac", tmp_path / "stems", tmp_path / "levels.csv"
    labs = []
    for k, s in enumerate(ENG_SENTS):
        p = tmp_path / f"s{k}.lab"
        p.write_text("\n".join(s) + "\n")
        labs.append(str(p))
    r = subprocess.run([sys.executable, str(root / "examples" / "mixture.py"), str(VOICE), *labs, "-o", str(out),
                        "--start-ms", "0,400,150", "--gain-db", "0,-6,-3", "--fit", "--stems", str(stems),
                        "--talker", "7", "2", "7", "--levels", str(levels)], capture_output=True, text=True,
                       timeout=300, cwd=str(root))
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in stems.iterdir()) == ["mix.flac", "s2.flac", "s7.flac"]
    assert (stems / "mix.flac").read_bytes() == out.read_bytes()
    units = {}
    for name in ("mix", "s7", "s2"):
        dec, _, meta = flac_check((stems / f"{name}.flac").read_bytes())  # verifies: MD5 and every seek point
        assert dec.size == meta["total"] > 0 and meta["md5"] == md5_of(dec)
        units[name] = dec
    assert units["s7"].size == units["s2"].size == units["mix"].size
    with open(levels) as f:
        rows = list(csv.DictReader(f))
    assert [row["stem"] for row in rows] == ["s7", "s2"]  # by the first sentence of each id
    for row in rows:  # the sums are taken from the units as stored: the host rule over the decoded streams gives them
        x = units[row["stem"]]
        nz = np.flatnonzero(x)
        e_s, d, e_p = J.mix_levels_host(x, units["mix"])
        assert float(row["e_p"]) == e_p and float(row["e_s"]) == e_s and float(row["d"]) == d, row["stem"]
        assert (float(row["level_db"]), float(row["sir_db"]), float(row["si_sdr_db"])) == J.mix_levels_db(e_s, d, e_p)
        assert nz.size and float(row["peak"]) > 0.0 and 0.0 < float(row["scale"]) <= 1.0
