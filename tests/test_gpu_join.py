"""The join stage on the GPU (jb_join.hip): the device seam against the host seam bit for bit (the host seam is held to
the numpy statement of the rules by tests/test_join_abi.py) over every misalignment of source against destination, pads,
fades and tile boundaries; then the stage in a batch -- from f64 and from the 16-bit sink, behind the converter and the
loudness apply pass -- with FLAC, the sample format and IMA ADPCM encoding programmes; redo rounds; the fast invariant
mode; the engine entries; and the batch without a request.  Every comparison is bit-exact."""
import hashlib
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import join_ref as R
from tests.conftest import VOICE
from tests.flac_meta_ref import check as flac_check
from tests.flac_meta_ref import split as flac_split
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE = {np.dtype(np.float64): 2048, np.dtype(np.int16): 8192}  # samples of a workgroup's tile (16 KiB)


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


def check_seam(pcms, req):
    want = J.join_host(pcms, req)
    got = J.join_pcm(pcms, req)
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (p, g.size, w.size, np.flatnonzero(g[:min(g.size, w.size)] != w[:min(g.size, w.size)])[:8])
    return got


LENGTHS, PADS = R.LENGTHS, R.PADS


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_lengths_pads_fades_and_every_misalignment(dtype):
    """Members of every listed length in one programme, twice over (so that each length meets several pads), under
    every listed fade.  The seam packs its inputs one after the other, so member u's source offset is the sum of the
    lengths in front of it: with the odd lengths and pads the 16-bit path meets all 8 offsets of source against
    destination within 16 bytes, the f64 path both 8-byte phases (asserted from the geometry)."""
    lengths = LENGTHS + LENGTHS[::-1]
    pcms = [pcm_of(n, 31 * u + n, dtype) for u, n in enumerate(lengths)]

    def fades(n):
        return [0, 1, 2, n, n + 5]
    req = [(0, PADS[u % 4], PADS[(u // 4) % 4], fades(n)[u % 5], fades(n)[(u + 2) % 5]) for u, n in enumerate(lengths)]
    check_seam(pcms, req)
    _, start, _ = J.join_geometry(req, lengths)
    per = 16 // np.dtype(dtype).itemsize
    src = np.cumsum([0] + lengths[:-1])
    phases = {int((s - d) % per) for s, d, n in zip(src, start, lengths) if n >= 2 * per}
    assert phases == set(range(per))
    # the same members each a programme of its own, and with every fade against every length
    check_seam(pcms, [(None,) + r[1:] for r in req])
    for fi in range(5):
        check_seam(pcms[:10], [(0, 1, 0, fades(n)[fi], fades(n)[(fi + 3) % 5]) for n in LENGTHS])


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_every_source_offset_against_every_destination_offset(dtype):
    """A first member of k samples shifts the source of the second by k; a pad of d shifts its destination."""
    per = 16 // np.dtype(dtype).itemsize
    pcms, req = [], []
    for k in range(per):
        for d in range(per):
            pcms += [pcm_of(k, k, dtype), pcm_of(3 * per + 5, 100 + 8 * k + d, dtype)]
            req += [(len(req) // 2, 0, 0), (len(req) // 2, d, 2, 3, 4)]
    check_seam(pcms, req)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_member_boundaries_inside_a_tile_and_on_its_edge(dtype):
    t = TILE[np.dtype(dtype)]
    # a boundary exactly on the tile edge, one sample to either side of it, and a pad across it
    for first, pad in ((t, 0), (t - 1, 0), (t + 1, 0), (t - 3, 3), (t - 3, 7), (2 * t, 0)):
        pcms = [pcm_of(first, 5, dtype), pcm_of(t // 2 + 3, 6, dtype), pcm_of(9, 7, dtype)]
        check_seam(pcms, [(0, 0, pad, 5, 5), (0, 0, 0, 9, 9), (0, 0, 0)])
    # fades longer than a tile
    check_seam([pcm_of(3 * t + 1, 8, dtype)], [(None, 1, 1, 2 * t + 3, t + 9)])


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_seam_programme_shapes(dtype):
    one = [pcm_of(777, 1, dtype)]
    (got,) = check_seam(one, [(None,)])
    assert same(got, one[0])  # no pads, no fades: the member, bit for bit
    pcms = [pcm_of(50 + 13 * u, u, dtype) for u in range(64)]
    assert len(check_seam(pcms, [(7, u % 3, u % 5, 4, 4) for u in range(64)])) == 1  # one programme of all
    assert len(check_seam(pcms, [(None, u % 3, u % 5, 4, 4) for u in range(64)])) == 64  # 64 programmes of one
    assert check_seam([], []) == []
    # a programme of empty members and pads alone
    (z,) = check_seam([np.zeros(0, dtype)] * 3, [(0, 2, 3, 4, 4)] * 3)
    assert z.size == 15 and not z.any()


def test_seam_keeps_the_bits_of_a_copied_f64_sample():
    x = np.arange(64, dtype=np.float64)
    x[5] = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]
    x[6], x[7], x[8] = -0.0, 5e-324, -np.inf
    (got,) = check_seam([x], [(None, 3, 0, 2, 2)])
    assert got[3 + 2:3 + 62].tobytes() == x[2:62].tobytes()


# ---- 2. the batch path ----------------------------------------------------------------------------------------------
FRAMES6 = (7, 1, 40, 3, 12, 5)
REQ6 = [(0, 4097, 3, 240, 240), (1, 1, 0, 0, 7), (0, 0, 5, 0, 0), (1, 7, 9, 3, 0), (0, 0, 11, 5, 99999), (None, 2, 4, 1, 1)]


@pytest.fixture(scope="module")
def utts6(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 3 + t) for t in FRAMES6]


def member_pcm(b, i16):
    return [b.pcm_i16(u) if i16 else b.pcm(u) for u in range(len(b))]


def check_programmes(b, i16, req):
    """programme_pcm(p) is join_ref of the PCM the same batch hands out; the layout entries agree."""
    pcms = member_pcm(b, i16)
    want, prog_of, start = R.join(pcms, req)
    assert b.num_outputs() == len(want)
    assert [b.programme_of(u) for u in range(len(b))] == prog_of
    assert [b.member_start(u) for u in range(len(b))] == start
    got = []
    for p, w in enumerate(want):
        members = [u for u in range(len(b)) if prog_of[u] == p]
        assert b.programme_layout(p) == (len(members), w.size, b.output_rate(members[0]))
        got.append(b.programme_pcm(p))
        assert same(got[p], w.astype(np.int16 if i16 else np.float64)), p
    return got


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("chain", ["native", "rate", "loudness", "both"])
def test_batch_programmes_are_the_join_of_the_batch_pcm(eng, utts6, i16, chain):
    vi, utts = utts6
    with J.Batch(vi, utts, pcm_i16=i16) as b:
        if chain in ("rate", "both"):
            b.set_output_rate(44100)  # 48 kHz -> 44.1 kHz: odd lengths
        if chain in ("loudness", "both"):
            b.set_loudness_target(-20.0, -1.0)
        b.set_join(REQ6)
        # the geometry answers before the run
        assert b.num_outputs() == 3 and b.programme_of(4) == 0 and b.member_start(0) == 4097
        with pytest.raises(J.JbError, match="has not run"):
            b.programme_pcm(0)
        b.run()
        if chain in ("rate", "both"):
            assert any(b.num_samples(u) % 2 for u in range(6))
        check_programmes(b, i16, REQ6)


@pytest.mark.parametrize("i16", [False, True])
def test_no_pads_no_fades_all_none_is_the_final_slab(eng, utts6, i16):
    vi, utts = utts6
    with J.Batch(vi, utts, pcm_i16=i16) as b:
        b.set_join([(None,)] * 6)
        b.run()
        got = check_programmes(b, i16, [(None,)] * 6)
        for u, x in enumerate(member_pcm(b, i16)):
            assert same(got[u], x)


# ---- 3. the encoders take programmes --------------------------------------------------------------------------------
def md5_of(pcm):
    return hashlib.md5(np.ascontiguousarray(pcm, dtype="<i2").tobytes()).digest()


def check_flac(b, progs, hz, decode=True, **opts):
    streams = J.flac_encode(progs, hz, **opts)
    every = b.flac_all()
    assert len(every) == len(progs)
    for p, x in enumerate(progs):
        s = b.flac(p)
        assert s == every[p] == streams[p], p  # byte for byte the seam's stream of those samples
        if not decode:  # (a long programme: the seam's streams are decoded by tests/test_gpu_flac_meta.py)
            assert flac_split(s)[0]["md5"] == md5_of(x) and flac_split(s)[0]["total"] == x.size
            continue
        dec, _, meta = flac_check(s)  # decodes, and every seek point verifies
        assert np.array_equal(dec, x) and meta["total"] == x.size and meta["rate"] == hz
        if opts.get("md5"):
            assert meta["md5"] == md5_of(x)
        if opts.get("seek_interval_ms"):
            assert meta["points"] is not None or x.size == 0


def test_flac_streams_of_programmes(eng, utts6):
    vi, utts = utts6
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_join(REQ6)
        b.set_flac(block_size=1152, md5=True, seek_interval_ms=20)
        b.run()
        progs = check_programmes(b, True, REQ6)
        check_flac(b, progs, vi.sampling_frequency, block_size=1152, md5=True, seek_interval_ms=20)
        assert b.num_outputs() == 3
        L = J.lib()
        n = J._ffi.C.c_size_t()
        assert L.jb_batch_flac_size(b._h, 3, J._ffi.C.byref(n)) == -1  # index 3 is refused
        assert L.jb_batch_read_flac(b._h, 3, None, 0) == -1
        # the per-utterance PCM entries keep handing out utterances
        assert len(b.pcm_all()) == 6


def test_formatted_and_adpcm_of_programmes(eng, utts6):
    vi, utts = utts6
    hz = vi.sampling_frequency
    with J.Batch(vi, utts) as b:
        b.set_join(REQ6)
        b.set_format("s16", dither=True, seed=77)  # TPDF: the dither index runs over the programme
        b.set_adpcm()
        b.run()
        progs = check_programmes(b, False, REQ6)
        assert b.formatted_all() == [b.formatted(p) for p in range(3)]
        assert b.read_adpcm_all() == [b.read_adpcm(p) for p in range(3)]
        for p, x in enumerate(progs):
            assert b.formatted(p) == J.format_pcm_host(x, "s16", True, 77), p
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, hz), p
            assert b.adpcm_block_align(p) == J.adpcm_geometry(hz, 0)[0]
            assert b.adpcm_size(p) == J.adpcm_geometry(hz, x.size)[3]
        L, C = J.lib(), J._ffi.C
        n = C.c_size_t()
        assert L.jb_batch_formatted_size(b._h, 3, C.byref(n)) == -1 and L.jb_batch_adpcm_size(b._h, 3, C.byref(n)) == -1
        assert L.jb_batch_read_formatted(b._h, 3, None, 0) == -1 and L.jb_batch_read_adpcm(b._h, 3, None, 0) == -1
    # A by the programme's rate; 16-bit source
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_output_rate([8000, 22050, 8000, 22050, 8000, 0])
        b.set_join(REQ6)
        b.set_adpcm()
        assert [b.adpcm_block_align(p) for p in range(3)] == [256, 512, J.adpcm_geometry(hz, 0)[0]]
        b.run()
        progs = check_programmes(b, True, REQ6)
        for p, x in enumerate(progs):
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, b.programme_layout(p)[2]), p


# ---- 4. redo rounds -------------------------------------------------------------------------------------------------
REDO_REQ = [(0, 100, 0, 48, 48), (1, 3, 5, 48, 48), (0, 2400, 7, 48, 48), (1, 1, 0, 48, 48)]


@pytest.mark.parametrize("i16,grouped", [(False, False), (True, False), (False, True), (True, True)])
def test_redo_rounds_leave_no_stale_programme(eng, tab, i16, grouped):
    """Every hand-off of the long members fails, so redo rounds rewrite them behind the first join.  With the loudness
    group {1, 2} spanning both programmes, utterance 1 (one chunk: the vocoder never rewrites it) changes its gain with
    utterance 2's redo, and with it programme 1's bytes."""
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (400, 90, 600, 30)]
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        if grouped:
            b.set_loudness_target(-21.0, math.inf)
            b.set_loudness_groups([None, 0, 0, None])
        b.set_join(REDO_REQ)
        if i16:
            b.set_flac(md5=True, seek_interval_ms=50)
        else:
            b.set_format("s24", dither=True, seed=5)
        b.set_adpcm()
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 1 and sum(b.redo_stats()) >= 1
        progs = check_programmes(b, i16, REDO_REQ)  # recomputed from the final per-utterance PCM
        hz = vi.sampling_frequency
        for p, x in enumerate(progs):
            assert b.read_adpcm(p) == J.adpcm_encode_host(x, hz), p
            if not i16:
                assert b.formatted(p) == J.format_pcm_host(x, "s24", True, 5), p
        if i16:
            check_flac(b, progs, hz, decode=False, md5=True, seek_interval_ms=50)


# ---- 5. invariance --------------------------------------------------------------------------------------------------
def test_programme_alone_and_among_64(eng, tab):
    vi = eng.voice_info()
    probe = [synth.synth_utterance(tab, T, 77 + T) for T in (300, 40, 210)]
    others = [synth.synth_utterance(tab, 50 + 7 * k, 1000 + k) for k in range(64)]
    req = [(0, 1000, 3, 100, 100), (0, 0, 2401, 100, 100), (0, 5, 7, 100, 100)]
    res = []
    for utts, r, p in ((probe, req, 0),
                       (others[:20] + probe[:1] + others[20:50] + probe[1:] + others[50:],
                        [(None, 1, 1)] * 20 + req[:1] + [(None, 1, 1)] * 30 + req[1:] + [(None, 1, 1)] * 14, 20)):
        with J.Batch(vi, utts, fast_invariant=True, pcm_i16=True) as b:
            b.set_join(r)
            b.set_flac(md5=True)
            b.run()
            assert b.programme_layout(p)[0] == 3
            res.append((b.programme_pcm(p).tobytes(), b.flac(p)))
    assert res[0] == res[1]


# ---- 6. the engine entries ------------------------------------------------------------------------------------------
SENTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1]
OPTS = dict(lead_ms=12.5, gap_ms=500.0, trail_ms=3.3, fade_ms=5.0)


def test_engine_programme_i16_flac_and_scope(eng):
    for e in (eng, eng.clone()):
        if e is not eng:
            e.condition.set_output_sampling_frequency(22050)
            e.condition.set_loudness_target(-19.0)
            e.condition.set_loudness_scope(J.LOUDNESS_PER_REQUEST)
        hz = e._out_hz()
        parts = e.synthesize_batch(SENTS, i16=True)
        req = R.chapter([x.size for x in parts], hz, **OPTS)
        (want,), _, want_start = R.join(parts, req)
        got, starts = e.synthesize_programme(SENTS, sink="i16", **OPTS)
        assert same(got, want) and starts == want_start
        assert starts[0] == R.ms_to_samples(12.5, hz) and req[0][2] == R.ms_to_samples(500.0, hz)
        stream, fstarts = e.synthesize_programme(SENTS, sink="flac", md5=True, seek_interval_ms=100, **OPTS)
        dec, _, meta = flac_check(stream)
        assert np.array_equal(dec, want) and meta["md5"] == md5_of(want) and meta["rate"] == hz
        assert fstarts == want_start


def test_engine_programme_f64_formatted_and_adpcm(eng):
    hz = eng._out_hz()
    parts = eng.synthesize_batch(SENTS)
    (want,), _, want_start = R.join(parts, R.chapter([x.size for x in parts], hz, **OPTS))
    got, starts = eng.synthesize_programme(SENTS, **OPTS)
    assert same(got, want) and starts == want_start
    data, _ = eng.synthesize_programme(SENTS, sink="formatted", fmt="s24", dither=True, seed=3, **OPTS)
    assert data == J.format_pcm_host(want, "s24", True, 3)
    # the ADPCM entry goes through the 16-bit sink, as jb_synthesize_batch_adpcm does: the join of the 16-bit samples
    parts16 = eng.synthesize_batch(SENTS, i16=True)
    (want16,), _, _ = R.join(parts16, R.chapter([x.size for x in parts16], hz, **OPTS))
    s, astarts = eng.synthesize_programme(SENTS, sink="adpcm", **OPTS)
    assert (s.n_samples, s.hz) == (want16.size, hz) and s.data == J.adpcm_encode_host(want16, hz)
    assert astarts == want_start
    with pytest.raises(J.JbError, match="not negative"):
        eng.synthesize_programme(SENTS, gap_ms=-1.0)
    with pytest.raises(J.JbError, match="at least one utterance"):
        eng.synthesize_programme([])


def test_chapter_example(tmp_path):
    out = tmp_path / "chapter.flac"
    labs = []
    for k, s in enumerate(SENTS):
        p = tmp_path / f"s{k}.lab"
        p.write_text("\n".join(s) + "\n")
        labs.append(str(p))
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "chapter.py"), str(VOICE), *labs, "-o", str(out),
                        "--gap-ms", "300", "--fade-ms", "5"], capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    dec, _, meta = flac_check(out.read_bytes())
    assert dec.size == meta["total"] > 0 and meta["md5"] == md5_of(dec) and meta["points"]
    cues = [ln for ln in r.stdout.splitlines() if ln.startswith("cue ")]
    assert len(cues) == 3 and cues[0].split()[2] == "0"


# ---- 7. without the request -----------------------------------------------------------------------------------------
def test_default_unchanged_and_rules(eng, utts6):
    vi, utts = utts6
    with J.Batch(vi, utts) as b:
        b.run()
        plain, info, kinfo = [x.tobytes() for x in member_pcm(b, False)], b.info(), b.kernel_info()
        assert b.num_outputs() == 6 and b.programme_of(0) == -1
        with pytest.raises(J.JbError, match="was not called"):
            b.programme_pcm(0)
        with pytest.raises(J.JbError, match="was not called"):
            b.member_start(0)
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_join(REQ6)
    with J.Batch(vi, utts) as b:  # a request made and withdrawn: the batch of today, the encoders by utterance
        b.set_join(REQ6)
        b.set_join(None)
        b.set_adpcm()
        b.set_format("s16")
        b.run()
        assert b.num_outputs() == 6 and len(b.read_adpcm_all()) == 6 and len(b.formatted_all()) == 6
        assert [x.tobytes() for x in member_pcm(b, False)] == plain and b.info() == info and b.kernel_info() == kinfo
        for u in range(6):
            assert b.read_adpcm(u) == J.adpcm_encode_host(b.pcm(u), vi.sampling_frequency)
    with J.Batch(vi, utts) as b:  # with the request the members' PCM and the vocoder's work items stay as they were
        b.set_join(REQ6)
        b.run()
        assert [x.tobytes() for x in member_pcm(b, False)] == plain and b.info() == info and b.kernel_info() == kinfo
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError, match="no PCM"):
            b.set_join(REQ6)
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one request per utterance"):
            b.set_join(REQ6[:5])
        with pytest.raises(J.JbError, match="programme id 6"):
            b.set_join([(6,)] + REQ6[1:])
        bad = J._ffi.join_request(REQ6)
        bad[2].reserved = 9
        assert J.lib().jb_batch_set_join(b._h, bad, 6) == -1 and b"reserved" in J.lib().jb_last_error()
        # a programme of mixed rates is refused by whichever setter comes second, and changes nothing
        b.set_output_rate([8000, 0, 16000, 0, 8000, 0])
        with pytest.raises(J.JbError, match="programme 0 would disagree on the output rate"):
            b.set_join(REQ6)
        assert b.num_outputs() == 6
        b.set_output_rate([8000, 0, 8000, 0, 8000, 0])
        b.set_join(REQ6)
        with pytest.raises(J.JbError, match="programme 1 would disagree on the output rate"):
            b.set_output_rate([8000, 0, 8000, 16000, 8000, 0])
        assert [b.output_rate(u) for u in range(6)] == [8000, vi.sampling_frequency] * 3
        assert b.programme_layout(0)[2] == 8000 and b.num_outputs() == 3
