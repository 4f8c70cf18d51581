"""The speech-activity stage on the GPU (jb_activity.hip): the device seam against the host rule byte for byte, reports
included (the host rule is held to the numpy statement by tests/test_activity_abi.py) -- every case of the host tests,
frame counts around the label kernel's word (64 frames) and word block (4096 frames), gaps, short runs and hangs laid
across those edges, f64 and 16-bit sources, a column of zeros, the absolute gate; then programmes through the seam; then
the stage in a batch through synthesis -- a mix, a join and no programme, f64 and 16-bit, the other outputs bit for bit
those of the batch without the request -- through redo rounds, under the fast invariant mode, and the engine entry."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi, synth
from tests import activity_ref as R
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

HZ = 16000
NINF = -math.inf
WORD = 64                 # frames of a packed word (a ballot of one wave)
BLOCK = 64 * WORD         # frames of k_act_label's word block (kActBlockFrames): the scan's carry crosses here
SMOOTH = dict(min_speech=3, min_gap=2, hang_before=1, hang_after=2)
REPORT = ("active", "first", "last", "peak", "thr")


@pytest.fixture(scope="module", autouse=True)
def device():
    assert J.lib().jb_device_count() > 0


def opts_of(grid, wl, hop, **kw):
    return J.activity(wl, hop, grid=grid, samples=True, **kw)


def check_units(pcms, opts, hz=HZ):
    """Every utterance a unit of its own: the device's labels and reports are jb_activity_host's"""
    labs, cols, units = J.activity_pcm(pcms, hz, opts)
    assert len(labs) == len(pcms)
    for u, x in enumerate(pcms):
        want, rep = J.activity_host(np.asarray(x, dtype=np.float64), hz, opts)
        got = labs[u]
        assert got.shape == (want.size, 1), (u, got.shape, want.size)
        assert got[:, 0].tobytes() == want.tobytes(), (u, len(x), np.flatnonzero(got[:, 0] != want)[:8])
        R.same_report(cols[u][0], {k: getattr(rep, k) for k in REPORT})
        R.same_report(units[u], R.unit_report_of(got))
    return labs


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_seam_is_the_host_rule_on_the_host_tests_cases(grid, i16):
    for wl in R.WINDOWS:
        for hop in R.hops_of(wl):
            pcms = [R.speechy(n, 7 * wl + hop + k, i16) for k, n in enumerate(R.lengths_of(wl, hop))]
            pcms.append(np.zeros(wl + hop, dtype=pcms[0].dtype))  # a column of zeros
            check_units(pcms, opts_of(grid, wl, hop))
            check_units(pcms, opts_of(grid, wl, hop, gate_db=20.0, **SMOOTH))


def pcm_of_bits(bits, wl=8):
    return R.pattern_pcm(bits, wl)


def edge_patterns(T):
    """Raw bits of T frames with gaps, short runs and lone frames laid across every word edge and the block edge"""
    rng = np.random.default_rng(T)
    out = []
    b = np.zeros(T, dtype=np.uint8)
    for e in [e for e in (WORD, 2 * WORD, BLOCK - WORD, BLOCK, BLOCK + WORD) if e < T]:
        b[max(0, e - 5):e - 2] = 1   # a run of three in front of the edge, a gap of three across it,
        b[min(T, e + 1):min(T, e + 3)] = 1  # a run of two behind it
    b[0] = b[T - 1] = 1
    out.append(b)
    out.append((rng.random(T) < 0.5).astype(np.uint8))
    sparse = (rng.random(T) < 0.01).astype(np.uint8)
    sparse[T // 2] = 1
    out.append(sparse)   # gaps of hundreds of frames: the carried frames come from far words
    out.append(1 - sparse if sparse.sum() < T else sparse)
    lone = np.zeros(T, dtype=np.uint8)
    lone[min(T - 1, WORD - 1)] = 1
    out.append(lone)
    return out


@pytest.mark.parametrize("T", [63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 70])
def test_smoothing_across_word_and_block_edges(T):
    pcms = [pcm_of_bits(b) for b in edge_patterns(T)]
    for kw in (dict(), dict(min_gap=3), dict(min_gap=2), dict(min_gap=200), dict(min_gap=65535), dict(min_speech=3),
               dict(min_speech=4), dict(min_speech=130), dict(hang_before=3), dict(hang_after=3),
               dict(hang_before=70, hang_after=5000), dict(hang_before=65535, hang_after=65535), SMOOTH,
               dict(min_gap=100, min_speech=80, hang_before=64, hang_after=63)):
        labs = check_units(pcms, opts_of("snip", 8, 8, **kw))
        assert all(l.shape[0] == T for l in labs)
    # the same on 16 bits
    check_units([p.astype(np.int16) for p in pcms], opts_of("snip", 8, 8, **SMOOTH))


def test_absolute_gate_long_units_and_many_workgroups():
    cases = [("snip", 400, 160, 70001), ("kaldi", 400, 160, 33333), ("center", 1200, 480, 50001),
             ("stft", 1024, 256, 30000), ("snip", 4096, 1, 9000), ("center", 2, 1, 5000), ("kaldi", 65, 72, 20000)]
    for i16 in (False, True):
        for seed, (grid, wl, hop, n) in enumerate(cases):
            x = [R.speechy(n, 100 + seed, i16), R.speechy(n // 3, 200 + seed, i16)]
            check_units(x, opts_of(grid, wl, hop))
            check_units(x, opts_of(grid, wl, hop, gate_db=26.0, reference="abs", **SMOOTH))
    # rates: the window and the hop follow each unit's own rate
    o = J.activity(25, 10, grid="kaldi", **SMOOTH)
    pcms, hz = [R.speechy(30000, 1), R.speechy(30000, 2), R.speechy(30000, 3)], [16000, 48000, 22050]
    labs, cols, _ = J.activity_pcm(pcms, hz, o)
    for x, h, lab, c in zip(pcms, hz, labs, cols):
        want, rep = J.activity_host(x, h, o)
        assert lab[:, 0].tobytes() == want.tobytes()
        R.same_report(c[0], {k: getattr(rep, k) for k in REPORT})


def programme_case(i16):
    # three members with starts that are no multiple of the hop; one muted, one of no samples; and an utterance alone
    pcms = [R.speechy(9000, 11, i16), R.speechy(7000, 12, i16), R.speechy(0, 13, i16), R.speechy(6001, 14, i16),
            R.speechy(5000, 15, i16)]
    req = [(0, 37, 0.0), (0, 4001, NINF), (0, 555, 0.0), (0, 6111, -6.0, 777), (None, 0, 0.0)]
    return pcms, req


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_programme_members_through_the_seam(grid, i16):
    pcms, req = programme_case(i16)
    _, starts, ns, _, _ = J.mix_geometry(req, [p.size for p in pcms])
    for kw in ({}, SMOOTH):
        o = opts_of(grid, 400, 160, gate_db=30.0, **kw)
        labs, cols, units = J.activity_pcm(pcms, HZ, o, req=req)
        assert len(labs) == 2 and labs[0].shape[1] == 4 and labs[1].shape[1] == 1
        f64 = [np.asarray(p, dtype=np.float64) for p in pcms]
        want, wcols, wunit = J.activity_members_host(f64[:4], starts[:4], ns[0], HZ, o, [r[2] for r in req[:4]])
        assert labs[0].tobytes() == want.tobytes(), np.argwhere(labs[0] != want)[:8]
        for c, w in zip(cols[0], wcols):
            R.same_report(c, {k: getattr(w, k) for k in REPORT})
        R.same_report(units[0], {k: getattr(wunit, k) for k in ("frames", "none", "one", "many")})
        assert not labs[0][:, 1].any() and not labs[0][:, 2].any() and labs[0][:, 0].any() and labs[0][:, 3].any()
        assert units[0].many > 0
        # the utterance alone: a programme of one at start 0 is the utterance, byte for byte
        alone = J.activity_pcm([pcms[4]], HZ, o)[0][0]
        assert labs[1].tobytes() == alone.tobytes() == J.activity_host(f64[4], HZ, o)[0].tobytes()
        one = J.activity_pcm([pcms[4]], HZ, o, req=[(0, 0, 0.0)])[0][0]
        assert one.tobytes() == alone.tobytes()


@pytest.mark.parametrize("i16", [False, True])
def test_programme_unit_column_is_the_mixture(i16):
    pcms, req = programme_case(i16)
    for fit in (False, True):
        mo = _ffi.mix_opts(fit, -6.0)
        # (with the fit the scale is the device's own: the mixture is read from the device's mix)
        mixes = J.mix_pcm(pcms, req, mo)[0] if fit else J.mix_host(pcms, req, mo)[0]
        for grid in R.GRIDS:
            o = opts_of(grid, 400, 160, gate_db=30.0, columns="unit", **SMOOTH)
            labs, cols, units = J.activity_pcm(pcms, HZ, o, req=req, mix=mo)
            assert len(labs) == len(mixes) == 2
            for p, m in enumerate(mixes):
                want, rep = J.activity_host(np.asarray(m, dtype=np.float64), HZ, o)
                assert labs[p].shape == (want.size, 1) and labs[p][:, 0].tobytes() == want.tobytes()
                R.same_report(cols[p][0], {k: getattr(rep, k) for k in REPORT})
                R.same_report(units[p], R.unit_report_of(labs[p]))


# ---- the stage in a batch, through synthesis ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


FRAMES4 = (60, 25, 90, 40)
# (programme, start, gain_db, pad_after, fade_in, fade_out): starts that are no multiple of the hop, a muted member
MIX4 = [(0, 37, 0.0, 0, 48, 48), (0, 2401, NINF, 5, 0, 0), (0, 1111, -6.0, 7, 48, 48), (None, 3, 0.0, 4)]
# (programme, pad_before, pad_after, fade_in, fade_out)
JOIN4 = [(0, 100, 7, 48, 48), (0, 0, 333, 0, 0), (1, 5, 0, 48, 48), (1, 1, 1, 0, 0)]
KINDS = {"mix": MIX4, "join": JOIN4, "none": None}


def request(b, kind):
    if kind == "mix":
        b.set_mix(MIX4)
    elif kind == "join":
        b.set_join(JOIN4)


def stems_of(b, i16):
    return [np.asarray(b.pcm_i16(u) if i16 else b.pcm(u), dtype=np.float64) for u in range(len(b))]


def check_batch_labels(b, i16, opts, kind):
    """Every unit's labels and reports are the host rule on the stems the same batch hands out, placed at member_start
    (columns="members"), or on the programme it hands out (columns="unit")"""
    joined = kind != "none"
    stems = stems_of(b, i16)
    every = b.read_activity_all()
    assert len(every) == b.num_outputs()
    out = []
    for p in range(b.num_outputs()):
        members = [u for u in range(len(b)) if (b.programme_of(u) if joined else u) == p]
        n_unit = b.programme_layout(p)[1] if joined else b.num_samples(p)
        hz = b.output_rate(members[0])
        got = b.read_activity(p)
        if opts.columns == _ffi.ACTIVITY_UNIT:
            x = b.programme_pcm(p) if joined else stems[p]
            lab, rep = J.activity_host(np.asarray(x, dtype=np.float64), hz, opts)
            want, wcols = lab.reshape(-1, 1), [rep]
        else:
            starts = [b.member_start(u) if joined else 0 for u in members]
            gains = [MIX4[u][2] if kind == "mix" else 0.0 for u in members]
            want, wcols, _ = J.activity_members_host([stems[u] for u in members], starts, n_unit, hz, opts, gains)
        assert b.activity_shape(p) == (want.shape[0], want.shape[1], hz)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (p, np.argwhere(got != want)[:8])
        assert every[p].tobytes() == got.tobytes()
        for j, w in enumerate(wcols):
            R.same_report(b.activity_report(p, j), {k: getattr(w, k) for k in REPORT})
        R.same_report(b.activity_unit_report(p), R.unit_report_of(got))
        out.append(got)
    return out


def other_outputs(b, i16, kind):
    """What the batch hands out beside the labels: the PCM, the programmes and a byte sink's streams"""
    res = [(b.pcm_i16(u) if i16 else b.pcm(u)).tobytes() for u in range(len(b))]
    if kind != "none":
        res += [b.programme_pcm(p).tobytes() for p in range(b.num_outputs())]
    res += b.flac_all() if i16 else [b.formatted(p) for p in range(b.num_outputs())]
    return res


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_batch_labels_are_the_host_rule_on_the_batch_stems(eng, tab, kind, i16):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 11 + T) for T in FRAMES4]
    opts = J.activity(25, 10, gate_db=35, grid="kaldi", **SMOOTH)

    def sinks(b):
        request(b, kind)
        if i16:
            b.set_flac(md5=True)
        else:
            b.set_format("s24", dither=True, seed=5)

    with J.Batch(vi, utts, pcm_i16=i16) as b:
        sinks(b)
        b.run()
        plain = other_outputs(b, i16, kind)
        with pytest.raises(J.JbError, match="jb_batch_set_activity was not called"):
            b.read_activity(0)
    labels = {}
    for columns in ("members", "unit"):
        opts.columns = _ffi._ACTIVITY_COLUMNS[columns]
        with J.Batch(vi, utts, pcm_i16=i16) as b:
            sinks(b)
            b.set_activity(opts)
            T, C, hz = b.activity_shape(0)  # the shape answers before the run
            assert hz == vi.sampling_frequency and C == (1 if columns == "unit" or kind == "none" else
                                                         3 if kind == "mix" else 2)
            with pytest.raises(J.JbError, match="has not run"):
                b.read_activity(0)
            b.run()
            labels[columns] = check_batch_labels(b, i16, opts, kind)
            assert other_outputs(b, i16, kind) == plain  # bit for bit the batch without the request
        assert any(l.any() for l in labels[columns])
    if kind == "mix":
        assert not labels["members"][0][:, 1].any()  # the muted member keeps its column, all zeros
    if kind == "none":
        assert all(a.tobytes() == c.tobytes() for a, c in zip(labels["members"], labels["unit"]))
    # a fast invariant batch: the same labels
    opts.columns = _ffi.ACTIVITY_MEMBERS
    for inv in (False, True):
        with J.Batch(vi, utts, pcm_i16=i16, fast_invariant=inv) as b:
            request(b, kind)
            b.set_activity(opts)
            b.run()
            got = check_batch_labels(b, i16, opts, kind)
            if not inv:
                assert all(g.tobytes() == l.tobytes() for g, l in zip(got, labels["members"]))


def test_batch_request_rules(eng, tab):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 11 + T) for T in FRAMES4[:2]]
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="grid"):
            b.set_activity(J.activity(grid=7))
        with pytest.raises(J.JbError, match="win_us"):
            b.set_activity(J.activity(win_ms=100))  # 4800 samples at 48 kHz
        with pytest.raises(J.JbError, match="jb_batch_set_activity was not called"):
            b.activity_shape(0)
        b.set_activity(J.activity())
        assert b.activity_shape(1)[1] == 1
        b.set_activity(None)  # withdrawn
        with pytest.raises(J.JbError, match="jb_batch_set_activity was not called"):
            b.activity_shape(0)
        b.set_activity(win_ms=80, hop_ms=10)  # 3840 samples at 48 kHz ...
        b.set_output_rate(96000)              # ... 7680 at this rate: refused at the first run
        with pytest.raises(J.JbError, match="win_us"):
            b.run()
    with J.Batch(vi, utts) as b:
        b.run()
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_activity(J.activity())


REDO_MIX = [(0, 100, 0.0, 0, 48, 48), (1, 3, -2.0, 5, 48, 48), (0, 2400, 3.0, 7, 48, 48), (1, 1000, 0.0, 0, 48, 48)]


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("kind", ["mix", "none"])
def test_redo_rounds_leave_no_stale_label(eng, tab, kind, i16):
    """tests/test_gpu_chain_redo.py's recipe: every hand-off of the long utterances fails, so redo rounds rewrite them
    behind the first pass of the chain; a unit with a rewritten member is measured again, whole."""
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (400, 90, 600, 30)]
    opts = J.activity(25, 10, gate_db=35, grid="center", **SMOOTH)
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        if kind == "mix":
            b.set_mix(REDO_MIX)
        b.set_activity(opts)
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 1
        joined = kind == "mix"
        stems = stems_of(b, i16)
        for p in range(b.num_outputs()):
            members = [u for u in range(len(b)) if (b.programme_of(u) if joined else u) == p]
            n_unit = b.programme_layout(p)[1] if joined else b.num_samples(p)
            starts = [b.member_start(u) if joined else 0 for u in members]
            want, wcols, wunit = J.activity_members_host([stems[u] for u in members], starts, n_unit,
                                                         vi.sampling_frequency, opts)
            got = b.read_activity(p)
            assert got.tobytes() == want.tobytes(), (p, np.argwhere(got != want)[:8])
            for j, w in enumerate(wcols):
                R.same_report(b.activity_report(p, j), {k: getattr(w, k) for k in REPORT})
            R.same_report(b.activity_unit_report(p), {k: getattr(wunit, k) for k in ("frames", "none", "one", "many")})


SENTS = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
OPTS = dict(lead_ms=12.5, trail_ms=3.3, fade_ms=5.0)


def test_engine_programme_activity(eng):
    e = eng.clone()
    hz = e._out_hz()
    parts = e.synthesize_batch(SENTS)
    opts = J.activity(25, 10, gate_db=35, grid="snip", min_gap=3, hang_after=2)
    for mix in (None, [(0.0, 0.0), (350.0, -6.5)]):
        want_pcm, want_starts = e.synthesize_programme(SENTS, mix=mix, **OPTS)
        pcm, labels, starts = e.synthesize_programme_activity(SENTS, opts, mix=mix, **OPTS)
        assert pcm.tobytes() == want_pcm.tobytes() and starts == want_starts
        want, _, _ = J.activity_members_host(parts, starts, pcm.size, hz, opts)
        assert labels.shape == want.shape and labels.tobytes() == want.tobytes()
        assert labels[:, 0].any() and labels[:, 1].any() and not labels.all()
        if mix:
            assert (labels.sum(axis=1) == 2).any()  # the talkers overlap
    whole = J.activity(25, 10, gate_db=35, columns="unit")
    pcm, labels, _ = e.synthesize_programme_activity(SENTS, whole, **OPTS)
    assert labels.shape[1] == 1 and labels[:, 0].tobytes() == J.activity_host(pcm, hz, whole)[0].tobytes()
    with pytest.raises(J.JbError, match="gate_db"):
        e.synthesize_programme_activity(SENTS, gate_db=0.0)
    assert e.get_programme_mix()[0] is None


def test_mixture_example_writes_labels_and_rttm(tmp_path):
    """examples/mixture.py --activity --rttm: the .npy matrix, and RTTM lines that are the runs of its columns"""
    out, npy, rttm = tmp_path / "mixture.wav", tmp_path / "labels.npy", tmp_path / "out.rttm"
    labs = []
    for k, s in enumerate(SENTS):
        p = tmp_path / f"s{k}.lab"
        p.write_text("\n".join(s) + "\n")
        labs.append(str(p))
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "mixture.py"), str(VOICE), *labs, "-o", str(out),
                        "--start-ms", "0,400", "--gain-db", "0,-6", "--activity", str(npy), "--rttm", str(rttm)],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    labels = np.load(npy)
    assert labels.dtype == np.uint8 and labels.shape[1] == 2 and labels[:, 0].any() and labels[:, 1].any()
    assert any(ln.startswith("activity ") for ln in r.stdout.splitlines())
    back = np.zeros_like(labels)
    for ln in rttm.read_text().splitlines():
        w = ln.split()
        assert w[0] == "SPEAKER" and w[1] == "mixture" and w[2] == "1" and w[5:7] == ["<NA>", "<NA>"] and w[8:] == ["<NA>", "<NA>"]
        a, d, j = round(float(w[3]) * 100), round(float(w[4]) * 100), int(w[7][3:])
        assert d > 0 and not back[a:a + d, j].any()
        back[a:a + d, j] = 1
    assert back.tobytes() == labels.tobytes()
