"""The limiter stage on the GPU (jb_limiter.hip): the device seam against the host seam bit for bit on the shapes of
tests/limiter_ref.py; then the stage in a batch -- bit for bit the host seam applied to the measured PCM under the
reported gain -- with groups, the converter, the filter, the join and FLAC around it; redo rounds; the fast invariant
mode; the engine entries; the report."""

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from jbonsai_amd import synth
from tests import join_ref
from tests import limiter_ref as R
from tests.conftest import VOICE
from tests.flac_meta_ref import check as flac_check
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2

pytestmark = pytest.mark.gpu

CEIL, DEPTH = -1.0, 6.0


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


def same(a, b):
    return a.dtype == b.dtype and a.size == b.size and a.tobytes() == b.tobytes()


def opts_of(case):
    o = case[4]
    return J.limiter() if o is None else J.limiter(lookahead_ms=o[0], hold_ms=o[1])


# ---- 1. the seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [F.PEAK_SAMPLE, F.PEAK_TRUE], ids=["sample", "true"])
def test_device_seam_is_the_host_seam(mode):
    """One launch with every shape (three rates, two geometries), an utterance under the ceiling, one that is not
    limited (JB_LIMITER_OFF) and one of no samples among them: f64 and 16-bit, and the report."""
    cases = R.cases()
    rng = np.random.default_rng(5)
    quiet = rng.standard_normal(2500) * 2000.0
    # (the one that is not limited at 192 kHz, where the defaults' geometry would not fit: its values are not read)
    pcms = [c[1] for c in cases] + [quiet, cases[5][1], np.zeros(0)]
    hz = [c[2] for c in cases] + [16000, 192000, 16000]
    gain = [c[3] for c in cases] + [1.0, 1.3, 1.0]
    opts = [opts_of(c) for c in cases] + [J.limiter(), J.no_limiter(), J.limiter()]
    for i16 in (False, True):
        got, reps = J.limiter_pcm(pcms, hz, gain, CEIL, mode, opts, i16=i16)
        assert len(got) == len(pcms)
        for k, x in enumerate(pcms):
            want, rep = J.limiter_host(x, hz[k], gain[k], CEIL, mode, opts[k], i16=i16)
            assert same(got[k], want), (k, i16)
            assert reps[k] == rep, (k, reps[k], rep)
        n = len(cases)
        assert all(r["limited_samples"] > 0 and r["max_reduction_db"] > 0.0 for r in reps[:n])
        assert [r["limited_samples"] for r in reps[n:]] == [0, 0, 0]
        if not i16:
            assert same(got[n], quiet) and same(got[n + 1], cases[5][1] * 1.3)


# ---- 2. the batch path ----------------------------------------------------------------------------------------------
FRAMES = (700, 1500, 900)
TARGETS = [-8.0, -45.0, -8.0]  # the second utterance stays far under the ceiling


@pytest.fixture(scope="module")
def batch_utts(eng, tab):
    return eng.voice_info(), [synth.synth_utterance(tab, t, 11 + t) for t in FRAMES]


@pytest.fixture(scope="module")
def plain_pcm(batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        b.run()
        return [b.pcm(i) for i in range(len(utts))]


def applied(vi, utts, targets, ceiling, mode=None, groups=None, **kw):
    """What the limiter reads, u = x g, from the code in front of this stage: the same batch without the request under
    a ceiling that much higher runs the same gain rule (min(T - L, C + depth - P)) and the plain apply pass.  Returns
    (u, the reported gains, the native PCM)."""
    with J.Batch(vi, utts, **kw) as b:
        if mode is not None:
            b.set_peak_mode(mode)
        b.set_loudness_target(targets, ceiling)
        if groups is not None:
            b.set_loudness_groups(groups)
        b.run()
        b.sync()
        n = len(utts)
        return [b.pcm(i) for i in range(n)], [b.loudness(i)[2] for i in range(n)], [b.pcm_native(i) for i in range(n)]


def test_batch_is_the_host_seam_bit_for_bit(batch_utts, plain_pcm):
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    lim = J.limiter(max_reduction_db=DEPTH)
    with J.Batch(vi, utts) as b:
        b.set_limiter(lim)
        b.set_loudness_target(TARGETS, CEIL)
        b.run()
        got = [b.pcm(i) for i in range(3)]
        reps = [b.limiter_report(i) for i in range(3)]
        gains = [b.loudness(i) for i in range(3)]
        with pytest.raises(J.JbError, match="before the batch's first run"):
            b.set_limiter(lim)
    # the static gain: min(T - L, C + depth - P), reported as before
    for i, (lufs, peak, gain) in enumerate(gains):
        assert abs(gain - min(TARGETS[i] - lufs, CEIL + DEPTH - peak)) <= 1e-12
    c = 32768.0 * 10.0 ** (CEIL / 20.0)
    u, ugains, _ = applied(vi, utts, TARGETS, CEIL + DEPTH)
    for i in range(3):
        assert ugains[i] == gains[i][2]  # the reported gain is the one u was made with
        np.testing.assert_allclose(u[i], plain_pcm[i] * 10.0 ** (gains[i][2] / 20.0), rtol=1e-15, atol=0)  # (the device's pow against the host's)
        want, rep = J.limiter_host(u[i], hz, 1.0, CEIL, F.PEAK_SAMPLE, lim)
        assert same(got[i], want), i
        assert reps[i] == rep, (i, reps[i], rep)
        assert np.max(np.abs(got[i])) <= c
    print("limited samples", [r["limited_samples"] for r in reps], "reduction", [r["max_reduction_db"] for r in reps])
    assert reps[0]["limited_samples"] > 0 and reps[2]["limited_samples"] > 0 and reps[1]["limited_samples"] == 0
    # the utterance that is not limited: the bytes of the same batch without the request
    with J.Batch(vi, utts) as b:
        b.set_loudness_target(TARGETS, CEIL)
        b.run()
        assert same(b.pcm(1), got[1]) and not same(b.pcm(0), got[0])
        nolim = [b.pcm(i) for i in range(3)]
        with pytest.raises(J.JbError, match="jb_batch_set_limiter"):
            b.limiter_report(0)
    # a request that is withdrawn, JB_LIMITER_OFF or without depth: that batch, bit for bit
    for req in (None, [None, None, None], J.limiter(max_reduction_db=0.0)):
        with J.Batch(vi, utts) as b:
            b.set_limiter(lim)
            b.set_limiter(req)
            b.set_loudness_target(TARGETS, CEIL)
            b.run()
            assert all(same(b.pcm(i), nolim[i]) for i in range(3))
            if req is not None:  # a request that limits no utterance is no request: nothing was limited
                assert b.limiter_report(0) == {"max_reduction_db": 0.0, "limited_samples": 0, "lookahead": 0, "hold": 0}
    # per utterance: the one without a request gets the plain apply pass
    with J.Batch(vi, utts) as b:
        b.set_loudness_target(TARGETS, CEIL)
        b.set_limiter([lim, None, None])
        b.run()
        assert same(b.pcm(0), got[0]) and same(b.pcm(1), nolim[1]) and same(b.pcm(2), nolim[2])
        assert b.limiter_report(2) == {"max_reduction_db": 0.0, "limited_samples": 0, "lookahead": 0, "hold": 0}
    # 16 bits and the true-peak mode: the host seam's forms under the gain of the f64 run
    with J.Batch(vi, utts, pcm_i16=True) as b:
        b.set_limiter(lim)
        b.set_loudness_target(TARGETS, CEIL)
        b.run()
        for i in range(3):
            assert same(b.pcm_i16(i), J.limiter_host(u[i], hz, 1.0, CEIL, 0, lim, i16=True)[0]), i
    with J.Batch(vi, utts) as b:
        b.set_peak_mode(F.PEAK_TRUE)
        b.set_limiter(lim)
        b.set_loudness_target(TARGETS, CEIL)
        b.run()
        ut, tgains, _ = applied(vi, utts, TARGETS, CEIL + DEPTH, mode=F.PEAK_TRUE)
        for i in range(3):
            want, rep = J.limiter_host(ut[i], hz, 1.0, CEIL, F.PEAK_TRUE, lim)
            assert tgains[i] == b.loudness(i)[2]
            assert same(b.pcm(i), want) and b.limiter_report(i) == rep, i
    # without a target the request has no effect
    with J.Batch(vi, utts) as b:
        b.set_limiter(lim)
        b.run()
        assert all(same(b.pcm(i), plain_pcm[i]) for i in range(3))


def test_refusals(batch_utts):
    vi, utts = batch_utts
    with J.Batch(vi, utts) as b:
        with pytest.raises(J.JbError, match="one request, or one per utterance"):
            b.set_limiter([J.limiter(), J.limiter()])
        with pytest.raises(J.JbError, match="utterance 1: hold_ms"):
            b.set_limiter([J.limiter(), J.limiter(hold_ms=60.0), None])
        # a mixed group is refused by whichever setter comes second, naming the group and the field
        b.set_loudness_target(-20.0, CEIL)
        b.set_loudness_groups([2, 2, None])
        with pytest.raises(J.JbError, match="group 2 would disagree on the limiter's max_reduction_db"):
            b.set_limiter([J.limiter(), J.limiter(max_reduction_db=3.0), J.limiter(hold_ms=1.0)])
        b.set_limiter([J.limiter(), J.limiter(), J.limiter(hold_ms=1.0)])
        with pytest.raises(J.JbError, match="group 1 would disagree on the limiter's hold_ms"):
            b.set_loudness_groups([None, 1, 1])
        with pytest.raises(J.JbError, match="has not run"):
            b.limiter_report(0)
    with J.Batch(vi, utts, mlpg_only=True) as b:
        with pytest.raises(J.JbError, match="no PCM"):
            b.set_limiter(J.limiter())
    # 2 L + H above 2048 samples at the output rate: refused at the run
    with J.Batch(vi, utts[:1]) as b:
        b.set_output_rate(96000)
        b.set_loudness_target(-8.0, CEIL)
        b.set_limiter(J.limiter(lookahead_ms=10.0, hold_ms=8.0))
        with pytest.raises(J.JbError, match="2 L \\+ H") as e:
            b.run()
        assert e.value.code == -2


def test_a_group_spans_limited_and_unlimited_members(batch_utts, plain_pcm):
    """One gain for the three: it puts the group's highest peak half a dB over the ceiling, so the member that holds it
    is limited and a member whose own peak is lower by more than that is not."""
    vi, utts = batch_utts
    hz = vi.sampling_frequency
    lim = J.limiter(max_reduction_db=0.5)
    with J.Batch(vi, utts) as b:
        b.set_loudness_groups([0, 0, 0])
        b.set_limiter(lim)
        b.set_loudness_target(-8.0, CEIL)
        b.run()
        grp = b.loudness_group(0)
        assert abs(grp["gain_db"] - (CEIL + 0.5 - grp["sample_peak_dbfs"])) <= 1e-12
        reps = [b.limiter_report(i) for i in range(3)]
        print("peaks", [b.loudness(i)[1] for i in range(3)], "limited", [r["limited_samples"] for r in reps])
        assert any(r["limited_samples"] > 0 for r in reps) and any(r["limited_samples"] == 0 for r in reps)
        assert len({b.loudness(i)[2] for i in range(3)}) == 1
        u, ugains, _ = applied(vi, utts, -8.0, CEIL + 0.5, groups=[0, 0, 0])
        for i in range(3):
            want, rep = J.limiter_host(u[i], hz, 1.0, CEIL, 0, lim)
            assert ugains[i] == grp["gain_db"]
            assert same(b.pcm(i), want) and reps[i] == rep, i


def test_with_rate_filter_join_and_flac(batch_utts):
    """Everything on: the FLAC stream decodes to the join of the limited 16-bit members.  What the limiter reads is the
    product of the same chain without the request under a ceiling DEPTH higher: the same gain rule, the same bits."""
    vi, utts = batch_utts
    hp, lim = J.highpass(70.0), J.limiter(max_reduction_db=DEPTH)
    req = [(0, 100, 3, 48, 48), (0, 7, 500, 48, 48), (0, 1, 1, 0, 0)]

    def chain(b):
        b.set_output_rate(8000)
        b.set_filter(hp)
    with J.Batch(vi, utts) as b:
        chain(b)
        b.set_loudness_target(-8.0, CEIL + DEPTH)
        b.run()
        u = [b.pcm(i) for i in range(3)]
    with J.Batch(vi, utts, pcm_i16=True) as b:
        chain(b)
        b.set_loudness_target(-8.0, CEIL)
        b.set_limiter(lim)
        b.set_join(req)
        b.set_flac(md5=True)
        b.run()
        parts = [b.pcm_i16(i) for i in range(3)]
        for i in range(3):
            want, rep = J.limiter_host(u[i], 8000, 1.0, CEIL, 0, lim, i16=True)
            assert same(parts[i], want), i
            assert b.limiter_report(i) == rep and rep["lookahead"] == 16 and rep["hold"] == 64
        assert sum(b.limiter_report(i)["limited_samples"] for i in range(3)) > 0
        (prog,), _, _ = join_ref.join(parts, req)
        dec, _, meta = flac_check(b.flac(0))
        assert b.num_outputs() == 1 and np.array_equal(dec, prog) and meta["total"] == prog.size


# ---- 3. redo rounds -------------------------------------------------------------------------------------------------
def test_redo_rounds_limit_the_final_pcm(eng, tab):
    """Every hand-off fails (2-frame warm-up, a tolerance of 1e-12): redo rounds rewrite most chunks after run() has
    limited the first PCM.  The output is the host seam applied to the final native PCM under the final gain.  Once more
    under a group with a third member of 80 frames: one chunk, no hand-off, so the vocoder never rewrites it, and yet
    its group's second measurement gives it a new gain -- the limiter's redo list follows `post`, not `measured`."""
    vi = eng.voice_info()
    hz = vi.sampling_frequency
    lim = J.limiter(max_reduction_db=DEPTH)
    kw = dict(chunk_frames=96, warmup_frames=2, verify_tol=1e-12)
    for frames, group in (((600, 1100), None), ((600, 1100, 80), [0, 0, 0])):
        utts = [synth.synth_utterance(tab, t, 40 + t) for t in frames]
        n = len(utts)
        u, ugains, unative = applied(vi, utts, -8.0, CEIL + DEPTH, groups=group, **kw)
        with J.Batch(vi, utts, **kw) as b:
            b.set_limiter(lim)
            b.set_loudness_target(-8.0, CEIL)
            if group:
                b.set_loudness_groups(group)
            b.run()
            b.sync()
            assert b.info()["n_redo"] >= 4 and b.info()["chunk_frames"] == 96
            limited = 0
            for i in range(n):
                assert same(b.pcm_native(i), unative[i]) and b.loudness(i)[2] == ugains[i]
                want, rep = J.limiter_host(u[i], hz, 1.0, CEIL, 0, lim)
                assert same(b.pcm(i), want), (group, i)
                assert b.limiter_report(i) == rep
                limited += rep["limited_samples"]
            assert limited > 0
            if group:
                assert len({b.loudness(i)[2] for i in range(n)}) == 1


# ---- 4. invariance --------------------------------------------------------------------------------------------------
def test_invariance_alone_and_among_64(eng, tab):
    vi = eng.voice_info()
    probe = synth.synth_utterance(tab, 900, 77)
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(63)]
    pl = J.limiter(max_reduction_db=DEPTH)
    ol = [[J.limiter(), None, J.limiter(lookahead_ms=1.0, hold_ms=0.0, max_reduction_db=3.0)][k % 3] for k in range(63)]
    res = []
    for utts, lims, pos in (([probe], [pl], 0), (others[:20] + [probe] + others[20:], ol[:20] + [pl] + ol[20:], 20)):
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_limiter(lims)
            b.set_loudness_target(-8.0, CEIL)
            b.run()
            res.append((b.pcm(pos).tobytes(), b.limiter_report(pos)))
    assert res[0] == res[1] and len(res[0][0]) == 8 * 900 * vi.fperiod
    assert res[0][1]["limited_samples"] > 0


# ---- 5. the engine entries ------------------------------------------------------------------------------------------
def test_engine_entries(eng):
    """An engine with a target, a ceiling and a limiter against the same engine without the limiter under a ceiling
    DEPTH higher (the same static gain): the host seam over that output under a gain of 1."""
    hz = eng._out_hz()
    sents = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    lim = J.limiter(max_reduction_db=DEPTH)
    eu = eng.clone()
    eu.condition.set_loudness_target(-8.0)
    eu.condition.set_peak_ceiling(CEIL + DEPTH)
    el = eng.clone()
    el.condition.set_loudness_target(-8.0)
    el.condition.set_peak_ceiling(CEIL)
    assert el.get_limiter() is None
    el.set_limiter(lim)
    o = el.clone().get_limiter()  # copied with the Condition
    assert (o.lookahead_ms, o.hold_ms, o.max_reduction_db, o.flags) == (2.0, 8.0, DEPTH, F.LIMITER_EXACT)
    with pytest.raises(J.JbError, match="lookahead_ms"):
        el.set_limiter(J.limiter(lookahead_ms=11.0))
    u = [np.array(x) for x in eu.synthesize_batch(sents)]
    want = [J.limiter_host(x, hz, 1.0, CEIL, 0, lim)[0] for x in u]
    want16 = [J.limiter_host(x, hz, 1.0, CEIL, 0, lim, i16=True)[0] for x in u]
    assert any(not same(w, x) for w, x in zip(want, u))  # something is limited
    assert same(el.synthesize(SAMPLE_SENTENCE_1), want[0])
    assert all(same(np.array(g), w) for g, w in zip(el.synthesize_batch(sents), want))
    assert all(same(np.array(g), w) for g, w in zip(el.synthesize_batch(sents, i16=True), want16))
    # the generator: no serially served head, the whole utterance through the chain
    assert same(el.generator(SAMPLE_SENTENCE_1).generate_all(), want[0])
    # _each: each engine's own request; an engine without one gets the plain apply pass
    ec = eng.clone()
    ec.condition.set_loudness_target(-8.0)
    ec.condition.set_peak_ceiling(CEIL)
    plain = [np.array(x) for x in ec.synthesize_batch(sents)]
    each = J.synthesize_batch_each([el, ec], sents)
    assert same(np.array(each[0]), want[0]) and same(np.array(each[1]), plain[1])
    # a programme: the join of the limited members
    prog, starts = el.synthesize_programme(sents, gap_ms=100.0)
    (wprog,), _, wstarts = join_ref.join(want, join_ref.chapter([x.size for x in want], hz, gap_ms=100.0))
    assert same(np.array(prog), wprog.astype(np.float64)) and starts == wstarts
    # without a target, or with the request withdrawn, every entry returns what it did
    el.set_limiter(None)
    assert el.get_limiter() is None
    assert all(same(np.array(g), w) for g, w in zip(el.synthesize_batch(sents), plain))
    en = eng.clone()
    en.set_limiter(lim)
    base = [np.array(x) for x in eng.synthesize_batch(sents)]
    assert all(same(np.array(g), w) for g, w in zip(en.synthesize_batch(sents), base))
