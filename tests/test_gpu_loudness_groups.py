"""Programme loudness on the GPU (jb_loudness.hip: k_ln_gate_group, k_ln_windows, k_ln_range): one measurement, one
peak and one gain per group of utterances, the R128 report, the redo closure, the fast invariant mode, the output
rate and the engine's per-request scope, against the numpy reference (tests/loudness_groups_ref.py).

Tolerances: loudness values 1e-8 LU (close_lu of tests/test_gpu_loudness.py), sample peaks 1e-12 dB and true peaks
1e-10 dB (tests/test_gpu_true_peak.py).  The reference asserts that no block or window lies within 1e-6 LU of a gate
it is compared with: a condition on the inputs, met by the seeds below."""
import math

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F
from jbonsai_amd import synth
from tests import flac_ref
from tests import loudness_groups_ref as R
from tests.conftest import VOICE
from tests.flac_meta_ref import split
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.loudness_ref import integrated
from tests.test_gpu_flac_meta import md5_of
from tests.test_gpu_loudness import close_lu, same_bits
from tests.true_peak_ref import true_peak, true_peak_lin

pytestmark = pytest.mark.gpu

IN = 48000
LU_TOL, PEAK_TOL, TP_TOL = 1e-8, 1e-12, 1e-10
DB12 = 10.0 ** (12.0 / 20.0)


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


@pytest.fixture(scope="module")
def tab(eng):
    return synth.VoiceTables(eng)


def close(got, want, tol):
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got), (got, want)
    else:
        close_lu(got, want, tol)


def check_group(got, want, tp_tol=TP_TOL):
    close(got["lufs"], want["lufs"], LU_TOL)
    close(got["sample_peak_dbfs"], want["sample_peak_dbfs"], PEAK_TOL)
    close(got["true_peak_dbtp"], want["true_peak_dbtp"], tp_tol)
    close(got["gain_db"], want["gain_db"], LU_TOL)


def check_r128(got, want):
    assert got["n_windows"] == want["n_windows"], (got, want)
    for k in ("max_momentary_lufs", "max_short_term_lufs", "lra_lu", "lra_low_lufs", "lra_high_lufs"):
        close(got[k], want[k], LU_TOL)


def measured(pcms, hz):
    """(hop energies, hop, largest magnitudes) of PCM: each utterance through the reference's filter once."""
    zs = [R.hop_energies(x, hz)[0] for x in pcms]
    return zs, R.hop_energies(np.zeros(0), hz)[1], [float(np.max(np.abs(x))) if len(x) else 0.0 for x in pcms]


def sample_peak_db(x):
    return R.db(float(np.max(np.abs(x))))


def members_of(b, n):
    groups = {}
    for i in range(n):
        groups.setdefault(b.loudness_group_of(i), []).append(i)
    return groups


def volumes(vi, factors):
    return [(vi.alpha, vi.beta, vi.volume * f) for f in factors]


# ---- 1. interleaved groups ------------------------------------------------------------------------------------------
FRAMES7 = (640, 70, 300, 700, 610, 120, 650)   # 70: under 4 hops (peak only); 120, 300: blocks, no window
GROUPS7 = (4, 2, 4, None, 4, 2, 4)             # a group of 4, one of 2 and one utterance of its own, interleaved
VOLS7 = (1.0, DB12, 1.0 / DB12, 1.0, DB12, 1.0, 1.0)


@pytest.mark.parametrize("i16", [False, True])
def test_interleaved_groups(eng, tab, i16):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 600 + T) for T in FRAMES7]
    target = -20.0
    with J.Batch(vi, utts, voc=volumes(vi, VOLS7), pcm_i16=i16) as b:
        b.set_loudness_groups(GROUPS7)
        b.set_loudness_target(target, math.inf)
        b.run()
        b.sync()
        assert [b.loudness_group_of(i) for i in range(7)] == [0, 1, 0, 2, 0, 1, 0]
        nat = [b.pcm_native(i) for i in range(7)]
        zs, H, peaks = measured(nat, IN)
        for g, mem in members_of(b, 7).items():
            want = R.group([zs[i] for i in mem], H, [peaks[i] for i in mem], None, target, math.inf)
            rep = b.loudness_group(mem[0])
            check_group(rep, want)
            assert rep["members"] == len(mem) and rep["flags"] == 0 and rep["peak_mode"] == 0
            gain = rep["gain_db"]
            outs = []
            for i in mem:
                assert repr(b.loudness_group(i)) == repr(rep)  # (repr: NaN true peaks compare equal)
                # the utterance's own L and P stay in its report; the gain applied is the group's, the identical f64
                lufs, peak, g_i = b.loudness(i)
                own = R.group([zs[i]], H, [peaks[i]])
                close_lu(lufs, own["lufs"], LU_TOL)
                close_lu(peak, own["sample_peak_dbfs"], PEAK_TOL)
                assert g_i == gain
                scaled = nat[i] * 10.0 ** (gain / 20.0)
                if i16:
                    same_bits(b.pcm_i16(i), np.clip(scaled, -32768.0, 32767.0).astype(np.int16))
                else:
                    np.testing.assert_allclose(b.pcm(i), scaled, rtol=1e-15, atol=0)
                    outs.append(b.pcm(i))
            if outs:  # f64: the group of the outputs sits on the target
                close_lu(R.group_of_pcm(outs, IN)[0]["lufs"], target, 1e-6)
        # the relative levels inside the group of four survived: 12 dB apart stays 12 dB apart
        assert b.loudness(0)[2] == b.loudness(2)[2] == b.loudness(4)[2] == b.loudness(6)[2]


# ---- 2. no behaviour change -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True])
def test_group_of_one_and_no_group_change_nothing(eng, tab, i16):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 900 + T) for T in (700, 90, 1300)]
    res = []
    for groups in (False, [None, None, None], [2, None, 0]):
        with J.Batch(vi, utts, pcm_i16=i16) as b:
            b.set_loudness_target([-16.0, -30.0, -23.0], -0.5)
            b.set_peak_mode([0, 1, 0])
            if groups is not False:
                b.set_loudness_groups(groups)
            b.run()
            b.sync()
            assert b.loudness_group_of(1) == (-1 if groups is False else 1)
            res.append((b.pcm_all(), [b.loudness_report(i) for i in range(3)]))
            if groups is not False:
                for i in range(3):
                    rep, own = b.loudness_group(i), b.loudness_report(i)
                    assert rep["members"] == 1
                    for k in ("lufs", "sample_peak_dbfs", "gain_db", "peak_mode", "oversampling"):
                        assert rep[k] == own[k], (i, k)
                    assert rep["true_peak_dbtp"] == own["true_peak_dbtp"] or i != 1
    for pcm, reports in res[1:]:
        for a, c in zip(pcm, res[0][0]):
            same_bits(a, c)
        assert repr(reports) == repr(res[0][1])  # (repr: NaN true peaks compare equal)


# ---- 3. the ceiling binds on the loudest member ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", [F.PEAK_SAMPLE, F.PEAK_TRUE])
def test_ceiling_binds_on_the_loudest_member(eng, tab, mode):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 300 + T) for T in (400, 650, 200)]
    C_ = -1.0
    with J.Batch(vi, utts, voc=volumes(vi, (1.0, DB12, 1.0 / DB12))) as b:
        b.set_loudness_target(0.0, C_)
        b.set_peak_mode(mode)
        b.set_loudness_groups([0, 0, 0])
        b.run()
        b.sync()
        nat = [b.pcm_native(i) for i in range(3)]
        tps = [true_peak_lin(x, IN) for x in nat] if mode == F.PEAK_TRUE else None
        want, _, _ = R.group_of_pcm(nat, IN, tps, 0.0, C_)
        rep = b.loudness_group(0)
        check_group(rep, want)
        own = [b.loudness_report(i) for i in range(3)]
        key = "true_peak_dbtp" if mode == F.PEAK_TRUE else "sample_peak_dbfs"
        peaks = [r[key] for r in own]
        loudest = int(np.argmax(peaks))
        assert rep[key] == max(peaks) and rep["peak_mode"] == mode
        assert rep["oversampling"] == (4 if mode == F.PEAK_TRUE else 1)
        assert rep["gain_db"] == pytest.approx(C_ - max(peaks), abs=1e-12) and rep["gain_db"] < 0.0 - rep["lufs"]
        out = [b.pcm(i) for i in range(3)]
        for i in range(3):
            np.testing.assert_allclose(out[i], nat[i] * 10.0 ** (rep["gain_db"] / 20.0), rtol=1e-15, atol=0)
        # the loudest member sits on the ceiling, the others under it
        if mode == F.PEAK_TRUE:
            assert abs(true_peak(out[loudest], IN) - C_) <= 1e-9
        else:
            assert abs(sample_peak_db(out[loudest]) - C_) <= 1e-9
        assert all(sample_peak_db(out[i]) < C_ for i in range(3) if i != loudest)


# ---- 4. the redo closure --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True])
def test_redo_reaches_every_member_of_a_touched_group(eng, tab, i16):
    """Every hand-off of the long member fails, so redo rounds rewrite it after run() measured the group; the short
    member has one chunk, no hand-off, and is never touched.  Both must carry the FINAL group gain, and what is
    encoded behind the apply pass must be the short member's final PCM as well."""
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 40 + T) for T in (1100, 90, 400)]
    target = -21.0
    with J.Batch(vi, utts, chunk_frames=96, warmup_frames=2, verify_tol=1e-12, pcm_i16=i16) as b:
        b.set_loudness_target(target, math.inf)
        b.set_loudness_groups([0, 0, None])
        b.set_loudness_report()
        if i16:
            b.set_flac(md5=True)
        else:
            b.set_format("s16")
            b.set_adpcm()
        b.run()
        b.sync()
        assert b.info()["n_redo"] >= 4
        nat = [b.pcm_native(i) for i in range(3)]
        want, want_r, want_m = R.group_of_pcm(nat[:2], IN, None, target, math.inf)
        rep = b.loudness_group(1)
        check_group(rep, want)
        assert repr(rep) == repr(b.loudness_group(0)) and rep["members"] == 2 and rep["flags"] == F.LOUDNESS_R128
        check_r128(rep["r128"], want_r)
        for i in range(2):
            check_r128(b.loudness_r128(i), want_m[i])
        for i in range(3):
            gain = b.loudness(i)[2]
            assert gain == (rep["gain_db"] if i < 2 else b.loudness_group(2)["gain_db"])
            scaled = nat[i] * 10.0 ** (gain / 20.0)
            if i16:
                pcm = b.pcm_i16(i)
                same_bits(pcm, np.clip(scaled, -32768.0, 32767.0).astype(np.int16))
                meta, plain = split(b.flac(i))  # (the strict decoder takes the plain form: a zeroed digest)
                dec, _ = flac_ref.decode(plain)
                assert np.array_equal(dec, pcm)
                assert meta["md5"] == md5_of(pcm)
            else:
                np.testing.assert_allclose(b.pcm(i), scaled, rtol=1e-15, atol=0)
                assert b.formatted(i) == J.format_pcm_host(b.pcm(i), "s16")
                assert b.read_adpcm(i) == J.adpcm_encode_host(b.pcm(i), IN, 0)
        if not i16:
            close_lu(R.group_of_pcm([b.pcm(0), b.pcm(1)], IN)[0]["lufs"], target, 1e-6)


# ---- 5. invariance --------------------------------------------------------------------------------------------------
def test_group_alone_and_among_60(eng, tab):
    vi = eng.voice_info()
    probe = [synth.synth_utterance(tab, T, 77 + T) for T in (900, 100, 640)]
    others = [synth.synth_utterance(tab, 150 + 37 * k, 1000 + k) for k in range(60)]
    res = []
    for utts, pos in ((probe, (0, 1, 2)),
                      (others[:7] + [probe[0]] + others[7:30] + [probe[1]] + others[30:41] + [probe[2]] + others[41:],
                       (7, 31, 43))):
        groups = [None] * len(utts)
        for k, p in enumerate(pos):
            groups[p] = pos[2]  # any id: the group is its members
        for k in range(0, len(utts), 9):
            if groups[k] is None:
                groups[k] = 0  # a second group around them
        with J.Batch(vi, utts, fast_invariant=True) as b:
            b.set_loudness_target(-19.0, -2.0)
            b.set_loudness_groups(groups)
            b.set_loudness_report()
            b.run()
            b.sync()
            res.append(([b.pcm(p) for p in pos], [b.loudness_report(p) for p in pos], b.loudness_group(pos[0]),
                        [b.loudness_r128(p) for p in pos]))
    for a, c in zip(res[0][0], res[1][0]):
        same_bits(a, c)
    assert repr(res[0][1:]) == repr(res[1][1:])


# ---- 6. the output rate ---------------------------------------------------------------------------------------------
def test_group_is_measured_at_the_output_rate(eng, tab):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 300 + T) for T in (700, 1300, 200)]
    with J.Batch(vi, utts) as b:
        b.set_output_rate(16000)
        b.set_loudness_target(-18.0, math.inf)
        b.set_loudness_groups([1, 1, 1])
        b.set_loudness_report()
        b.run()
        b.sync()
        conv = [J.resample(b.pcm_native(i), IN, 16000) for i in range(3)]
        want, want_r, want_m = R.group_of_pcm(conv, 16000, None, -18.0, math.inf)
        rep = b.loudness_group(2)
        check_group(rep, want)
        check_r128(rep["r128"], want_r)
        for i in range(3):
            check_r128(b.loudness_r128(i), want_m[i])
            np.testing.assert_allclose(b.pcm(i), conv[i] * 10.0 ** (rep["gain_db"] / 20.0), rtol=1e-15, atol=0)
    # a call that would leave a group mixed is refused, whichever call comes last, and the request stays as it was
    with J.Batch(vi, utts) as b:
        b.set_loudness_groups([1, 1, None])
        with pytest.raises(J.JbError, match="group 1 would disagree on the output rate"):
            b.set_output_rate([16000, 8000, 16000])
        b.set_output_rate([16000, 16000, 8000])
        with pytest.raises(J.JbError, match="group 1 would disagree on the target"):
            b.set_loudness_target([-16.0, -18.0, -16.0])
        b.set_loudness_target([-16.0, -16.0, math.nan])
        with pytest.raises(J.JbError, match="group 1 would disagree on the peak mode"):
            b.set_peak_mode([0, 1, 1])
        with pytest.raises(J.JbError, match="group 0 would disagree on the target"):
            b.set_loudness_groups([0, None, 0])
        with pytest.raises(J.JbError, match="group id 3"):
            b.set_loudness_groups([0, 3, 0])
        with pytest.raises(J.JbError):
            b.set_loudness_groups([0, 0])
        assert [b.loudness_group_of(i) for i in range(3)] == [0, 0, 1]
        with pytest.raises(J.JbError):
            b.loudness_group(0)  # not run yet
        b.run()
        b.sync()
        assert b.loudness_group(0)["members"] == 2 and b.loudness_group(2)["members"] == 1
        with pytest.raises(J.JbError):
            b.loudness_r128(0)  # no report was asked for
        with pytest.raises(J.JbError):
            b.set_loudness_groups([0, 0, 0])  # after the first run


# ---- 7. the R128 report ---------------------------------------------------------------------------------------------
def programme(rng, n, hz, level):
    """Noise under a slow swing of the level: something with a loudness range."""
    t = np.arange(n) / hz
    env = 10.0 ** ((8.0 * np.sin(2 * np.pi * t / 7.3 + rng.uniform(0, 6))) / 20.0)
    return rng.standard_normal(n) * level * env


def test_r128_report_of_a_batch(eng, tab):
    vi = eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 500 + T) for T in (1300, 90, 590, 620, 1000)]
    with J.Batch(vi, utts, voc=volumes(vi, (1.0, 1.0, DB12, 1.0, 1.0 / DB12))) as b:
        b.set_loudness_target(math.nan, math.inf)
        b.set_loudness_groups([0, 0, 0, 1, 1])
        b.set_loudness_report()
        b.run()
        b.sync()
        nat = [b.pcm_native(i) for i in range(5)]
        for mem in ([0, 1, 2], [3, 4]):
            want, want_r, want_m = R.group_of_pcm([nat[i] for i in mem], IN)
            rep = b.loudness_group(mem[0])
            check_group(rep, want)
            assert rep["gain_db"] == 0.0
            check_r128(rep["r128"], want_r)
            for i, w in zip(mem, want_m):
                check_r128(b.loudness_r128(i), w)
                same_bits(b.pcm(i), nat[i])
        assert b.loudness_r128(1)["max_momentary_lufs"] > -70 and b.loudness_r128(1)["n_windows"] == 0
        assert b.loudness_r128(2)["max_short_term_lufs"] == -math.inf  # 590 frames: 29 hops
        assert b.loudness_r128(3)["max_short_term_lufs"] > -70          # 620 frames: 31 hops, 2 windows
    # the report without groups: per utterance only
    with J.Batch(vi, utts[:2]) as b:
        b.set_loudness_target(-20.0)
        b.set_loudness_report()
        b.run()
        b.sync()
        check_r128(b.loudness_r128(0), R.group_of_pcm([b.pcm_native(0)], IN)[2][0])
        with pytest.raises(J.JbError):
            b.loudness_group(0)


def test_r128_seam_edges_at_8k():
    """nh = 3, 29, 30 and 31 exactly (H = 800 at 8 kHz), each alone and as one group."""
    rng = np.random.default_rng(29)
    hz, H = 8000, 800
    sigs = [programme(rng, nh * H + 17, hz, 2500.0) for nh in (3, 29, 30, 31)]
    got = J.loudness_groups(sigs, hz, [None, None, None, None])
    assert got["group_of"] == [0, 1, 2, 3]
    for i, x in enumerate(sigs):
        want, want_r, _ = R.group_of_pcm([x], hz)
        check_group(got["groups"][i], want)
        check_r128(got["groups"][i]["r128"], want_r)
        check_r128(got["r128"][i], want_r)
        close_lu(got["lufs"][i], want["lufs"], LU_TOL)
    assert [r["n_windows"] for r in got["r128"]] == [0, 0, 1, 2]
    assert got["r128"][0]["max_momentary_lufs"] == -math.inf and got["r128"][1]["max_momentary_lufs"] > -70
    assert got["r128"][1]["max_short_term_lufs"] == -math.inf
    assert got["r128"][2]["lra_lu"] == 0.0 and got["r128"][2]["lra_low_lufs"] == got["r128"][2]["max_short_term_lufs"]
    one = J.loudness_groups(sigs, hz, [3, 3, 3, 3], mode=F.PEAK_TRUE, target=-14.0, ceiling=-2.0)
    assert one["group_of"] == [0, 0, 0, 0] and len(one["groups"]) == 1
    want, want_r, want_m = R.group_of_pcm(sigs, hz, [true_peak_lin(x, hz) for x in sigs], -14.0, -2.0)
    check_group(one["groups"][0], want)
    assert one["groups"][0]["members"] == 4 and one["groups"][0]["oversampling"] == 24
    check_r128(one["groups"][0]["r128"], want_r)
    for g, w in zip(one["r128"], want_m):
        check_r128(g, w)


def test_r128_seam_selection_over_more_values_than_threads():
    """5 x 40 s at 8 kHz, two members identical: 5 x 371 windows, so every lane of the selection holds several values
    and the duplicates tie."""
    rng = np.random.default_rng(31)
    hz, H, n = 8000, 800, 40 * 8000
    four = [programme(rng, n, hz, 3000.0 * 10.0 ** (-k / 4.0)) for k in range(4)]
    sigs = [four[0], four[1], four[2], four[1].copy(), four[3]]
    z4 = [R.hop_energies(x, hz)[0] for x in four]
    zs = [z4[0], z4[1], z4[2], z4[1], z4[3]]
    peaks = [float(np.max(np.abs(x))) for x in sigs]
    got = J.loudness_groups(sigs, hz, [0, 0, 0, 0, 0], target=-23.0)
    check_group(got["groups"][0], R.group(zs, H, peaks, None, -23.0, math.inf))
    want_r = R.r128(zs, H)
    assert want_r["n_windows"] > 1024
    check_r128(got["groups"][0]["r128"], want_r)
    for i in range(5):
        check_r128(got["r128"][i], R.r128([zs[i]], H))
    assert repr(got["r128"][1]) == repr(got["r128"][3])


# ---- 8. the engine --------------------------------------------------------------------------------------------------
def scoped(eng, target=-20.0, ceiling=math.inf, scope=F.LOUDNESS_PER_REQUEST, **kw):
    e = eng.clone()
    e.condition.set_loudness_target(target)
    e.condition.set_peak_ceiling(ceiling)
    e.set_loudness_scope(scope)
    for k, v in kw.items():
        getattr(e.condition, "set_" + k)(v)
    return e


def test_engine_per_request_scope(eng):
    texts = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    assert eng.get_loudness_scope() == F.LOUDNESS_PER_UTTERANCE
    e = scoped(eng)
    assert e.get_loudness_scope() == F.LOUDNESS_PER_REQUEST and e.clone().get_loudness_scope() == F.LOUDNESS_PER_REQUEST
    with pytest.raises(J.JbError):
        e.set_loudness_scope(2)
    got = e.synthesize_batch(texts)
    with J.Batch(eng.voice_info(), [eng.states(t) for t in texts]) as b:
        b.set_loudness_target(-20.0, math.inf)
        b.set_loudness_groups([0, 0])
        b.run()
        b.sync()
        for i in range(2):
            same_bits(np.asarray(got[i]), b.pcm(i))
        assert b.loudness(0)[2] == b.loudness(1)[2]
    close_lu(R.group_of_pcm([np.asarray(x) for x in got], IN)[0]["lufs"], -20.0, 1e-6)
    # per utterance, the two sentences get two gains; per request, one
    per_utt = scoped(eng, scope=F.LOUDNESS_PER_UTTERANCE).synthesize_batch(texts)
    assert not np.array_equal(np.asarray(per_utt[1]), np.asarray(got[1]))
    # the 16-bit entry is the sink rule of the f64 entry; _each with agreeing engines is the batch entry
    i16 = e.synthesize_batch(texts, i16=True)
    each = J.synthesize_batch_each([e, e.clone()], texts)
    for k in range(2):
        same_bits(np.asarray(i16[k]), np.clip(np.asarray(got[k]), -32768.0, 32767.0).astype(np.int16))
        same_bits(np.asarray(each[k]), np.asarray(got[k]))
    # a single utterance and the generator: a group of one, the bits of the per-utterance scope
    one = scoped(eng, scope=F.LOUDNESS_PER_UTTERANCE).synthesize(SAMPLE_SENTENCE_1)
    same_bits(e.synthesize(SAMPLE_SENTENCE_1), one)
    g = e.generator(SAMPLE_SENTENCE_1)
    buf, parts = np.zeros(g.fperiod()), []
    while True:
        n = g.generate_step(buf)
        if n == 0:
            break
        parts.append(buf[:n].copy())
    same_bits(np.concatenate(parts), one)


def test_engine_each_mismatch_and_multi_refusal(eng):
    texts = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2]
    e = scoped(eng, ceiling=-1.0)
    for other, field in ((scoped(eng, ceiling=-1.0, scope=F.LOUDNESS_PER_UTTERANCE), "loudness_scope"),
                         (scoped(eng, target=-23.0, ceiling=-1.0), "loudness_target"),
                         (scoped(eng, ceiling=-2.0), "peak_ceiling"),
                         (scoped(eng, ceiling=-1.0, peak_mode=F.PEAK_TRUE), "peak_mode"),
                         (scoped(eng, ceiling=-1.0, output_sampling_frequency=16000), "output_sampling_frequency")):
        with pytest.raises(J.JbError, match=field):
            J.synthesize_batch_each([e, other], texts)
    # per utterance, engines may differ in all of these, as before
    a, c = scoped(eng, scope=F.LOUDNESS_PER_UTTERANCE), scoped(eng, target=-28.0, scope=F.LOUDNESS_PER_UTTERANCE)
    out = J.synthesize_batch_each([a, c], texts)
    close_lu(integrated(np.asarray(out[1]), IN)[0], -28.0, 1e-6)
    with pytest.raises(J.JbError, match="one device"):
        e.synthesize_batch(texts, devices=[0, 0])
