"""The fast batch-invariant mode (JB_BATCH_INVARIANT, jb_engine_set_fast_invariant) on the GPU: each case builds one
of the two batches so that a choice the default mode makes from the whole batch flips -- vocoder kernel, warm-up,
redo-round kernel, GV kernel, entry point -- and compares one utterance's output byte for byte; the utterance alone
is also checked against the oracle."""
import dataclasses

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import assert_pcm_close
from tests.test_gpu_configs import oracle_pcm
from tests.test_gpu_stage import lsp_utterance, oracle_stage_pcm, stable_utterance, stage_voice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


def _run(vi, utts, which, **kw):
    """PCM of utts[which] (and the batch's info, kernel, redo counts, GV track) in the invariant mode."""
    with J.Batch(vi, utts, fast_invariant=True, **kw) as b:
        b.run()
        b.sync()
        out = dict(pcm=b.pcm(which), info=b.info(), kernel=b.kernel_info(), fallbacks=b.gang_fallbacks())
        if kw.get("keep_tracks"):
            out["tracks"] = [b.track(which, s) for s in range(3)]
            out["coef"], out["first"] = b.coefficients(which), b.first_coefficients(which)
    return out


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def test_kernel_and_warmup_choice(ctx):
    """Alone, one utterance of 3,000 frames gets the wave / pair kernel and 18 frames of warm-up by default; in a
    batch of 200 distinct utterances (1.2 M frames, thousands of hand-off positions) the lane-triple kernel at two
    waves per SIMD and 14 frames.  Here: the same geometry and the same bits."""
    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 3000, 4101)
    others = [synth.synth_utterance(tab, 6000, 4200 + i) for i in range(200)]
    batch = others[:77] + [u] + others[77:]
    alone = _run(vi, [u], 0)
    inside = _run(vi, batch, 77)
    _same(alone["pcm"], inside["pcm"])
    assert alone["kernel"] == inside["kernel"] == ("k_vocoder_lt", 2)
    assert alone["info"]["warmup_frames"] == inside["info"]["warmup_frames"] == 18
    default = []
    for utts in ([u], batch):  # what the default does with the two
        with J.Batch(vi, utts) as b:
            b.run()
            b.sync()
            default.append((b.kernel_info(), b.info()["warmup_frames"]))
    assert default[0][0][0] == "k_vocoder" and default[0][1] == 18, default
    assert default[1] == (("k_vocoder_lt", 2), 14), default
    want, _ = oracle_pcm(vi, u)
    assert_pcm_close(alone["pcm"], want, 240)


def test_redo_rounds(ctx):
    """A tolerance far below the rounding floor makes most hand-offs fail: few failing chunks alone (the pair kernel
    would redo them by default), many in the batch (the wave kernel).  The redo rounds run one fixed kernel form."""
    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 1500, 4301)
    others = [synth.synth_utterance(tab, 1500, 4400 + i) for i in range(40)]
    tol = 1e-14
    alone = _run(vi, [u], 0, verify_tol=tol)
    inside = _run(vi, others + [u], 40, verify_tol=tol)
    assert 0 < alone["info"]["n_redo"] < inside["info"]["n_redo"]
    assert inside["info"]["n_redo"] > 2 * 256  # more than the CUs: the default would redo on the wave kernel
    _same(alone["pcm"], inside["pcm"])
    want, _ = oracle_pcm(vi, u)
    assert_pcm_close(alone["pcm"], want, 240)


def test_gang_timeout_fallback_gives_the_same_bits(ctx):
    """The resident GV kernel (k_mlpg_gv_gang) against its multi-launch form (k_mlpg_gv_gsweep), which runs after a
    formation timeout: tracks and PCM bitwise equal, on rows of one to seven gang tiles (the default mode's fallback,
    k_mlpg_gv_tp, agrees only to ~1e-12)."""
    eng, tab, vi = ctx
    utts = [synth.synth_utterance(tab, T, 4500 + i) for i, T in enumerate((9000, 1200, 26000, 4000))]
    a = [_run(vi, utts, i, keep_tracks=True) for i in (0, 2)]
    b = [_run(vi, utts, i, keep_tracks=True, test_gang_timeout=True) for i in (0, 2)]
    assert a[0]["fallbacks"] == 0 and b[0]["fallbacks"] == 1
    for x, y in zip(a, b):
        _same(x["pcm"], y["pcm"])
        for tx, ty in zip(x["tracks"], y["tracks"]):
            _same(tx, ty)
    alone = _run(vi, [utts[0]], 0, keep_tracks=True)
    _same(a[0]["pcm"], alone["pcm"])
    for x, y in zip(a[0]["tracks"], alone["tracks"]):
        _same(x, y)
    with J.Batch(vi, utts, keep_tracks=True, test_gang_timeout=True) as d:  # the default's fallback differs
        d.run()
        d.sync()
        assert d.gang_fallbacks() == 1
        assert not np.array_equal(d.track(2, 0), a[1]["tracks"][0])


def test_rows_beside_a_row_longer_than_the_gang(ctx):
    """A row of more than 64 gang tiles (> 249,856 frames) sends the whole batch to the multi-launch form; rows of one
    and of three tiles beside it keep the bits they have alone (where the resident kernel runs)."""
    eng, tab, vi = ctx
    us = [synth.synth_utterance(tab, 900, 4601), synth.synth_utterance(tab, 9500, 4603)]
    long = synth.synth_utterance(tab, 256000, 4602)
    for i, u in enumerate(us):
        alone = _run(vi, [u], 0, keep_tracks=True)
        beside = _run(vi, [long] + us, 1 + i, keep_tracks=True)
        _same(alone["pcm"], beside["pcm"])
        for x, y in zip(alone["tracks"], beside["tracks"]):
            _same(x, y)
        want, _ = oracle_pcm(vi, u)
        assert_pcm_close(alone["pcm"], want, 240)


@pytest.mark.parametrize("kind", ["mglsa", "odd_fperiod", "order63"])
def test_voices_without_the_lane_kernel(ctx, kind):
    eng, tab, vi = ctx
    if kind == "mglsa":  # Stage::NonZero: the MGLSA cascade
        v2 = stage_voice(vi, 2, False)
        u = stable_utterance(tab, vi, v2, 2000, 4701, 2, False, 0.0)
        others = [lsp_utterance(tab, vi, 1000, 4800 + i, False, jit=(0.06, 0.03)) for i in range(60)]
    elif kind == "odd_fperiod":  # the lane-triple kernel walks a frame's samples two at a time
        v2 = dataclasses.replace(vi, fperiod=241)
        u = synth.synth_utterance(tab, 2000, 4701)
        others = [synth.synth_utterance(tab, 1000, 4800 + i) for i in range(60)]
    else:  # nmcp 64: k_vocoder<6> in the wave kernel, the widest lane-kernel form
        v2, u = synth.with_order(vi, synth.synth_utterance(tab, 2000, 4701), 64)
        others = [synth.with_order(vi, synth.synth_utterance(tab, 1000, 4800 + i), 64, seed=20 + i)[1]
                  for i in range(60)]
    alone = _run(v2, [u], 0, keep_tracks=True)
    inside = _run(v2, others[:9] + [u] + others[9:], 9, keep_tracks=True)
    assert alone["kernel"] == inside["kernel"]
    if kind != "order63":
        assert alone["kernel"][0] == "k_vocoder"
    _same(alone["pcm"], inside["pcm"])
    if kind == "mglsa":
        # the filter on the GPU's own coefficients against the oracle's filter loop (the LSP conversion itself is
        # ill-conditioned: tests/test_gpu_stage.py)
        _, tr = oracle_stage_pcm(v2, u, 2, False, 0.0)
        want = O.vocoder(v2.sampling_frequency, v2.fperiod, v2.alpha, 1.0, tr[1][:, 0], tr[0], tr[2], stage=2,
                         use_log_gain=False, coef=alone["coef"], cfirst=alone["first"])
    else:
        want = oracle_pcm(v2, u)[0]
    assert_pcm_close(alone["pcm"], want, v2.fperiod)


def test_engine_level_entries_agree():
    """SAMPLE_SENTENCE_2 through jb_synthesize, jb_synthesize_batch (a batch of 128 k frames), jb_synthesize_batch_each
    beside utterances under other conditions, jb_synthesize_batch_multi on devices [0, 0] and the generator: the same
    bits; the 16-bit sink likewise."""
    e = J.Engine.load([VOICE])
    e.condition.set_fast_invariant(True)
    alone = e.synthesize(SAMPLE_SENTENCE_2)
    ref = O.Voice(VOICE).synthesize(SAMPLE_SENTENCE_2)
    assert alone.shape == ref.shape
    assert_pcm_close(alone, ref, 240)
    big_list = [list(SAMPLE_SENTENCE_2) * 40, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, []] * 4
    big = e.synthesize_batch(big_list)
    small = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
    for got in (big[2], big[14], small[1]):
        _same(got, alone)
    _same(small[0], big[1])
    o1, o2 = e.clone(), e.clone()
    o1.condition.set_alpha(0.5)
    o2.condition.set_volume(-6.0)
    each = J.engine.synthesize_batch_each([o1, e, o2, o1], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2,
                                                           list(SAMPLE_SENTENCE_2) * 20, SAMPLE_SENTENCE_2])
    _same(each[1], alone)
    multi = e.synthesize_batch(big_list[:8], devices=[0, 0])
    _same(multi[2], alone)
    _same(multi[6], alone)
    _same(e.generator(SAMPLE_SENTENCE_2).generate_all(), alone)
    # the 16-bit sink
    a16 = e.synthesize_batch([SAMPLE_SENTENCE_2], i16=True)[0]
    b16 = e.synthesize_batch(big_list, i16=True)
    _same(b16[2], a16)
    _same(b16[14], a16)
    e16 = J.engine.synthesize_batch_each([o1, e, o2], [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2,
                                                      list(SAMPLE_SENTENCE_2) * 20], i16=True)
    _same(e16[1], a16)
