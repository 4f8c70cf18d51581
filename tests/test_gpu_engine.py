"""Engine-level drop-in tests on the GPU, written after the reference's own
end-to-end tests (src/lib.rs:38-160): same labels, same golden samples, at the
reference's own gate of abs 1e-10 in f64.  The HIP path re-associates sums (DPP
scans, FMAs) and chunks the vocoder; measured on the MI355X, 2026-10-15, max |delta|
over the golden samples: 5.2e-11 on the default path, 5.5e-11 on the serial
recursion (test_goldens_at_the_reference_epsilon)."""
import numpy as np
import pytest

import jbonsai_amd as J
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import assert_pcm_close, rel_rms

pytestmark = pytest.mark.gpu
EPS = 1e-10  # src/lib.rs:45-46


@pytest.fixture(scope="module")
def engine():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def test_bonsai(engine):
    speech = engine.synthesize(SAMPLE_SENTENCE_1)
    assert len(speech) == 66480
    assert abs(speech[2000] - 19.35141137623778) < EPS
    assert abs(speech[30000] - -980.6757547598129) < EPS


def test_bonsai_load_from_bytes():
    e = J.Engine.load_from_bytes([VOICE.read_bytes()])
    speech = e.synthesize(SAMPLE_SENTENCE_1)
    assert len(speech) == 66480
    assert abs(speech[30000] - -980.6757547598129) < EPS


def test_is_this_bonsai(engine):
    speech = engine.synthesize(SAMPLE_SENTENCE_2)
    assert len(speech) == 100800
    assert abs(speech[2000] - 17.15977345625943) < EPS
    assert abs(speech[30000] - 2566.2058730889985) < EPS
    assert abs(speech[70000] - -1898.2890228814217) < EPS
    assert abs(speech[100799] - -13.514971382534956) < EPS


def test_is_this_bonsai_fast():
    e = J.Engine.load([VOICE])
    e.condition.set_speed(1.4)
    speech = e.synthesize(SAMPLE_SENTENCE_2)
    assert len(speech) == 72000
    assert abs(speech[2000] - 15.0481014871396) < EPS
    assert abs(speech[30000] - -56.77163803227678) < EPS
    assert abs(speech[70000] - -9.15409432584658) < EPS
    assert abs(speech[71199] - 7.840225089163972) < EPS


# the golden samples of the reference's end-to-end tests (src/lib.rs:38-75): (labels, speed, {index: value})
GOLDENS = [(SAMPLE_SENTENCE_1, 1.0, {2000: 19.35141137623778, 30000: -980.6757547598129}),
           (SAMPLE_SENTENCE_2, 1.0, {2000: 17.15977345625943, 30000: 2566.2058730889985, 70000: -1898.2890228814217,
                                     100799: -13.514971382534956}),
           (SAMPLE_SENTENCE_2, 1.4, {2000: 15.0481014871396, 30000: -56.77163803227678, 70000: -9.15409432584658,
                                     71199: 7.840225089163972})]


def _golden_err(e):
    worst = 0.0
    for labels, speed, want in GOLDENS:
        e.condition.set_speed(speed)
        speech = e.synthesize(labels)
        worst = max([worst] + [abs(speech[i] - v) for i, v in want.items()])
    return worst


def test_goldens_at_the_reference_epsilon():
    """The serial recursion (set_batch_invariant: one item per utterance, no chunk hand-offs) meets the reference's
    epsilon on every golden sample, and so does the default path."""
    e = J.Engine.load([VOICE])
    e.condition.set_batch_invariant(True)
    serial = _golden_err(e)
    default = _golden_err(J.Engine.load([VOICE]))
    print(f"golden samples, max |delta|: serial {serial:.3e}, default {default:.3e}")
    assert serial < EPS, serial
    assert default < EPS, default


def test_bonsai_multi():
    """src/lib.rs:77-91 through the GPU engine: two DIFFERENT voices blended on the device (k_gather_blend).
    Skipped until the tohoku-f01 files are supplied (tests/conftest.py: JB_TOHOKU_DIR)."""
    from tests.conftest import BONSAI_MULTI_GOLDEN, BONSAI_MULTI_WEIGHTS, tohoku_voices

    e = J.Engine.load(tohoku_voices())
    e.condition.set_interpolation_duration(BONSAI_MULTI_WEIGHTS["duration"])
    for i, w in enumerate(BONSAI_MULTI_WEIGHTS["parameter"]):
        e.condition.set_interpolation_parameter(i, w)
    speech = e.synthesize(SAMPLE_SENTENCE_1)
    assert len(speech) == BONSAI_MULTI_GOLDEN["len"]
    assert abs(speech[2000] - BONSAI_MULTI_GOLDEN[2000]) < EPS
    assert abs(speech[30000] - BONSAI_MULTI_GOLDEN[30000]) < EPS


def test_empty():
    e = J.Engine.load([VOICE])
    assert len(e.synthesize([])) == 0
    e.condition.set_speed(1.2)
    assert len(e.synthesize([])) == 0


def test_generator_streaming_equals_synthesize(engine):
    """SpeechGenerator::generate_step: frame-granular steps with persistent filter /
    excitation state reproduce generate_all (src/speech.rs:65-96)."""
    whole = engine.synthesize(SAMPLE_SENTENCE_1)
    g = engine.generator(SAMPLE_SENTENCE_1)
    fp = g.fperiod()
    assert fp == 240 and g.synthesized_frames() == 0 and g.total_frames() == 277
    buf = np.zeros(fp)
    out = []
    for k in range(10):
        assert g.generate_step(buf) == fp
        out.append(buf.copy())
    assert g.synthesized_frames() == 10
    rest = g.generate_all()
    assert g.generate_step(buf) == 0
    got = np.concatenate(out + [rest])
    assert len(got) == len(whole)
    # the first steps may come from the serial recursion while the utterance is still in flight, the rest
    # from the time-chunked run: equal to the hand-off tolerance (1e-9 of the filter state, certified)
    assert rel_rms(got, whole) < 1e-10
    with pytest.raises(J.JbError) as ei:
        engine.generator(SAMPLE_SENTENCE_1).generate_step(np.zeros(10))
    assert ei.value.code == -8


def test_generator_steps_n_and_generators_in_flight(engine):
    """jb_generator_step_n: up to n generate_step calls in one (one D2H copy), mixed with single steps;
    several generators made back to back and drained in turn; the same audio as Engine::synthesize."""
    whole = engine.synthesize(SAMPLE_SENTENCE_2)
    g = engine.generator(SAMPLE_SENTENCE_2)
    fp, T = g.fperiod(), g.total_frames()
    assert T * fp == len(whole) == 100800
    buf = np.zeros(8 * fp)
    parts = []
    assert g.generate_steps(buf, 0) == 0
    assert g.generate_steps(buf, 3) == 3 * fp and g.synthesized_frames() == 3
    parts.append(buf[:3 * fp].copy())
    assert g.generate_step(buf) == fp
    parts.append(buf[:fp].copy())
    while True:
        r = g.generate_steps(buf, 100)  # bounded by the buffer: 8 frames
        if r == 0:
            break
        assert r == min(8, T - (g.synthesized_frames() - r // fp)) * fp
        parts.append(buf[:r].copy())
    assert g.synthesized_frames() == T and g.generate_step(buf) == 0
    got = np.concatenate(parts)
    assert len(got) == len(whole) and rel_rms(got, whole) < 1e-12
    with pytest.raises(J.JbError) as ei:
        engine.generator(SAMPLE_SENTENCE_1).generate_steps(np.zeros(10), 4)
    assert ei.value.code == -8
    labs = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2] * 4
    gens = [engine.generator(l) for l in labs]
    ref = [engine.synthesize(SAMPLE_SENTENCE_1), whole]
    for i, gg in enumerate(gens):
        assert rel_rms(gg.generate_all(), ref[i % 2]) < 1e-12
    assert len(engine.generator([]).generate_all()) == 0


def test_synthesize_batch(engine):
    outs = engine.synthesize_batch([SAMPLE_SENTENCE_1, [], SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1])
    assert [len(o) for o in outs] == [66480, 0, 100800, 66480]
    assert np.array_equal(outs[0], outs[3])
    assert abs(outs[2][70000] - -1898.2890228814217) < EPS


def test_synthesize_batch_threaded_front_half(engine):
    """The host front half runs on worker threads, one utterance each: results must not depend
    on the thread count, and an error in one utterance (here: a malformed label, LabelError in the
    reference) must surface with its message."""
    import os
    batch = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2] * 12 + [[]]
    ref = engine.synthesize_batch(batch[:2])
    first = None
    for nt in ("1", "5"):
        os.environ["JB_HOST_THREADS"] = nt
        try:
            outs = engine.synthesize_batch(batch)
        finally:
            del os.environ["JB_HOST_THREADS"]
        assert len(outs) == 25 and len(outs[24]) == 0
        for i in range(24):
            # bitwise among the copies and across thread counts; against the two-utterance batch only to
            # the hand-off tolerance (the vocoder's chunk length follows the batch's total length)
            assert np.array_equal(outs[i], outs[i % 2])
            assert rel_rms(outs[i], ref[i % 2]) <= 1e-10
        if first is None:
            first = outs
        else:
            assert all(np.array_equal(a, b) for a, b in zip(outs, first))
    bad = list(SAMPLE_SENTENCE_1)
    bad[3] = "not a full-context label"
    with pytest.raises(J.JbError) as ei:
        engine.synthesize_batch([SAMPLE_SENTENCE_1] * 7 + [bad] + [SAMPLE_SENTENCE_2] * 3)
    assert "LABEL" in str(ei.value).upper() or "label" in str(ei.value)


def test_device_gather_blend_equals_host_blend():
    """jb_synthesize_batch hands pdf ROW INDICES to the device, where the gather and
    the multi-voice blend (voice_set.rs:80-95) run; JB_HOST_BLEND=1 selects the host blend.  Both
    must produce the same bits -- one voice, and two voices (the nitech voice loaded twice) with
    unequal interpolation weights, a half-tone shift and a speed change."""
    import os

    def both(e, batch):
        outs = []
        for hb in ("0", "1"):
            os.environ["JB_HOST_BLEND"] = hb
            try:
                outs.append(e.synthesize_batch(batch))
            finally:
                del os.environ["JB_HOST_BLEND"]
        return outs

    batch = [SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, [], SAMPLE_SENTENCE_1]
    e1 = J.Engine.load([VOICE])
    a, b = both(e1, batch)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert abs(a[0][2000] - 19.35141137623778) < EPS  # src/lib.rs:44-46 through the device gather
    e2 = J.Engine.load([VOICE, VOICE])
    e2.condition.set_interpolation_parameter(0, [0.3, 0.7])
    e2.condition.set_interpolation_parameter(1, [0.8, 0.2])
    e2.condition.set_interpolation_duration([0.5, 0.5])
    e2.condition.set_additional_half_tone(2.5)
    e2.condition.set_speed(1.2)
    a, b = both(e2, batch)
    for x, y in zip(a, b):
        assert len(x) == len(y) and np.array_equal(x, y)
    assert len(a[0]) > 0 and len(a[2]) == 0


def test_concurrent_synthesize_on_one_engine(engine):
    """Engine::synthesize takes &self and the reference Engine is Sync: several host threads may
    synthesise through one engine at once (each call owns its batch and streams; the noise table
    and the device pdf tables are shared behind locks)."""
    import threading

    ref = {0: engine.synthesize(SAMPLE_SENTENCE_1), 1: engine.synthesize(SAMPLE_SENTENCE_2)}
    out, errs = {}, []

    def work(i):
        try:
            for k in range(3):
                out[(i, k)] = (engine.synthesize_batch([SAMPLE_SENTENCE_2, SAMPLE_SENTENCE_1])
                               if (i + k) % 2 else [engine.synthesize(SAMPLE_SENTENCE_2), engine.synthesize(SAMPLE_SENTENCE_1)])
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert len(out) == 12
    for v in out.values():
        assert np.array_equal(v[0], ref[1]) and np.array_equal(v[1], ref[0])


def test_volume_db(engine):
    e = J.Engine.load([VOICE])
    base = e.synthesize(SAMPLE_SENTENCE_1)
    e.condition.set_volume(-6.0)
    quiet = e.synthesize(SAMPLE_SENTENCE_1)
    np.testing.assert_allclose(quiet, base * np.exp(-6.0 * 0.11512925464970228), rtol=1e-12, atol=1e-12)


def test_engine_beta_postfilter(oracle_voice):
    """Engine::synthesize with Condition::set_beta (engine.rs:215-218 -> cepstrum.rs:23-37).
    The reference has no golden for beta > 0: the oracle for this case is unpinned."""
    e = J.Engine.load([VOICE])
    e.condition.set_beta(0.3)
    got = e.synthesize(SAMPLE_SENTENCE_1)
    want = oracle_voice.synthesize(SAMPLE_SENTENCE_1, beta=0.3)
    assert len(got) == len(want) == 66480
    assert_pcm_close(got, want, 240)


def test_synthesize_batch_i16_and_staged_readback(engine):
    """jb_synthesize_batch_i16 = the f64 result through the reference callers' sink
    (value.min(i16::MAX).max(i16::MIN) as i16, examples/is-bonsai/main.rs:44-48), and both entries
    bring the slab back through the pinned staging ring: utterances of different lengths, more
    than one 16 MB slot in total, buffers owned by the library until the arrays die."""
    long = list(SAMPLE_SENTENCE_2) * 24  # ~50 s -> 19 MB of f64 per utterance
    utts = [SAMPLE_SENTENCE_1, long, [], SAMPLE_SENTENCE_2, long, SAMPLE_SENTENCE_1]
    f64 = engine.synthesize_batch(utts)
    i16 = engine.synthesize_batch(utts, i16=True)
    assert sum(x.nbytes for x in f64) > 2 * (16 << 20)
    assert [len(x) for x in f64] == [len(x) for x in i16] and len(f64[2]) == 0
    for a, b in zip(f64, i16):
        assert b.dtype == np.int16
        assert np.array_equal(np.clip(a, -32768.0, 32767.0).astype(np.int16), b)
    # same utterance twice in the batch, and against the single-utterance entry
    assert np.array_equal(f64[0], f64[5]) and np.array_equal(f64[1], f64[4])
    # (not bitwise: the chunk length of the time-chunked vocoder follows the batch's total length, and
    # hand-offs are certified to 1e-9 of the filter state, not to the last bit)
    assert rel_rms(f64[3], engine.synthesize(SAMPLE_SENTENCE_2)) <= 1e-10


def test_generator_with_postfilter_equals_synthesize():
    """Streaming generate_step with Condition::set_beta: the first step starts from the un-filtered
    coefficients like generate_all does (vocoder/mod.rs:80-89,116-118)."""
    e = J.Engine.load([VOICE])
    e.condition.set_beta(0.4)
    whole = e.synthesize(SAMPLE_SENTENCE_2)
    g = e.generator(SAMPLE_SENTENCE_2)
    fp = g.fperiod()
    buf = np.zeros(fp)
    out = []
    for _ in range(3):
        assert g.generate_step(buf) == fp
        out.append(buf.copy())
    got = np.concatenate(out + [g.generate_all()])
    assert len(got) == len(whole) == 100800
    # the generator is the serial recursion, synthesize() runs time-chunked: equal to the hand-off
    # tolerance (1e-9 of the filter state, certified), not to rounding
    assert rel_rms(got, whole) < 1e-10


def test_synthesize_batch_in_groups_equals_one_batch(engine, monkeypatch):
    """jb_synthesize_batch's grouped pipeline (front half of group g+1 and read-back of group g-1
    beside the GPU work of group g): same lengths, same audio as the one-batch path, empty
    utterances and group boundaries included."""
    long = list(SAMPLE_SENTENCE_2) * 6
    utts = [SAMPLE_SENTENCE_1, long, [], SAMPLE_SENTENCE_2, long, SAMPLE_SENTENCE_1, [], long, SAMPLE_SENTENCE_2]
    monkeypatch.setenv("JB_SYNTH_GROUPS", "1")
    one = engine.synthesize_batch(utts)
    for g in ("2", "3", "9"):
        monkeypatch.setenv("JB_SYNTH_GROUPS", g)
        got = engine.synthesize_batch(utts)
        assert [len(x) for x in got] == [len(x) for x in one]
        for a, b in zip(got, one):
            if len(a):
                assert rel_rms(a, b) <= 1e-10
    monkeypatch.setenv("JB_SYNTH_GROUPS", "3")
    i16 = engine.synthesize_batch(utts, i16=True)
    for a, b in zip(i16, one):
        assert np.array_equal(a, np.clip(b, -32768.0, 32767.0).astype(np.int16)) or \
            np.max(np.abs(a.astype(np.float64) - np.clip(b, -32768.0, 32767.0))) <= 1.0


def test_batch_invariant_option_gives_the_same_bits_alone_and_in_any_batch():
    """By default an utterance's audio depends (to ~1e-10) on what else is in its batch: the chunk length of
    the time-chunked vocoder follows the batch's total length.  jb_engine_set_batch_invariant (JB_BATCH_SERIAL
    for every batch of the engine) makes it the same bits alone, in a small and in a larger batch, and through
    the streaming generator."""
    e = J.Engine.load([VOICE])
    assert not e.condition.get_batch_invariant()
    e.condition.set_batch_invariant(True)
    assert e.condition.get_batch_invariant()
    alone = e.synthesize(SAMPLE_SENTENCE_2)
    assert abs(alone[30000] - 2566.2058730889985) < EPS  # src/lib.rs:130
    small = e.synthesize_batch([SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2])
    big = e.synthesize_batch([list(SAMPLE_SENTENCE_2) * 30, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2, []] * 3)
    assert np.array_equal(small[1], alone) and np.array_equal(big[2], alone) and np.array_equal(big[10], alone)
    assert np.array_equal(small[0], big[1])
    assert np.array_equal(e.generator(SAMPLE_SENTENCE_2).generate_all(), alone)
    k = e.clone()
    assert k.condition.get_batch_invariant()


def test_examples_run(tmp_path):
    """examples/is_bonsai.py and examples/genji.py (the reference's two examples) run end to end and write
    16-bit mono WAV files of the expected lengths."""
    import subprocess
    import sys
    import wave
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    for script, n_expected in (("is_bonsai.py", 100800), ("genji.py", None)):
        out = tmp_path / (script + ".wav")
        args = [sys.executable, str(root / "examples" / script)] + ([str(VOICE)] if script == "is_bonsai.py" else []) + [str(out)]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        with wave.open(str(out), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48000)
            assert w.getnframes() % 240 == 0 and w.getnframes() > 0
            if n_expected:
                assert w.getnframes() == n_expected
        assert "samples in total" in r.stdout
