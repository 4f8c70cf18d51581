"""The PCM gate itself, without a GPU: a whole-utterance relative RMS dilutes an error confined to one frame by
sqrt(1 / frames), so an error the hand-off certification exists to catch can pass it; the per-frame gate of
assert_pcm_close sees it at its own size (tests/helpers.py)."""
import numpy as np
import pytest

from tests.helpers import LOCAL_TOL, PCM_TOL, assert_pcm_close, frame_err, rel_rms

FP = 240


def _signal(n_frames, seed=20261015):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1000.0, n_frames * FP)
    x *= np.repeat(rng.uniform(0.05, 1.0, n_frames), FP)  # louder and quieter frames
    return x


def test_one_bad_frame_passes_rel_rms_and_fails_the_local_gate():
    # rel RMS of an error of size a * RMS in one frame of N is a / sqrt(N): under PCM_TOL once N > (a / PCM_TOL)^2
    a = 2.0 * LOCAL_TOL
    n = int((a / PCM_TOL) ** 2) * 2 + 64
    want = _signal(n)
    rms = np.sqrt(np.mean(want * want))
    bad = n // 3 + 7
    err = np.random.default_rng(5).normal(0.0, 1.0, FP)
    err *= a * rms / np.sqrt(np.mean(err * err))
    got = want.copy()
    got[bad * FP:(bad + 1) * FP] += err
    assert rel_rms(got, want) <= PCM_TOL
    fe, f = frame_err(got, want, FP)
    assert f == bad and fe == pytest.approx(a, rel=1e-6)
    with pytest.raises(AssertionError, match=rf"frame {bad} \(chunk {bad // 153}, offset {bad % 153} of 153\)"):
        assert_pcm_close(got, want, FP, chunk=153)
    with pytest.raises(AssertionError, match=rf"at frame {bad}\b"):
        assert_pcm_close(got, want, FP)


def test_gate_passes_rounding_and_checks_lengths():
    want = _signal(500)
    got = want * (1.0 + 1e-15)
    assert_pcm_close(got, want, FP)
    assert frame_err(want, want, FP) == (0.0, 0)
    with pytest.raises(AssertionError, match="samples against"):
        assert_pcm_close(got[:-1], want, FP)
    # an error spread evenly over the utterance: the same size per frame as over the whole
    got = want + 0.5 * PCM_TOL * np.sqrt(np.mean(want * want)) * np.sign(want)
    fe, _ = frame_err(got, want, FP)
    assert fe == pytest.approx(rel_rms(got, want), rel=1e-9)


def test_short_last_frame_and_silence():
    want = np.zeros(3 * FP + 17)
    got = want.copy()
    got[-1] = 1e-3
    fe, f = frame_err(got, want, FP)  # silent reference: absolute, per frame (the last one has 17 samples)
    assert f == 3 and fe == pytest.approx(1e-3 / np.sqrt(17))
