"""The vocoder kernels against the transfer functions of the filters they run (tests/mlsa_ref.py), on the case table
of tests/mlsa_cases.py -- never against the oracle, which tests/test_mlsa_transfer.py holds to the same reference on
the CPU.  Every shape goes through the C ABI as parameter tracks, one resident batch per schedule:

  default | kernel="wave" | kernel="triple" | serial | fast_invariant | chunk_frames=8 |
  chunk_frames=8 with a one-frame warm-up (hand-offs fail their check and the chunks are redone)

with nlpf = 1 and lpf = [1.0] (SpeechGenerator::new refuses nlpf = 0), and once through jb_vocoder_synthesize_batch
with nlpf = 0, where the noise is drawn on unvoiced samples only.  Each run prints the vocoder kernel it took
(kernel_info: the lane-triple kernel takes even frame periods of Stage::Zero only) and its chunk geometry.

MGLSA: the tracks hold one constant row of line spectral pairs.  The LSP -> coefficient conversion is ill-conditioned
(tests/test_gpu_stage.py), so H is built from the coefficients the device itself converted (coefficients(),
first_coefficients(): equal, and constant over the frames), and both sides are scaled by the reference's peak (the
cascade's level reaches 1e17).

The gate is assert_pcm_close as it stands (PCM_TOL, LOCAL_TOL): the oracle's own distance from this reference, 4e-13 of
the peak at most, is four orders below it."""
import numpy as np
import pytest

import jbonsai_amd as J
from tests import mlsa_cases as C
from tests import mlsa_ref as R
from tests.helpers import VERIFY_TOL, assert_pcm_close

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")]

VARIANTS = [
    ("default", dict()),
    ("wave", dict(kernel="wave")),
    ("triple", dict(kernel="triple")),
    ("serial", dict(serial=True)),
    ("fast_invariant", dict(fast_invariant=True)),
    ("chunk8", dict(chunk_frames=8)),
    ("redo", dict(chunk_frames=8, warmup_frames=1, verify_tol=VERIFY_TOL)),
]
# a response that one frame behind its peak is still above this share of it cannot pass a hand-off check of
# VERIFY_TOL (1e-9) after a one-frame warm-up: such a shape must report redone chunks
MUST_REDO_ABOVE = 1e-6


def voice_of(case, nlpf):
    streams = [J.StreamInfo(case.nmcp, False, False, [[1.0]]), J.StreamInfo(1, True, False, [[1.0]]),
               J.StreamInfo(nlpf, False, False, [[1.0]])]
    return J.VoiceInfo(case.fs, case.fperiod, case.alpha, streams, volume=case.volume, stage=case.stage,
                       use_log_gain=case.log_gain)


def tracks_of(case, nlpf, frames=None):
    T = case.frames if frames is None else frames
    return J.TrackUtterance(case.mc[:T], case.lf0_track()[:T].reshape(T, 1), np.ones((T, nlpf)))


_device_response = {}  # the device's coefficient row (bytes) -> (h, N, margins)


def expected_of(case, nlpf, coef):
    """The reference PCM, read-only.  Stage::Zero: the table's own (computed once per process).  MGLSA: from the
    device's coefficients, one response per distinct row."""
    if not case.stage:
        return C.expected_pcm(case, nlpf)
    key = (case.shape, coef.tobytes())
    if key not in _device_response:
        _device_response[key] = R.case_response(case, coef)
    r = _device_response[key]
    assert r[2]["agree"] <= R.ALIAS_TOL and r[2]["tail"] <= R.ALIAS_TOL, (case.name, r[2])
    return R.expected_pcm(case, nlpf, C.noise(), response=r)


def compare(case, got, want, what):
    want = np.asarray(want, dtype=R.LD)
    peak = np.abs(want).max()
    assert np.isfinite(got).all(), what
    assert_pcm_close(np.asarray(got / peak, dtype=np.float64), np.asarray(want / peak, dtype=np.float64), case.fperiod,
                     what=what)


@pytest.mark.parametrize("shape", C.SHAPES)
def test_schedules_against_transfer_function(shape):
    cases = C.shape_cases(shape)
    voice = voice_of(cases[0], 1)
    utts = [tracks_of(c, 1) for c in cases]
    for name, kw in VARIANTS:
        with J.Batch(voice, utts, **kw) as b:
            b.run()
            b.sync()
            kernel, waves = b.kernel_info()
            info = b.info()
            got = [b.pcm(i) for i in range(len(cases))]
            coef = [None] * len(cases)
            if cases[0].stage:
                coef = [b.coefficients(i) for i in range(len(cases))]
                first = [b.first_coefficients(i) for i in range(len(cases))]
        if cases[0].stage:  # (kernel_info tells the two Stage::Zero families apart; a stage count has one kernel)
            kernel = "k_vocoder_mglsa<%s>" % (cases[0].stage if cases[0].stage <= 8 else "0: delay lines in LDS")
        print("%-22s %-15s %-13s waves/SIMD %d  %s" % (shape, name, kernel, waves, info))
        for i, case in enumerate(cases):
            row = None
            if case.stage:
                assert coef[i].shape == (case.frames, case.nmcp) and np.isfinite(coef[i]).all()
                assert np.array_equal(coef[i], np.tile(first[i], (case.frames, 1))), (case.name, name)
                row = first[i]
            compare(case, got[i], expected_of(case, 1, row), (case.name, name))
        if name == "redo":
            h = C.response(cases[0])[0]
            still = float(np.abs(h[int(np.argmax(np.abs(h))) + cases[0].fperiod:]).max() / np.abs(h).max())
            print("%-22s one frame behind its peak the response is at %.1e of it; n_redo %d" % (shape, still, info["n_redo"]))
            if still > MUST_REDO_ABOVE:
                assert info["n_redo"] > 0, (shape, info)


@pytest.mark.parametrize("shape", list(C.ZERO_SHAPES) + list(C.RAMP_SHAPES))
def test_without_ring_buffer_against_transfer_function(shape):
    """nlpf = 0 through jb_vocoder_synthesize_batch: Excitation::get's branch without a ring buffer."""
    cases = C.shape_cases(shape)
    got = J.vocoder_synthesize_batch(voice_of(cases[0], 0), [tracks_of(c, 0) for c in cases])
    for case, g in zip(cases, got):
        compare(case, g, expected_of(case, 0, None), (case.name, "nlpf 0"))


@pytest.mark.parametrize("shape", ["n5_a42_f65", "n35_a55_f240", "n64_a0_f37"])
def test_ragged_batch_with_one_frame_and_no_frame(shape):
    """One batch of a whole utterance, a one-frame one and an empty one; the filter is causal, so the one frame is the
    first frame of the whole case's reference."""
    pulses, noise = C.build_case(shape, "pulses"), C.build_case(shape, "noise")
    utts = [tracks_of(pulses, 1), tracks_of(noise, 1, frames=1), tracks_of(pulses, 1, frames=0), tracks_of(pulses, 1, frames=1),
            tracks_of(noise, 1)]
    want = [C.expected_pcm(pulses, 1), C.expected_pcm(noise, 1)[:noise.fperiod], None,
            C.expected_pcm(pulses, 1)[:pulses.fperiod], C.expected_pcm(noise, 1)]
    for kw in (dict(), dict(chunk_frames=8)):
        with J.Batch(voice_of(pulses, 1), utts, **kw) as b:
            b.run()
            b.sync()
            assert [b.num_samples(i) for i in range(5)] == [pulses.samples, noise.fperiod, 0, pulses.fperiod, noise.samples]
            got = [b.pcm(i) for i in range(5)]
        for i, w in enumerate(want):
            if w is None:
                assert got[i].size == 0
            else:
                compare(pulses, got[i], w, (shape, i, kw))
