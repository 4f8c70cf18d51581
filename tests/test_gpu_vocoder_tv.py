"""The kernels of the frame-to-frame vocoder path against the extended-precision reference (tests/vocoder_tv_ref.py) on the
table of tests/vocoder_tv_cases.py -- never against the oracle, which tests/test_vocoder_tv_ref.py holds to the same
reference on the CPU.  Everything goes through the C ABI as parameter tracks.

Excitation.  Odd tap counts: Batch(..., keep_tracks=True).excitation(i).  Even tap counts and nlpf = 0 are refused above
the vocoder level (SpeechGenerator::new, speech.rs:38-40), so they go through jb_vocoder_synthesize_batch with an order-1
spectrum of zeros: exp(0) = 1 and every filter weight is 0, the PCM IS the excitation.  The split form's shared table
is not built for a batch that keeps the debug tap (alloc_excitation_table: exc_no_table = exc || the flag), so the split
shapes are read as the PCM of a zero spectrum from a batch WITHOUT keep_tracks -- with the table, with no_exc_table=True
-- and once more through the tap.  With constant taps every voiced frame behind a voiced frame carries the batch's first
row and is read from the table; with taps that differ in every frame all go through the per-frame pass.  The gate is that
of tests/test_gpu_coef_ref.py, e_gpu <= 4 e_oracle + 64 u x peak, e_oracle the oracle's distance on the same case
computed here (the factor 4: the split form re-associates the tap sums).  Which family of launch_excite runs is asserted
from the conditions jb_vocoder.hip states (excite_is_split, excite_fits_staged, restated in launch_path) against the
family the shape's name claims, not from the result.

PCM.  Every filter shape with an odd tap count runs through the seven schedules of test_gpu_mlsa_transfer.VARIANTS and
is compared with assert_pcm_close as it stands (PCM_TOL, LOCAL_TOL), both sides scaled by the reference's peak.  MGLSA
takes its rows from the device's own coefficients() / first_coefficients().  The slow shape must report redone chunks
under the redo variant.  The `_table` shape has one row of taps for the whole batch: its schedules (none keeps the debug
tap) take their voiced frames from the shared table.  The beta shapes run again as state-level utterances with per-utterance conditions (voc=), two
betas in one batch, each against the reference of its own beta.  A ragged batch holds a full case, its first frame alone
and an empty utterance."""
import numpy as np
import pytest

import jbonsai_amd as J
from tests import mlsa_ref as R
from tests import test_gpu_mlsa_transfer as M
from tests import vocoder_tv_cases as T
from tests.coef_ref import within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.wide_enough(), reason="numpy.longdouble is no wider than f64 here")]

EXC_FLOOR = 64 * R.U  # of the peak


def frame_blocks(fperiod, nlpf):
    """plan_frame_blocks (jb_plan.cpp): (block size, blocks per frame)."""
    bs = min(64, fperiod)
    while fperiod % bs:
        bs -= 1
    if (bs < nlpf - 1 or bs < 16) and bs < min(64, fperiod):
        nblk = (fperiod + 63) // 64
        bs = (fperiod + nblk - 1) // nblk
    return bs, (fperiod + bs - 1) // bs


def launch_path(fperiod, nlpf):
    """launch_excite (jb_vocoder.hip): excite_is_split, then nlpf == 0, then excite_fits_staged, else k_excite_any."""
    bs, nblk = frame_blocks(fperiod, nlpf)
    if fperiod % 4 == 0 and 32 <= fperiod <= 256 and nlpf in (31, 15) and nblk <= 4 and fperiod % bs == 0:
        return "split"
    if nlpf == 0:
        return "nolpf"
    if fperiod >= 30 and nlpf <= 64 and nlpf - 1 <= fperiod:
        return "staged"
    return "any"


def table_frames(utts):
    """Frames the split form reads from the shared table: voiced behind voiced, both rows equal to the batch's first."""
    first, n = utts[0].lpf[0], 0
    for u in utts:
        ok = u.voiced & np.all(u.lpf == first, axis=1)
        n += int(np.count_nonzero(ok[1:] & ok[:-1]))
    return n


def voice_of(fperiod, nmcp, nlpf, alpha=0.42, volume=1.0, beta=0.0, stage=0, log_gain=False):
    streams = [J.StreamInfo(nmcp, False, False, [[1.0]]), J.StreamInfo(1, True, False, [[1.0]]),
               J.StreamInfo(nlpf, False, False, [[1.0]])]
    return J.VoiceInfo(T.FS, fperiod, alpha, streams, volume=volume, beta=beta, stage=stage, use_log_gain=log_gain)


def shape_voice(shape, beta=None):
    stage, nmcp, alpha, fperiod, volume, _, b, nlpf, log_gain = T.FILTER_SHAPES[shape]
    return voice_of(fperiod, nmcp, nlpf, alpha, volume, b if beta is None else beta, stage, log_gain)


def tracks_of(u, frames=None, spectrum=None):
    n = u.frames if frames is None else frames
    spec = u.spectrum if spectrum is None else spectrum
    return J.TrackUtterance(spec[:n], u.lf0[:n].reshape(n, 1), u.lpf[:n])


def state_utt(u):
    """State level, one frame per state, one-tap windows: the generated tracks are the means."""
    S, v = u.frames, u.voiced
    return J.Utterance(np.ones(S, dtype=np.uint32),
                       [J.StreamStates(u.spectrum, np.ones_like(u.spectrum)),
                        J.StreamStates(np.where(v, u.lf0, 0.0).reshape(S, 1), np.ones((S, 1)), v.astype(np.float64)),
                        J.StreamStates(u.lpf, np.ones_like(u.lpf))])


@pytest.mark.parametrize("shape", list(T.EXC_SHAPES))
def test_excitation_against_the_gather_form(shape):
    fperiod, nlpf, per_frame, _ = T.EXC_SHAPES[shape]
    family = launch_path(fperiod, nlpf)
    assert family == shape.split("_")[0], (shape, family, frame_blocks(fperiod, nlpf))
    utts = T.exc_cases(shape)
    zeros = [np.zeros((u.frames, 2)) for u in utts]
    voice = voice_of(fperiod, 2, nlpf)
    tracks = [tracks_of(u, spectrum=z) for u, z in zip(utts, zeros)]
    in_table = table_frames(utts) if family == "split" else 0
    if family == "split":  # the shape is what it is for
        assert (in_table == 0) if per_frame else (in_table >= 2 * (T.EXC_SHAPES[shape][3] - 1)), in_table
    # keep_tracks allocates the debug tap, and a batch with the tap never builds the shared table (alloc_excitation_table,
    # jb_batch.cpp): the table is reached only by a batch WITHOUT it, whose PCM under a zero spectrum is the excitation
    if family == "split":
        runs = [("table (%d frames)" % in_table if in_table else "general", "pcm", dict()),
                ("without table", "pcm", dict(no_exc_table=True)), ("debug tap, hence without table", "tap", dict())]
    else:
        runs = [("", "tap" if nlpf % 2 else "level", dict())]
    for label, how, kw in runs:
        if how == "level":
            got = J.vocoder_synthesize_batch(voice, tracks)
            via = "vocoder_synthesize_batch, zero spectrum"
        else:
            with J.Batch(voice, tracks, keep_tracks=how == "tap", **kw) as b:
                b.run()
                b.sync()
                got = [b.excitation(i) if how == "tap" else b.pcm(i) for i in range(len(utts))]
            via = "Batch.excitation" if how == "tap" else "Batch.pcm, zero spectrum"
        print("%-22s (%3d, %4d)  bs, nblk %s  family %s%s  via %s" % (shape, fperiod, nlpf, frame_blocks(fperiod, nlpf),
                                                                      family, "/" + label if label else "", via))
        for u, g in zip(utts, got):
            want = T.expected_excitation(shape, u.name.rsplit("-", 1)[1])
            assert g.shape == want.shape and np.isfinite(g).all(), (u.name, label)
            e_gpu, e_oracle = T.exc_err(g, want), T.exc_err(T.oracle_excitation(u), want)
            print("    %-30s e_gpu %.3g  e_oracle %.3g of the peak" % (u.name, e_gpu, e_oracle))
            assert within(e_gpu, e_oracle, EXC_FLOOR), (u.name, label, e_gpu, e_oracle)


_mglsa_reference = {}


def expected_of(shape, utts, coef, first):
    """The reference PCM per utterance.  Stage::Zero: the table's own.  MGLSA: from the device's rows, once per set."""
    if not T.FILTER_SHAPES[shape][0]:
        return T.expected_pcm(shape)
    key = (shape, tuple(u.name for u in utts), b"".join(c.tobytes() for c in coef), b"".join(f.tobytes() for f in first))
    if key not in _mglsa_reference:
        _mglsa_reference[key] = T.reference_pcm(shape, utts, coef, first)
    return _mglsa_reference[key]


def kernel_name(shape, kernel):
    stage = T.FILTER_SHAPES[shape][0]
    return kernel if not stage else "k_vocoder_mglsa<%s>" % (stage if stage <= 8 else "0: delay lines in LDS")


@pytest.mark.parametrize("shape", [s for s, v in T.FILTER_SHAPES.items() if v[7] % 2])
def test_schedules_against_the_time_varying_reference(shape):
    stage = T.FILTER_SHAPES[shape][0]
    utts = T.filter_cases(shape)
    voice, tracks = shape_voice(shape), [tracks_of(u) for u in utts]
    for name, kw in M.VARIANTS:
        with J.Batch(voice, tracks, **kw) as b:
            b.run()
            b.sync()
            kernel, waves = b.kernel_info()
            info = b.info()
            got = [b.pcm(i) for i in range(len(utts))]
            coef = [b.coefficients(i) for i in range(len(utts))] if stage else None
            first = [b.first_coefficients(i) for i in range(len(utts))] if stage else None
        print("%-22s %-15s %-40s waves/SIMD %d  %s" % (shape, name, kernel_name(shape, kernel), waves, info))
        if stage:
            assert all(np.isfinite(c).all() and np.ptp(c, axis=0).min() > 0 for c in coef), (shape, name)  # every row moves
        for u, g, want in zip(utts, got, expected_of(shape, utts, coef, first)):
            M.compare(u, g, want, (u.name, name))
        if name == "redo" and shape.startswith("slow"):
            assert info["n_redo"] > 0, (shape, info)


@pytest.mark.parametrize("shape", [s for s, v in T.FILTER_SHAPES.items() if v[7] % 2 == 0])
def test_vocoder_level_against_the_time_varying_reference(shape):
    """nlpf = 0 through jb_vocoder_synthesize_batch, at PCM level: Excitation::get's branch without a ring buffer in
    front of moving coefficients."""
    utts = T.filter_cases(shape)
    got = J.vocoder_synthesize_batch(shape_voice(shape), [tracks_of(u) for u in utts])
    print("%-22s jb_vocoder_synthesize_batch  excitation family %s" % (shape, launch_path(T.FILTER_SHAPES[shape][3], 0)))
    for u, g, want in zip(utts, got, T.expected_pcm(shape)):
        M.compare(u, g, want, (u.name, "vocoder level"))


@pytest.mark.parametrize("shape", T.BETA_SHAPES)
def test_beta_per_utterance(shape):
    """Two utterances of one batch under different betas (voc=, state-level utterances), each against the reference of
    its own beta; the voice's own beta is 0."""
    _, _, alpha, _, volume, _, beta, _, _ = T.FILTER_SHAPES[shape]
    utts = T.filter_cases(shape)[:2]
    betas = [beta, 0.4 - beta]  # 0.1 and 0.3, either way round
    want = [T.reference_pcm(shape, [u], beta=bt)[0] for u, bt in zip(utts, betas)]
    for kw in (dict(), dict(chunk_frames=8)):
        with J.Batch(shape_voice(shape, 0.0), [state_utt(u) for u in utts], keep_tracks=True,
                     voc=[(alpha, bt, volume) for bt in betas], **kw) as b:
            b.run()
            b.sync()
            got = [b.pcm(i) for i in range(2)]
            trk = [[b.track(i, s) for s in range(3)] for i in range(2)]
            print("%-22s voc= betas %s  %s  %s  %s" % (shape, betas, kw, b.kernel_info(), b.info()))
        for u, g, w, t, bt in zip(utts, got, want, trk, betas):
            assert np.array_equal(t[0], u.spectrum) and np.array_equal(t[1][:, 0], u.lf0) and np.array_equal(t[2], u.lpf), u.name
            M.compare(u, g, w, (u.name, "beta", bt, kw))


@pytest.mark.parametrize("shape", ["z5_a42_f65", "z35_a55_f240", "zb3_n35_a55_f65", "g4_n13_a55_f65"])
def test_ragged_batch_with_one_frame_and_no_frame(shape):
    """A whole utterance, its first frame alone, an empty one and another whole one; the filter is causal, so the one
    frame is the first frame of the whole case's reference (under beta > 0 it already interpolates, from the unfiltered
    row to the filtered one)."""
    stage, fperiod = T.FILTER_SHAPES[shape][0], T.FILTER_SHAPES[shape][3]
    utts = T.filter_cases(shape)
    tracks = [tracks_of(utts[0]), tracks_of(utts[0], frames=1), tracks_of(utts[0], frames=0), tracks_of(utts[1])]
    for kw in (dict(), dict(chunk_frames=8)):
        with J.Batch(shape_voice(shape), tracks, **kw) as b:
            b.run()
            b.sync()
            assert [b.num_samples(i) for i in range(4)] == [utts[0].samples, fperiod, 0, utts[1].samples]
            got = [b.pcm(i) for i in range(4)]
            coef = [b.coefficients(i) for i in (0, 3)] if stage else None
            first = [b.first_coefficients(i) for i in (0, 3)] if stage else None
            if stage:
                assert np.array_equal(b.coefficients(1), coef[0][:1]) and np.array_equal(b.first_coefficients(1), first[0])
            print("%-22s ragged %s  %s  %s" % (shape, kw, kernel_name(shape, b.kernel_info()[0]), b.info()))
        want = expected_of(shape, utts[:2], coef, first)[:2]
        assert got[2].size == 0
        M.compare(utts[0], got[0], want[0], (shape, "whole", kw))
        M.compare(utts[0], got[1], want[0][:fperiod], (shape, "first frame alone", kw))
        M.compare(utts[1], got[3], want[1], (shape, "second", kw))
