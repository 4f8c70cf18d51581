"""Stage::NonZero (GAMMA != 0 voices -- the spectrum stream holds [gain, LSP...], the
synthesis filter is the MGLSA cascade; vocoder/mod.rs:90-107,142-176) on the GPU against the oracle's
restatement.  PARITY UNPINNED: no reference test reaches this branch and no such voice exists here;
the oracle side is held by the identities of tests/test_oracle_stage.py and, for the coefficient
conversion, by the extended-precision restatement of tests/coef_ref.py (tests/test_coef_ref.py), which
tests/test_gpu_coef_ref.py holds k_stage_coef to as well: both parities of n, every branch of
check_lsp_stability, under 4 x the oracle's own error (1e-15 at small orders, 6e-9 at n = 35).  The
rtol 1e-6 below stays as the end-to-end contract against the oracle."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.helpers import VERIFY_TOL, assert_pcm_close, rel_rms

pytestmark = pytest.mark.gpu
DMAX = 1.7976931348623157e308


@pytest.fixture(scope="module")
def ctx():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


def lsp_utterance(tab, vi, frames, seed, log_gain, jit=(0.2, 0.12)):
    """A synthetic utterance whose spectrum stream holds line spectral pairs: per state a gain and 34
    ordered frequencies (an even grid, jittered), static window only informative (dynamic means 0)."""
    u = synth.synth_utterance(tab, frames, seed)
    rng = np.random.default_rng(seed)
    S = len(u.durations)
    L = vi.streams[0].vector_length
    mean = np.zeros((S, 3 * L))
    var = np.zeros((S, 3 * L))
    h = np.pi / L
    base = h * (np.arange(1, L) + rng.uniform(-jit[0], jit[0], L - 1))
    for s in range(S):
        w = base + h * rng.uniform(-jit[1], jit[1], L - 1)
        # the reference's lsp2lpc takes the gain slot as a frequency too (lsp.rs:27-43): keep it below the
        # first real one, log gain or not, or the filter the reference builds is unstable
        mean[s, 0] = rng.uniform(0.02, 0.08)
        mean[s, 1:L] = np.sort(w)
    var[:, :L] = 1e-4
    var[:, L:] = 1e-3
    sts = list(u.streams)
    sts[0] = J.StreamStates(mean, var, None, None, None, None)
    return J.Utterance(u.durations, sts)


def stage_voice(vi, stage, log_gain, beta=0.0):
    streams = [J.StreamInfo(s.vector_length, s.is_msd, s.use_gv and i != 0, s.windows) for i, s in enumerate(vi.streams)]
    return J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha, streams, beta=beta, stage=stage,
                       use_log_gain=log_gain)


def oracle_stage_pcm(v2, u, stage, log_gain, beta):
    sts = []
    for i, s in enumerate(u.streams):
        si = v2.streams[i]
        msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
        sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                  [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                  s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch,
                                  s.gv_weight, s.msd_threshold))
    tr = [O.mlpg(s, u.durations) for s in sts]
    return O.vocoder(v2.sampling_frequency, v2.fperiod, v2.alpha, 1.0, tr[1][:, 0], tr[0], tr[2], beta=beta,
                     stage=stage, use_log_gain=log_gain), tr


def stable_utterance(tab, vi, v2, frames, seed, stage, log_gain, beta, bound=1e9):
    """Random LSP sets can make the filter the reference builds unstable (the post-filter sharpens the
    resonances; output ~1e240, identical on both sides but useless as a test): take the first seed
    whose reference output stays bounded."""
    for k in range(10):
        u = lsp_utterance(tab, vi, frames, seed + k, log_gain, jit=(0.02, 0.01) if beta > 0 else (0.06, 0.03))
        with np.errstate(all="ignore"):
            ref, _ = oracle_stage_pcm(v2, u, stage, log_gain, beta)
        if np.all(np.isfinite(ref)) and np.abs(ref).max() < bound:
            return u
    raise AssertionError("no stable test utterance found")


@pytest.mark.parametrize("stage,log_gain,beta", [(1, False, 0.0), (2, False, 0.0), (2, True, 0.3), (3, False, 0.2),
                                                 (4, True, 0.0)])
def test_stage_nonzero_vs_oracle(ctx, stage, log_gain, beta):
    """Three levels, because the reference's LSP -> LPC -> generalized-cepstrum conversion is
    ill-conditioned (lsp2lpc multiplies 18 second-order sections whose partial products reach ~1e10 before
    they cancel: one ulp in a cosine moves the coefficients by ~1e-8, tests/test_oracle_stage.py):
      (1) the filter kernel on the GPU's OWN coefficients against the oracle's filter loop on the same
          coefficients: rel RMS <= 1e-9 -- the kernel's arithmetic;
      (2) the coefficient kernel against the oracle's conversion: rtol 1e-6 (device cos / pow vs glibc);
      (3) end to end against the oracle: rel RMS <= 1e-4, north_star's tolerance."""
    eng, tab, vi = ctx
    v2 = stage_voice(vi, stage, log_gain, beta)
    utts = [stable_utterance(tab, vi, v2, T, 900 + 10 * k, stage, log_gain, beta) for k, T in enumerate((60, 400, 1))]
    with J.Batch(v2, utts, keep_tracks=True) as b:
        b.run()
        b.sync()
        got = [b.pcm(i) for i in range(len(utts))]
        coef = [b.coefficients(i) for i in range(len(utts))]
        first = [b.first_coefficients(i) for i in range(len(utts))]
    for i, u in enumerate(utts):
        ref, tr = oracle_stage_pcm(v2, u, stage, log_gain, beta)
        assert len(got[i]) == len(ref) and np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 0
        same = O.vocoder(v2.sampling_frequency, v2.fperiod, v2.alpha, 1.0, tr[1][:, 0], tr[0], tr[2], beta=beta,
                         stage=stage, use_log_gain=log_gain, coef=coef[i], cfirst=first[i])
        e1 = rel_rms(got[i], same)
        want = np.stack([O.stage_coefficients(tr[0][t], v2.alpha, beta, log_gain, stage) for t in range(len(tr[0]))])
        e2 = np.abs(coef[i] - want).max() / np.abs(want).max()
        w0 = O.stage_coefficients(tr[0][0], v2.alpha, beta, log_gain, stage, filtered=False)
        e3 = rel_rms(got[i], ref)
        print("stage", stage, "log gain", log_gain, "beta", beta, "utt", i, "filter on same coefficients", e1,
              "coefficients", e2, "end to end", e3)
        assert_pcm_close(got[i], same, v2.fperiod, what=(stage, log_gain, beta, i))
        assert e2 <= 1e-6 and np.abs(first[i] - w0).max() <= 1e-6 * np.abs(w0).max()
        assert e3 <= 1e-4


def test_stage_nonzero_chunked_serial_and_redo(ctx):
    """The MGLSA kernel rides the chunk / hand-off check / redo machinery: chunked (default), serial
    and a run with a 1-frame warm-up (every hand-off fails and is recomputed) agree."""
    eng, tab, vi = ctx
    v2 = stage_voice(vi, 2, False, 0.0)
    u = stable_utterance(tab, vi, v2, 1500, 950, 2, False, 0.0)
    outs = {}
    for name, kw in (("serial", dict(serial=True)), ("default", dict()),
                     ("redo", dict(chunk_frames=64, warmup_frames=1, verify_tol=VERIFY_TOL))):
        with J.Batch(v2, [u, u], **kw) as b:
            b.run()
            b.sync()
            outs[name] = (b.pcm(0), b.pcm(1), b.info())
    assert outs["redo"][2]["n_redo"] > 10
    for name in ("default", "redo"):
        assert np.array_equal(outs[name][0], outs[name][1])
        assert_pcm_close(outs[name][0], outs["serial"][0], 240, what=name)
    ref, _ = oracle_stage_pcm(v2, u, 2, False, 0.0)
    assert rel_rms(outs["serial"][0], ref) <= 1e-4  # end to end: the conversion's conditioning (above)


@pytest.mark.parametrize("stage,log_gain", [(9, False), (12, True), (70, False), (150, False)])
def test_stage_above_eight_generic_kernel(ctx, stage, log_gain):
    """Stage::NonZero is generic in the number of stages (stage.rs:24-39, mglsa.rs:15-41): above eight the delay
    lines of a chunk live in LDS instead of registers (four, two or one chunk per workgroup by their size).  The
    filter kernel on the GPU's own coefficients against the oracle's loop on the same coefficients, and end to end;
    chunked = serial.  (Every stage of the cascade multiplies the level of these synthetic LSP sets by ~25 -- the same
    on both sides: 1e13 at nine stages, 1e210 at 150; the comparisons are relative.)"""
    eng, tab, vi = ctx
    v2 = stage_voice(vi, stage, log_gain, 0.0)
    utts = [stable_utterance(tab, vi, v2, T, 1300 + 10 * k, stage, log_gain, 0.0, bound=1e280)
            for k, T in enumerate((40, 150, 1))]
    outs = {}
    for name, kw in (("serial", dict(serial=True)), ("chunked", dict(chunk_frames=32))):
        with J.Batch(v2, utts, keep_tracks=True, **kw) as b:
            b.run()
            b.sync()
            outs[name] = [b.pcm(i) for i in range(len(utts))]
            coef = [b.coefficients(i) for i in range(len(utts))]
            first = [b.first_coefficients(i) for i in range(len(utts))]
    for i, u in enumerate(utts):
        ref, tr = oracle_stage_pcm(v2, u, stage, log_gain, 0.0)
        same = O.vocoder(v2.sampling_frequency, v2.fperiod, v2.alpha, 1.0, tr[1][:, 0], tr[0], tr[2], beta=0.0,
                         stage=stage, use_log_gain=log_gain, coef=coef[i], cfirst=first[i])
        assert len(outs["serial"][i]) == len(ref) and np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 0
        sc = 1.0 / np.max(np.abs(ref))  # (squares of 1e210 are not doubles)
        assert_pcm_close(outs["serial"][i] * sc, same * sc, 240)
        assert_pcm_close(outs["chunked"][i] * sc, outs["serial"][i] * sc, 240)
        assert rel_rms(outs["serial"][i] * sc, ref * sc) <= 1e-4


def test_stage_limits(ctx):
    """The delay lines of a chunk's stages share one CU's LDS (64 taps x 8 B per stage): 256 stages at most."""
    eng, tab, vi = ctx
    u = lsp_utterance(tab, vi, 20, 960, False)
    with pytest.raises(J.JbError) as ei:
        J.Batch(stage_voice(vi, 257, False), [u])
    assert ei.value.code == -2
