"""BASELINE.json configs at (or near) their full sizes, and the ragged / degenerate
inputs the domain has: empty, single-frame, all-unvoiced, all-voiced, zero-duration
states, mixed lengths, two-voice interpolation.  Full-size checks use the oracle
where it finishes in seconds and size-independent properties elsewhere."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from oracle import oracle as O
from tests.conftest import VOICE
from tests.golden.labels import SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2
from tests.helpers import assert_pcm_close, oracle_states, rel_rms, to_utt, voice_info

pytestmark = pytest.mark.gpu
DMAX = 1.7976931348623157e308


@pytest.fixture(scope="module")
def ctx():
    assert J.lib().jb_device_count() > 0
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


def oracle_pcm(vi, u, volume=1.0):
    sts = []
    for i, s in enumerate(u.streams):
        si = vi.streams[i]
        msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
        sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                  [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                  s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch,
                                  s.gv_weight, s.msd_threshold))
    tr = [O.mlpg(s, u.durations) for s in sts]
    return O.vocoder(vi.sampling_frequency, vi.fperiod, vi.alpha, volume, tr[1][:, 0], tr[0], tr[2]), tr


def run(vi, utts, **kw):
    with J.Batch(vi, utts, **kw) as b:
        b.run()
        b.sync()
        return [b.pcm(i) for i in range(len(utts))], b.info()


def test_config2_full_length_utterance_vs_oracle(ctx):
    """BASELINE config 2's utterance at its full length (25,546 frames, 6,131,040
    samples): HIP (chunked, default) vs the oracle, plus copies are bitwise equal."""
    eng, tab, vi = ctx
    u = synth.u128(tab, 0)
    assert int(u.durations.sum()) == synth.T_128S
    got, info = run(vi, [u, u, u])
    assert len(got[0]) == 6131040 and info["chunk_frames"] > 0
    ref, _ = oracle_pcm(vi, u)
    e = rel_rms(got[0], ref)
    print("config 2 full length: rel RMS vs oracle", e, "chunks redone", info["n_redo"])
    assert_pcm_close(got[0], ref, 240, chunk=info["chunk_frames"])
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_config2_throughput_kernel_at_scale(ctx):
    """Config 2 at a quarter of its batch (64 x 25,546 frames = 1.6 M frames): enough for the
    lane-triple throughput kernel at two waves per SIMD, the 2048-frame GV tiles and the
    LDS-staged band solve to run as they do in bench.py.  Every hand-off is certified or redone,
    copies are bit-identical (each ran in a different lane triple / wave / CU), the first
    and last copy match the oracle, and the fused i16 sink equals clamp(f64)."""
    eng, tab, vi = ctx
    u = synth.u128(tab, 0)
    n = 64
    with J.Batch(vi, [u] * n) as b:
        b.run()
        b.sync()
        info = b.info()
        picks = [b.pcm(i) for i in (0, 1, 31, n - 1)]
    # (40-frame chunks at this size: a few hand-off positions of this utterance fail the check and are
    # redone from their predecessor's end state -- identically in every copy)
    assert info["n_items"] >= 8192 and info["n_redo"] % n == 0, info
    for p_ in picks[1:]:
        assert np.array_equal(picks[0], p_)
    ref, _ = oracle_pcm(vi, u)
    e = rel_rms(picks[0], ref)
    print("config 2 x64: rel RMS vs oracle", e, info)
    assert_pcm_close(picks[0], ref, 240, chunk=info["chunk_frames"])
    with J.Batch(vi, [u] * n, pcm_i16=True) as b:
        b.run()
        b.sync()
        q = b.pcm_i16(n - 1)
    assert np.array_equal(q, np.clip(picks[0], -32768.0, 32767.0).astype(np.int16))


def test_config3_mixed_lengths(ctx):
    """Mixed-length batch (config 3 shape, reduced count): every utterance checked
    against the oracle; lengths ragged; launch order must not leak between utterances."""
    eng, tab, vi = ctx
    lens = [1, 2, 31, 33, 159, 161, 400, 1000, 2777, 5000]
    utts = [synth.synth_utterance(tab, T, 100 + i) for i, T in enumerate(lens)]
    got, info = run(vi, utts)
    for u, g, T in zip(utts, got, lens):
        assert len(g) == T * 240
        ref, _ = oracle_pcm(vi, u)
        assert_pcm_close(g, ref, 240, what=T)


def test_gv_rows_of_short_utterances_share_a_gang_pass(ctx):
    """Resident GV (jb_gv_gang.hip): the rows of several short utterances are packed into one pass of a gang (bins by
    first fit in launch order).  A ragged batch whose longest utterance needs three tiles: every MCP track must be
    the one the same utterance gets in a batch of its own -- bit for bit, the sums have a fixed shape per row --
    and match the oracle's (mlpg.rs:145-292) to the MCP gate."""
    eng, tab, vi = ctx
    lens = [9000, 700, 4100, 3000, 2500, 1, 3905, 800, 5200, 60]
    utts = [synth.synth_utterance(tab, T, 300 + i) for i, T in enumerate(lens)]
    with J.Batch(vi, utts, keep_tracks=True) as b:
        b.run()
        b.sync()
        together = [b.track(i, 0) for i in range(len(utts))]
    for i in (0, 2, 3, 6, 8, 9):
        with J.Batch(vi, [utts[i]], keep_tracks=True) as b:
            b.run()
            b.sync()
            alone = b.track(0, 0)
        assert np.array_equal(together[i], alone), lens[i]
        _, tr = oracle_pcm(vi, utts[i])
        scale = np.abs(tr[0]).max(axis=0)
        assert (np.abs(together[i] - tr[0]).max(axis=0) <= 1e-12 * scale + 1e-13).all(), lens[i]


def test_config5_two_voice_interpolation_states(ctx):
    """Config 5 shape: two-voice blend (alpha = 0.5).  The blend is pre-boundary in the
    reference (voice_set.rs:80-95), done by the host front half; the blended states go
    through the GPU and are checked against the oracle on the same arrays.  The second
    'voice' is the nitech file again (tohoku-f01 is absent), with different labels'
    states standing in for a different voice's leaves."""
    e2 = J.Engine.load([VOICE, VOICE])
    for w in (0, 1, 2):
        e2.condition.set_interpolation_parameter(w, [0.5, 0.5])
    e2.condition.set_interpolation_duration([0.5, 0.5])
    u = e2.states(SAMPLE_SENTENCE_2)
    vi = e2.voice_info()
    got, _ = run(vi, [u])
    ref, _ = oracle_pcm(vi, u)
    assert_pcm_close(got[0], ref, 240)
    # a real blend of two different state sequences (same durations), alpha = 0.5
    e1 = J.Engine.load([VOICE])
    a, b = e1.states(SAMPLE_SENTENCE_1), e1.states(SAMPLE_SENTENCE_1[:4] + SAMPLE_SENTENCE_1[:4])
    assert len(a.durations) == len(b.durations)
    mix = J.Utterance(a.durations, [
        J.StreamStates(0.5 * sa.mean + 0.5 * sb.mean, 0.5 * sa.var + 0.5 * sb.var,
                       None if sa.msd is None else 0.5 * sa.msd + 0.5 * sb.msd,
                       sa.gv_mean, sa.gv_var, sa.gv_switch) for sa, sb in zip(a.streams, b.streams)])
    got, _ = run(vi, [mix])
    ref, _ = oracle_pcm(vi, mix)
    assert_pcm_close(got[0], ref, 240)


def _flat(vi, S, dur, voiced, gv_on=True):
    """Near-constant utterance (a small per-state ramp keeps the GV variance non-zero:
    conv_gv divides by it unguarded, src/mlpg_adjust/mlpg.rs:196-197)."""
    sts = []
    ramp = np.linspace(0.0, 0.3, S)
    for i, si in enumerate(vi.streams):
        WL = si.vector_length * len(si.windows)
        mean = np.zeros((S, WL))
        var = np.full((S, WL), 0.01)
        if i == 0:
            mean[:, 0] = 3.0 + ramp
            mean[:, 1] = 0.5 - ramp
            mean[:, 2:si.vector_length] = 0.01 * np.sin(np.arange(S))[:, None]
        if i == 1:
            mean[:, 0] = 5.0 + ramp
        if i == 2:
            mean[:, :] = 0.0
            mean[:, si.vector_length // 2] = 1.0
        msd = np.full(S, 0.9 if voiced else 0.1) if si.is_msd else None
        gm = gv = gs = None
        if si.use_gv:
            gm, gv, gs = np.full(si.vector_length, 0.02), np.full(si.vector_length, 1e-4), np.full(S, 1 if gv_on else 0, np.uint8)
        sts.append(J.StreamStates(mean, var, msd, gm, gv, gs))
    return J.Utterance(np.asarray(dur, np.uint32), sts)


@pytest.mark.parametrize("voiced", [True, False])
def test_degenerate_voicing(ctx, voiced):
    eng, tab, vi = ctx
    u = _flat(vi, 12, [7] * 12, voiced)
    got, _ = run(vi, [u])
    ref, tr = oracle_pcm(vi, u)
    assert (tr[1] == O.NODATA).all() == (not voiced)
    assert_pcm_close(got[0], ref, 240)


def test_zero_duration_states_and_single_frame(ctx):
    eng, tab, vi = ctx
    base = synth.synth_utterance(tab, 300, 5)
    d = base.durations.copy()
    d[3] = 0
    d[10] = 0
    d[-1] = 0
    u0 = J.Utterance(d, base.streams)
    # one-frame utterances: GV switched off (a single frame has zero variance; the
    # reference would divide by it), as for the silence phones of real labels
    u1 = _flat(vi, 1, [1], True, gv_on=False)
    u2 = _flat(vi, 3, [0, 1, 0], False, gv_on=False)
    got, _ = run(vi, [u0, u1, u2])
    for u, g in zip((u0, u1, u2), got):
        ref, _ = oracle_pcm(vi, u)
        assert len(g) == len(ref)
        assert_pcm_close(g, ref, 240)


def test_linearity_in_volume_and_idempotence(ctx):
    """Size-independent properties on a long utterance: PCM scales exactly with volume
    (one final multiply, vocoder/mod.rs:136) and re-running a batch is bitwise stable."""
    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 6000, 9)
    with J.Batch(vi, [u]) as b:
        b.run(); b.sync()
        p1 = b.pcm(0)
        b.run(); b.sync()
        p2 = b.pcm(0)
    assert np.array_equal(p1, p2)
    vi2 = J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha, vi.streams, volume=0.25)
    q, _ = run(vi2, [u])
    assert np.array_equal(q[0], p1 * 0.25)


@pytest.mark.parametrize("L2", [25, 50])
def test_other_spectral_orders(ctx, L2):
    """Voices with another mel-cepstral order (the reference is generic in it): the MCP stream of
    a synthetic utterance is cut to 25 dims (the lane-triple kernel's second specialisation) or
    widened to 50 (LDS-staged solve with LMAX=64, 5 taps per lane in the wave kernel, [dim][frame]
    build at L=50) by dropping / appending small-variance dimensions per window.  HIP vs oracle."""
    import dataclasses

    eng, tab, vi = ctx
    rng = np.random.default_rng(7)
    T = 700
    u = synth.synth_utterance(tab, T, 3)
    L = vi.streams[0].vector_length
    W = len(vi.streams[0].windows)
    m0 = u.streams[0]
    S = len(u.durations)

    def reshape(a, fill):
        a = a.reshape(S, W, L)
        if L2 <= L:
            return a[:, :, :L2].reshape(S, W * L2).copy()
        extra = fill((S, W, L2 - L))
        return np.concatenate([a, extra], axis=2).reshape(S, W * L2)

    mean = reshape(m0.mean, lambda sh: 0.02 * rng.standard_normal(sh))
    var = reshape(m0.var, lambda sh: 0.01 + 0.01 * rng.random(sh))
    gvm = m0.gv_mean[:L2] if L2 <= L else np.concatenate([m0.gv_mean, np.full(L2 - L, 4e-4)])
    gvv = m0.gv_var[:L2] if L2 <= L else np.concatenate([m0.gv_var, np.full(L2 - L, 1e-8)])
    s0 = dataclasses.replace(m0, mean=mean, var=var, gv_mean=gvm, gv_var=gvv)
    u2 = J.Utterance(u.durations, [s0, u.streams[1], u.streams[2]])
    st0 = dataclasses.replace(vi.streams[0], vector_length=L2)
    vi2 = dataclasses.replace(vi, streams=[st0, vi.streams[1], vi.streams[2]])
    ref, tr = oracle_pcm(vi2, u2)
    assert np.isfinite(ref).all()
    for kw in (dict(keep_tracks=True), dict(chunk_frames=64, kernel="triple")):
        with J.Batch(vi2, [u2, u2], **kw) as b:
            b.run()
            b.sync()
            got = [b.pcm(0), b.pcm(1)]
            if kw.get("keep_tracks"):
                np.testing.assert_allclose(b.track(0, 0), tr[0], rtol=1e-12, atol=1e-13)
        assert np.array_equal(got[0], got[1])
        assert_pcm_close(got[0], ref, 240, what=(L2, kw))


def test_five_point_delta_windows(ctx):
    """Voices with 5-point delta / acceleration windows (max_width 2 => band width 5): the generic
    band solver and build (`k_mlpg_solve<5>`, [frame][dim] workspace) on all three streams' shapes
    (MCP with GV, MSD LF0 with GV) against the oracle, tracks and PCM."""
    import dataclasses

    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 900, 11)
    w5 = [[1.0], [-0.2, -0.1, 0.0, 0.1, 0.2], [0.285714, -0.142857, -0.285714, -0.142857, 0.285714]]
    streams = [dataclasses.replace(vi.streams[0], windows=w5), dataclasses.replace(vi.streams[1], windows=w5),
               vi.streams[2]]
    vi5 = dataclasses.replace(vi, streams=streams)
    ref, tr = oracle_pcm(vi5, u)
    assert np.isfinite(ref).all()
    with J.Batch(vi5, [u, u], keep_tracks=True) as b:
        b.run()
        b.sync()
        for si in range(3):
            got = b.track(0, si)
            assert np.array_equal(got == O.NODATA, tr[si] == O.NODATA)
            np.testing.assert_allclose(got, tr[si], rtol=1e-12, atol=1e-13)
        g0, g1 = b.pcm(0), b.pcm(1)
    assert np.array_equal(g0, g1)
    assert_pcm_close(g0, ref, 240)


@pytest.mark.parametrize("width", [7, 9])
def test_seven_and_nine_point_delta_windows(ctx, width):
    """Round 6: windows of up to nine taps (band width 9; the reference takes any width, `model/voice/window.rs:19-56`):
    the generic build and band solve instantiated for band widths 7 and 9, all three streams' shapes against the
    oracle; ten taps are refused loudly."""
    import dataclasses

    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 700, 12)
    h = width // 2
    k = np.arange(-h, h + 1, dtype=np.float64)
    d1 = (k / np.sum(k * k)).tolist()                      # least-squares slope over the window
    d2 = (k * k - np.mean(k * k))
    d2 = (2.0 * d2 / np.sum(d2 * d2 * 1.0) * np.sum(np.abs(d2)) / width).tolist()  # a curvature-like zero-sum window
    wn = [[1.0], d1, d2]
    streams = [dataclasses.replace(vi.streams[0], windows=wn), dataclasses.replace(vi.streams[1], windows=wn),
               vi.streams[2]]
    viw = dataclasses.replace(vi, streams=streams)
    ref, tr = oracle_pcm(viw, u)
    assert np.isfinite(ref).all()
    with J.Batch(viw, [u, u], keep_tracks=True) as b:
        b.run()
        b.sync()
        for si in range(3):
            got = b.track(0, si)
            assert np.array_equal(got == O.NODATA, tr[si] == O.NODATA)
            np.testing.assert_allclose(got, tr[si], rtol=1e-12, atol=1e-13)
        g0, g1 = b.pcm(0), b.pcm(1)
    assert np.array_equal(g0, g1)
    assert_pcm_close(g0, ref, 240)
    if width == 9:
        w11 = [[1.0], [0.0] * 11, d2]
        with pytest.raises(J.JbError) as ei:
            J.Batch(dataclasses.replace(vi, streams=[dataclasses.replace(vi.streams[0], windows=w11)] + streams[1:]), [u])
        assert "UNSUPPORTED" in str(ei.value)


@pytest.mark.parametrize("fs,fp,alpha,nlpf", [(16000, 80, 0.42, 31), (48000, 90, 0.55, 31), (48000, 240, 0.55, 15),
                                              (22050, 100, 0.45, 31)])
def test_other_frame_periods_and_lpf_orders(ctx, fs, fp, alpha, nlpf):
    """Frame periods other than 240 (divisible by 4 or not: the 32-byte PCM stores and the wave-per-frame
    excitation kernel need fperiod % 4 == 0, the generic paths take over at 90), another warping
    alpha, and a 15-tap LPF stream (second specialisation of the split excitation).  HIP vs oracle,
    default kernels and the throughput kernel."""
    import dataclasses

    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 500, 21)
    streams = list(vi.streams)
    ustreams = list(u.streams)
    if nlpf != vi.streams[2].vector_length:
        L = vi.streams[2].vector_length
        lo = (L - nlpf) // 2  # centre taps of the (symmetric) low-pass filters
        s2 = u.streams[2]
        ustreams[2] = dataclasses.replace(s2, mean=s2.mean[:, lo:lo + nlpf].copy(), var=s2.var[:, lo:lo + nlpf].copy())
        streams[2] = dataclasses.replace(vi.streams[2], vector_length=nlpf)
    vi2 = dataclasses.replace(vi, sampling_frequency=fs, fperiod=fp, alpha=alpha, streams=streams)
    u2 = J.Utterance(u.durations, ustreams)
    ref, _ = oracle_pcm(vi2, u2)
    assert len(ref) == 500 * fp and np.isfinite(ref).all()
    for kw in (dict(), dict(chunk_frames=64, kernel="triple"), dict(chunk_frames=64, kernel="wave")):
        got, info = run(vi2, [u2, u2], **kw)
        assert np.array_equal(got[0], got[1])
        assert_pcm_close(got[0], ref, fp, what=(fs, fp, alpha, nlpf, kw))


def lpf_taps_utterance(tab, vi, frames, seed, nlpf):
    """The nitech utterance with its (static-only) LPF stream cut to its centre taps or widened with small flanks."""
    import dataclasses

    u = synth.synth_utterance(tab, frames, seed)
    streams, ustreams = list(vi.streams), list(u.streams)
    L = vi.streams[2].vector_length
    if nlpf != L:
        s2 = u.streams[2]
        S = s2.mean.shape[0]
        assert s2.mean.shape[1] == L  # one window
        if nlpf < L:
            lo = (L - nlpf) // 2
            mean, var = s2.mean[:, lo:lo + nlpf].copy(), s2.var[:, lo:lo + nlpf].copy()
        else:
            rng = np.random.default_rng(seed + 7)
            lo = (nlpf - L) // 2
            mean = rng.normal(0.0, 2e-3, (S, nlpf))
            var = np.full((S, nlpf), float(s2.var.mean()))
            mean[:, lo:lo + L] = s2.mean
            var[:, lo:lo + L] = s2.var
        ustreams[2] = dataclasses.replace(s2, mean=mean, var=var)
        streams[2] = dataclasses.replace(vi.streams[2], vector_length=nlpf)
    return streams, J.Utterance(u.durations, ustreams)


@pytest.mark.parametrize("fs,fp,nlpf", [(48000, 75, 31), (48000, 83, 31), (48000, 131, 15), (48000, 134, 31),
                                        (48000, 166, 31), (48000, 254, 15), (48000, 307, 31), (16000, 20, 31),
                                        (16000, 25, 5), (8000, 7, 3), (48000, 240, 127), (48000, 80, 65),
                                        (22050, 110, 255), (48000, 50, 1023), (48000, 240, 2047)])
def test_frame_periods_and_lpf_orders_the_reference_is_generic_in(ctx, fs, fp, nlpf):
    """Vocoder::new is generic in the frame period and the number of low-pass taps (vocoder/mod.rs:45-70; the ring
    buffer of excitation.rs:113-123 has nlpf slots).  Frame periods without a useful divisor <= 64 (75 = 3 x 25 under
    31 taps, primes) run on blocks with a shorter last block; more than 64 taps, frame periods below 30 samples and
    below nlpf - 1 (a sample's window then spans several frames) take k_excite_any.  HIP vs oracle, default kernels,
    the throughput kernel (even frame periods; the wave kernel otherwise) and the wave kernel."""
    import dataclasses

    eng, tab, vi = ctx
    T = 300
    streams, u2 = lpf_taps_utterance(tab, vi, T, 23, nlpf)
    vi2 = dataclasses.replace(vi, sampling_frequency=fs, fperiod=fp, streams=streams)
    ref, tr = oracle_pcm(vi2, u2)
    assert len(ref) == T * fp and np.isfinite(ref).all() and np.abs(ref).max() > 0
    for kw in (dict(), dict(chunk_frames=64, kernel="triple"), dict(chunk_frames=64, kernel="wave"), dict(serial=True)):
        with J.Batch(vi2, [u2, u2], keep_tracks=True, **kw) as b:
            b.run()
            b.sync()
            g0, g1, exc = b.pcm(0), b.pcm(1), b.excitation(0)
        assert np.array_equal(g0, g1)
        assert_pcm_close(g0, ref, fp, what=(fs, fp, nlpf, kw))
    _, exc_ref, _ = O.vocoder(fs, fp, vi.alpha, 1.0, tr[1][:, 0], tr[0], tr[2], dumps=True)
    assert np.abs(exc - exc_ref).max() <= 1e-9 * max(1.0, np.abs(exc_ref).max())


def test_shape_limits_fail_loudly(ctx):
    """What is still refused (JB_ERR_UNSUPPORTED, not mis-synthesised): more low-pass taps than k_excite_any keeps a
    block's history for in LDS."""
    import dataclasses

    eng, tab, vi = ctx
    streams, u = lpf_taps_utterance(tab, vi, 20, 1, 2049)
    with pytest.raises(J.JbError) as ei:
        J.Batch(dataclasses.replace(vi, streams=streams), [u])
    assert "UNSUPPORTED" in str(ei.value)


@pytest.mark.parametrize("case", ["static_mcp_with_gv", "no_gv_anywhere", "delta_only"])
def test_other_window_sets_and_gv_flags(ctx, case):
    """Stream shapes off the nitech voice's: a static-only spectral stream that still has GV (band
    width 1 through the generic solver), GV switched off on every stream (the fused sweeps end
    after the substitutions), static + delta only (two windows).  HIP vs oracle, tracks and PCM."""
    import dataclasses

    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 600, 31)
    streams, ustreams = list(vi.streams), list(u.streams)

    def cut_windows(si, nw):
        L = vi.streams[si].vector_length
        st = u.streams[si]
        ustreams[si] = dataclasses.replace(st, mean=st.mean[:, :nw * L].copy(), var=st.var[:, :nw * L].copy())
        streams[si] = dataclasses.replace(streams[si], windows=vi.streams[si].windows[:nw])

    if case == "static_mcp_with_gv":
        cut_windows(0, 1)
    elif case == "delta_only":
        cut_windows(0, 2)
        cut_windows(1, 2)
    else:
        for si in (0, 1):
            streams[si] = dataclasses.replace(streams[si], use_gv=False)
            ustreams[si] = dataclasses.replace(ustreams[si], gv_mean=None, gv_var=None, gv_switch=None)
    vi2 = dataclasses.replace(vi, streams=streams)
    u2 = J.Utterance(u.durations, ustreams)
    ref, tr = oracle_pcm(vi2, u2)
    assert np.isfinite(ref).all()
    with J.Batch(vi2, [u2, u2], keep_tracks=True) as b:
        b.run()
        b.sync()
        for si in range(3):
            got = b.track(0, si)
            assert np.array_equal(got == O.NODATA, tr[si] == O.NODATA)
            np.testing.assert_allclose(got, tr[si], rtol=1e-12, atol=1e-13)
        g0, g1 = b.pcm(0), b.pcm(1)
    assert np.array_equal(g0, g1)
    assert_pcm_close(g0, ref, 240)


def test_many_tiny_utterances(ctx):
    """A batch of 4,000 utterances of 30-70 frames (220 k frames: the throughput kernel with most
    utterances shorter than two chunks; one block / grid row per utterance in the serial kernels):
    a sample of them against the oracle, duplicates bit-identical."""
    eng, tab, vi = ctx
    base = [synth.synth_utterance(tab, 30 + (7 * i) % 41, 300 + i) for i in range(25)]
    utts = [base[i % 25] for i in range(4000)]
    with J.Batch(vi, utts) as b:
        b.run()
        b.sync()
        info = b.info()
        picks = {i: b.pcm(i) for i in (0, 1, 24, 25, 26, 1999, 3975, 3999)}
    assert info["n_items"] >= 4000
    for i, g in picks.items():
        assert len(g) == int(base[i % 25].durations.sum()) * 240
        assert np.array_equal(g, picks[i % 25]) if i % 25 in picks else True
        ref, _ = oracle_pcm(vi, base[i % 25])
        assert_pcm_close(g, ref, 240, what=i)


def test_one_very_long_utterance(ctx):
    """A single 200,000-frame (17 min) utterance: 98 GV tiles per row, 12,000 states in the state
    walk, the throughput kernel (batches of >= 190 k frames) fed by one utterance only; the same
    utterance through the wave kernel at one item per SIMD.  HIP vs oracle."""
    eng, tab, vi = ctx
    u = synth.synth_utterance(tab, 200000, 77)
    got, info = run(vi, [u])
    assert len(got[0]) == 200000 * 240 and info["n_items"] > 1024
    ref, _ = oracle_pcm(vi, u)
    e = rel_rms(got[0], ref)
    print("200 k frames: rel RMS vs oracle", e, info)
    assert_pcm_close(got[0], ref, 240, chunk=info["chunk_frames"])
    gotw, infow = run(vi, [u], kernel="wave")
    assert 512 < infow["n_items"] <= 2048
    assert_pcm_close(gotw[0], ref, 240)


def test_device_pool_reuse_release_and_dirty_blocks(oracle_voice):
    """Device blocks of finished batches go to the next batch (dirty, not zeroed) or back to the
    driver with jb_release_cached_memory: same bits either way, for equal and for different shapes."""
    v = oracle_voice
    d1, s1 = oracle_states(v, SAMPLE_SENTENCE_1)
    d2, s2 = oracle_states(v, SAMPLE_SENTENCE_2)
    vi = voice_info(v)
    L = J.lib()
    assert L.jb_release_cached_memory() == 0
    fresh1 = J.paramgen_vocode_batch(vi, [to_utt(d1, s1)])[0]
    fresh2 = J.paramgen_vocode_batch(vi, [to_utt(d2, s2), to_utt(d1, s1)])
    # now every block comes out of the pool, written by the batches before
    for _ in range(3):
        again2 = J.paramgen_vocode_batch(vi, [to_utt(d2, s2), to_utt(d1, s1)])
        again1 = J.paramgen_vocode_batch(vi, [to_utt(d1, s1)])[0]
        assert np.array_equal(again1, fresh1)
        assert np.array_equal(again2[0], fresh2[0]) and np.array_equal(again2[1], fresh2[1])
    assert L.jb_release_cached_memory() == 0
    assert np.array_equal(J.paramgen_vocode_batch(vi, [to_utt(d1, s1)])[0], fresh1)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])
def test_random_shape_combinations(ctx, seed):
    """Seeded random COMBINATIONS of what the tests above vary one at a time: mel-cepstral order,
    frame period, LPF order, warping alpha, volume, post-filter beta, a ragged batch with an empty
    utterance -- every utterance against the oracle."""
    import dataclasses

    eng, tab, vi = ctx
    rng = np.random.default_rng(1000 + seed)
    L = vi.streams[0].vector_length
    W = len(vi.streams[0].windows)
    L2 = int(rng.choice([8, 13, 20, 25, 30, 35]))
    if seed <= 6:
        fs, fp = [(16000, 80), (48000, 240), (44100, 220), (48000, 96), (22050, 100), (48000, 120)][seed - 1]
        nlpf = int(rng.choice([7, 15, 23, 31]))
    else:  # any frame period (blocks with a shorter last block, k_excite_any below 30 samples) and any odd tap count
        fs, fp = [(48000, 77), (44100, 201), (16000, 27), (48000, 323)][seed - 7]
        nlpf = 2 * int(rng.integers(0, 16)) + 1
    alpha = float(rng.choice([0.42, 0.5, 0.55]))
    beta = float(rng.choice([0.0, 0.0, 0.2, 0.5]))
    volume = float(rng.choice([1.0, 0.5, 1.7]))
    lens = [int(x) for x in rng.integers(1, 900, size=4)] + [0]
    utts = []
    for k, T in enumerate(lens):
        if T == 0:
            u = synth.synth_utterance(tab, 5, 50 + k)
            S = 0
            streams = [dataclasses.replace(s, mean=s.mean[:0], var=s.var[:0],
                                           msd=None if s.msd is None else s.msd[:0],
                                           gv_switch=None if s.gv_switch is None else s.gv_switch[:0])
                       for s in u.streams]
            u = J.Utterance(u.durations[:0], streams)
        else:
            u = synth.synth_utterance(tab, T, 50 * seed + k)
        S = len(u.durations)
        m0, s2 = u.streams[0], u.streams[2]
        lo = (vi.streams[2].vector_length - nlpf) // 2
        st0 = dataclasses.replace(m0, mean=m0.mean.reshape(S, W, L)[:, :, :L2].reshape(S, W * L2).copy(),
                                  var=m0.var.reshape(S, W, L)[:, :, :L2].reshape(S, W * L2).copy(),
                                  gv_mean=m0.gv_mean[:L2].copy(), gv_var=m0.gv_var[:L2].copy())
        st2 = dataclasses.replace(s2, mean=s2.mean[:, lo:lo + nlpf].copy(), var=s2.var[:, lo:lo + nlpf].copy())
        utts.append(J.Utterance(u.durations, [st0, u.streams[1], st2]))
    streams = [dataclasses.replace(vi.streams[0], vector_length=L2), vi.streams[1],
               dataclasses.replace(vi.streams[2], vector_length=nlpf)]
    vi2 = dataclasses.replace(vi, sampling_frequency=fs, fperiod=fp, alpha=alpha, beta=beta, volume=volume,
                              streams=streams)
    got, info = run(vi2, utts)
    for u, g, T in zip(utts, got, lens):
        assert len(g) == T * fp
        if T == 0:
            continue
        sts = []
        for i, s in enumerate(u.streams):
            si = vi2.streams[i]
            msd = s.msd if s.msd is not None else np.full(len(u.durations), DMAX)
            sts.append(O.StreamStates(si.vector_length, len(si.windows), si.is_msd, si.use_gv,
                                      [len(w) for w in si.windows], [c for w in si.windows for c in w],
                                      s.mean, s.var, msd, s.gv_mean, s.gv_var, s.gv_switch,
                                      s.gv_weight, s.msd_threshold))
        tr = [O.mlpg(s, u.durations) for s in sts]
        ref = O.vocoder(fs, fp, alpha, volume, tr[1][:, 0], tr[0], tr[2], beta=beta)
        assert np.isfinite(ref).all()
        assert_pcm_close(g, ref, fp, what=(seed, L2, fs, fp, nlpf, alpha, beta, volume, T))
