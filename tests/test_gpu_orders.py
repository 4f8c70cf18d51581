"""The throughput vocoder kernel at every mel-cepstral order the reference takes (round 6; VERDICT r5 "missing" 1).

The reference is generic in the order (`/root/reference/src/vocoder/mod.rs:45-70`, `mlsa.rs:38-45,127-163`); until
round 6 `k_vocoder_lt` existed for nitech's two orders only and every other voice fell back to the wave-per-chunk
kernel.  Here: voices of other orders (synth.with_order: nitech's MCP stream cut or widened) through the C ABI --
 * small batches with the lane kernel forced, at the borders of every code (lane triples 25 / 31 / 35, one stage per
   lane 41 / 51 / 61) against the oracle;
 * full batches, 1024 utterances x 2,000 frames (eight distinct x 128 copies): `jb_batch_kernel_info` must report the
   lane kernel at two waves per SIMD, copies must be bitwise equal, the distinct ones meet the oracle."""
import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests.conftest import VOICE
from tests.helpers import assert_pcm_close
from tests.test_gpu_configs import oracle_pcm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    eng = J.Engine.load([VOICE])
    return eng, synth.VoiceTables(eng), eng.voice_info()


@pytest.mark.parametrize("nmcp", [7, 12, 24, 26, 31, 32, 34, 36, 41, 42, 51, 52, 61])
def test_lane_kernel_small_batch_vs_oracle(ctx, nmcp):
    eng, tab, vi = ctx
    vi2, u2 = synth.with_order(vi, synth.synth_utterance(tab, 700, 3), nmcp)
    ref, _ = oracle_pcm(vi2, u2)
    assert np.isfinite(ref).all()
    for waves_hint in (64, 16):  # chunk lengths: few items (one wave per SIMD) / many
        with J.Batch(vi2, [u2, u2, u2], chunk_frames=waves_hint, kernel="triple") as b:
            b.run()
            b.sync()
            name, _ = b.kernel_info()
            got = [b.pcm(i) for i in range(3)]
        assert name == "k_vocoder_lt"
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
        assert_pcm_close(got[0], ref, 240, what=(nmcp, waves_hint))


@pytest.mark.parametrize("nmcp", [20, 30, 40, 50, 60])
def test_lane_kernel_full_batch(ctx, nmcp):
    eng, tab, vi = ctx
    T, distinct, copies = 2000, 8, 128
    pairs = [synth.with_order(vi, synth.synth_utterance(tab, T, 7000 + i), nmcp, seed=100 + i) for i in range(distinct)]
    vi2 = pairs[0][0]
    utts = [pairs[i % distinct][1] for i in range(distinct * copies)]
    with J.Batch(vi2, utts) as b:
        b.run()
        b.sync()
        name, waves = b.kernel_info()
        info = b.info()
        first = [b.pcm(i) for i in range(distinct)]
        for i in (distinct, 5 * distinct + 3, distinct * copies - 1):
            assert np.array_equal(b.pcm(i), first[i % distinct]), i
    print(f"order {nmcp - 1}: {name} at {waves} waves per SIMD, {info}")
    assert name == "k_vocoder_lt" and waves == 2
    for i in range(distinct):
        ref, _ = oracle_pcm(vi2, pairs[i][1])
        assert_pcm_close(first[i], ref, 240, what=(nmcp, i))


@pytest.mark.parametrize("nmcp", [62, 63, 64])
def test_orders_above_sixty(ctx, nmcp):
    """Round 6: nmcp up to 64 (six taps per lane in the wave kernels, the generic MLPG kernels, the 64-wide mc2b tile);
    the reference has no limit (`vocoder/mod.rs:45-70`), this library's is now 64 -- the width of the lane-per-tap
    kernels (post-filter, MGLSA).  Chunked and unchunked runs against the oracle, and the refusal behind the limit."""
    eng, tab, vi = ctx
    vi2, u2 = synth.with_order(vi, synth.synth_utterance(tab, 600, 5), nmcp)
    ref, tr = oracle_pcm(vi2, u2)
    assert np.isfinite(ref).all()
    for kw in (dict(keep_tracks=True), dict(serial=True), dict(chunk_frames=48)):
        with J.Batch(vi2, [u2, u2], **kw) as b:
            b.run()
            b.sync()
            g0, g1 = b.pcm(0), b.pcm(1)
            if kw.get("keep_tracks"):
                np.testing.assert_allclose(b.track(0, 0), tr[0], rtol=1e-12, atol=1e-13)
        assert np.array_equal(g0, g1)
        assert_pcm_close(g0, ref, 240, what=(nmcp, kw))


def test_order_limit_fails_loudly(ctx):
    eng, tab, vi = ctx
    vi2, u2 = synth.with_order(vi, synth.synth_utterance(tab, 100, 5), 65)
    with pytest.raises(J.JbError) as ei:
        J.Batch(vi2, [u2])
    assert "UNSUPPORTED" in str(ei.value)
