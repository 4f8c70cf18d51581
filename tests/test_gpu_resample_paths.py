"""Every path of k_resample against the rule itself, bit for bit.  The kernel's contract is "each output is h[p][0] x[.]
followed by ntaps - 1 explicit FMAs in ascending j: a function of x and h alone, not of the tile, wave or lane"; the
host probe (tests/plan/resample_probe.cpp) states that with std::fma, and the cases of tests/resample_ref.py reach the
LDS window with 4, 2 and 1 waves per row block, the row cap, the global-memory path, every pad shift, the largest L, M
and ntaps -- each asserted from jb_resample_geometry -- at lengths that put 1, rows - 1, rows, rows + 1 and
2 rows + 1 rows into the tiles with whole and partial last rows.  What a wrong kernel shows here and not in
tests/test_gpu_resample.py (whose six pairs reach the 4-wave path and two 1-wave tables, under an RMS gate), worked out
on the kernel's index arithmetic:
  - a window too short.  The last slot a tile reads is (rows - 1) M + floor((L - 1) M / L) + ntaps - 1, which is
    wlen - 2 where L >= M and lower otherwise: wlen - 1 changes no output (the last slot is slack), wlen - 2 does in the
    last phase of a full tile's last row, where the last tap is not zero -- 16000 -> 48000, 44100 -> 48000,
    8000 -> 44100, 1 -> 2048 at rows and 2 rows + 1 rows;
  - `i < tl.rows` dropped: in a tile that is not the utterance's last, the lanes past its rows compute rows of the
    tiles behind it from slots beyond this tile's window -- the 1-wave cases of fewer than 64 rows (3, 12, 24, 55) at
    rows + 1 and 2 rows + 1 rows; one differing output is named by row and phase;
  - a phase step that does not match the row mapping of a 2-wave table (step 2 from phase 0 on all four waves): the odd
    phases are never written -- 48000 -> 25000 (L = 25); a wrong row mapping there (rows 64..127 on waves 2 and 3
    instead of wave 1) leaves rows unwritten at any L -- 48000 -> 1500 too;
  - the global path's `a < n_in` made `<=`: the sample behind an utterance is not zero but whatever lies there, the next
    utterance of the same call -- 48000 -> 400 and 2048 -> 1, in the last C outputs of every length.
"""
import shutil

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import synth
from tests import resample_ref as R
from tests.conftest import VOICE

pytestmark = pytest.mark.gpu

IN = 48000


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not shutil.which(R.HIPCC):
        pytest.skip("hipcc not installed")
    return R.build_probe(tmp_path_factory.mktemp("resample_probe"))


@pytest.fixture(scope="module")
def eng():
    assert J.lib().jb_device_count() > 0
    return J.Engine.load([VOICE])


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("c", R.CASES, ids=R.IDS)
def test_device_is_the_fma_chain_bit_for_bit(probe, tmp_path, c):
    g = J.resample_geometry(c.in_hz, c.out_hz)
    R.check_class(g, c)
    ns = R.lengths(g.L, g.M, g.ntaps, g.rows)
    xs = R.signals(c, ns)
    want = R.run_probe(probe, c.in_hz, c.out_hz, xs, tmp_path)
    got = J.resample(xs, c.in_hz, c.out_hz)  # all lengths in one call: the utterances lie side by side on the device
    assert len(got) == len(want) == len(ns)
    for n, y, w in zip(ns, got, want):
        assert y.shape == w.shape == (R.out_len(n, g.L, g.M),), (c, n)
        if y.tobytes() != w.tobytes():
            bad = np.flatnonzero(y.view(np.uint64) != w.view(np.uint64))
            k = int(bad[0])
            pytest.fail(f"{c.in_hz} -> {c.out_hz} ({c.path}, {c.what}), n_in {n}: {bad.size} of {y.size} outputs "
                        f"differ, first k = {k} (row {k // g.L} = tile {k // g.L // g.rows} row {k // g.L % g.rows}, "
                        f"phase index {k % g.L}): {y[k]!r} against {w[k]!r}")


MIX = [0, 25000, 400, 11025, IN, 32000]
MIX_PATHS = ["identity", R.LDS2, R.GLOBAL, R.LDS1, "identity", R.LDS4]


@pytest.mark.parametrize("pcm_i16", [False, True])
def test_paths_side_by_side_in_one_launch(eng, pcm_i16):
    """Identity, 2-wave, global, 1-wave with pad 7, identity and 4-wave tables in one launch under one dynamic-LDS
    size: every utterance is the converter's output of its own native PCM, or the clamp-and-truncate of it (the first
    run of k_resample<int16_t> on the 2-wave and global paths)."""
    for hz, path in zip(MIX, MIX_PATHS):
        g = J.resample_geometry(IN, hz or IN)
        if path == "identity":
            assert g.identity == 1 and g.lds == 0
        else:
            assert (g.identity, g.lds, g.row_waves) == (0, path != R.GLOBAL, R.WAVES[path]), (hz, path)
    assert J.resample_geometry(IN, 11025).pad == 7
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    utts = [synth.synth_utterance(tab, T, 300 + T) for T in (700, 310, 450, 260, 130, 520)]
    with J.Batch(vi, utts, pcm_i16=pcm_i16) as b:
        b.set_output_rate(MIX)
        b.run()
        b.sync()
        allv = b.pcm_all()
        for i, hz in enumerate(MIX):
            nat = b.pcm_native(i)
            assert nat.size == b.num_frames(i) * vi.fperiod and b.output_rate(i) == (hz or IN)
            conv = nat if (hz or IN) == IN else J.resample(nat, IN, hz)
            assert b.num_samples(i) == conv.size
            want = np.clip(conv, -32768.0, 32767.0).astype(np.int16) if pcm_i16 else conv
            same_bits(b.pcm_i16(i) if pcm_i16 else b.pcm(i), want)
            same_bits(allv[i], want)
