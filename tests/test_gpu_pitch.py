"""The pitch stage on the GPU (jb_pitch.hip): jb_pitch_pcm_batch against the host rule jb_pitch_host (which
tests/test_pitch_abi.py holds to the long double model) -- the chosen lags equal, the tracker's two raw columns equal
bit for bit (steps 1 to 5 use + - * / sqrt and tables alone), the processed columns (exp, pow and a division) within
the 8 times gate of the long double model -- on ragged batches of five units: lengths of 0, 1, a window less a sample,
one frame exactly, and frame and sample counts on either side of every workgroup's share (k_pitch_post: 4 frames;
k_pitch_cols: 256 frames; k_pitch_down: 1,024 samples at 4 kHz), at rates with 1, 40 and 160 phases, both grids, f32 and
f64 elements, three, four and the two raw columns."""
import numpy as np
import pytest

import jbonsai_amd as J
from tests import pitch_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
GATE = 8
POST, COLS, TILE = 4, 256, 1024  # kPitchPostFrames, kPitchLanes, kPitchTile


@pytest.fixture(scope="module", autouse=True)
def device():
    assert J.lib().jb_device_count() > 0


def samples_for_frames(T, wl, hop, kaldi):
    """The fewest samples that give T frames"""
    if T == 0:
        return 0
    return T * hop - hop // 2 if kaldi else wl + (T - 1) * hop


def samples_for_n4(n4, hz):
    """The most samples whose 4 kHz signal has n4 samples"""
    return n4 * hz // 4000


def short_lengths(hz, grid):
    g = J.pitch_geometry(J.pitch(grid=grid), hz, 0)
    kaldi = grid == "kaldi"
    out = [0, 1, g.wl - 1, samples_for_frames(1, g.wl, g.hop, kaldi)]
    out += [samples_for_frames(T, g.wl, g.hop, kaldi) for T in (POST - 1, POST, POST + 1)]
    out += [samples_for_n4(m, hz) for m in (TILE - 1, TILE, TILE + 1)]
    return out


_host = {}


def host(x, hz, seed, n, grid, **mode):
    """jb_pitch_host of a signal, computed once per (signal, mode)"""
    key = (hz, seed, n, grid, tuple(sorted(mode.items())))
    if key not in _host:
        _host[key] = J.pitch_host(x, hz, J.pitch(grid=grid, **mode), grid=True)
    return _host[key]


def held(name, got, f64, ref):
    e, e64 = float(np.abs(got.astype(LD) - ref).max()), float(np.abs(f64.astype(LD) - ref).max())
    print(f"{name}: device {e:.3e}  float64 model {e64:.3e}  ratio {e / e64 if e64 else float('nan'):.3f}")
    assert e <= GATE * e64, (name, e, e64)


def check_batch(hz, grid, lengths, seed0, **mode):
    """One call over the units of `lengths`: the lags and the raw columns are the host's, the processed ones within the
    gate"""
    o = J.pitch(grid=grid, **mode)
    hzs = hz if isinstance(hz, (list, tuple)) else [hz] * len(lengths)
    xs = [R.test_signal(seed0 + u, hzs[u], n) for u, n in enumerate(lengths)]
    rows, idx = J.pitch_pcm(xs, list(hzs), o)
    assert len(rows) == len(idx) == len(xs)
    for u, x in enumerate(xs):
        want, widx, Q, P = host(x, hzs[u], seed0 + u, lengths[u], grid, **mode)
        T = J.pitch_geometry(o, hzs[u], lengths[u]).T
        assert rows[u].shape == want.shape == (T, want.shape[1]) and rows[u].dtype == want.dtype, (u, rows[u].shape)
        assert np.array_equal(idx[u], widx), (hzs[u], grid, lengths[u], np.flatnonzero(idx[u] != widx)[:8])
        if mode.get("raw"):
            assert rows[u].tobytes() == want.tobytes(), (hzs[u], grid, lengths[u], np.argwhere(rows[u] != want)[:8])
            continue
        if T == 0:
            continue
        if not mode.get("f64"):  # f32 elements: the host's, or their neighbour where the f64 values differ
            assert np.all(np.abs(rows[u].astype(np.float64) - want) <= np.spacing(np.abs(want))), (u, lengths[u])
            continue
        p = P[np.arange(T), widx]
        width = want.shape[1]
        ref, c64 = R.columns(widx, p.astype(LD), o, LD, width), R.columns(widx, p, o, np.float64, width)
        for c in range(width):
            if c == 3:
                assert np.array_equal(rows[u][:, 3], want[:, 3])  # the raw log-pitch is a table's entry
            else:
                held(f"{hzs[u]} {grid} n={lengths[u]} column {c + 1}", rows[u][:, c], c64[:, c], ref[:, c])


@pytest.mark.parametrize("grid", ["snip", "kaldi"])
@pytest.mark.parametrize("hz", [8000, 11025, 16000, 44100, 48000])
def test_seam_is_the_host_rule(hz, grid):
    n = short_lengths(hz, grid)
    check_batch(hz, grid, n[:5], 100, raw=True, f64=True)
    check_batch(hz, grid, n[5:], 105, raw=True, f64=True)
    check_batch(hz, grid, n[3:8], 103, raw_log=True, f64=True)


@pytest.mark.parametrize("grid", ["snip", "kaldi"])
def test_frame_counts_around_the_column_kernels_workgroup(grid):
    g = J.pitch_geometry(J.pitch(grid=grid), 16000, 0)
    n = [samples_for_frames(T, g.wl, g.hop, grid == "kaldi") for T in (COLS - 1, COLS, COLS + 1)]
    assert max(n) <= 3 * 16000
    check_batch(16000, grid, [n[0], 0, n[1], 1, n[2]], 200, raw_log=True, f64=True)
    check_batch(16000, grid, [n[0], 0, n[1], 1, n[2]], 200, raw=True, f64=True)


def test_element_types_and_widths():
    n = short_lengths(16000, "kaldi")
    check_batch(16000, "kaldi", n[3:8], 103)                    # [T][3] f32
    check_batch(16000, "kaldi", n[3:8], 103, raw=True)          # [T][2] f32
    check_batch(16000, "kaldi", n[3:8], 103, f64=True)          # [T][3] f64
    check_batch(16000, "kaldi", n[3:8], 103, raw_log=True)      # [T][4] f32


def test_one_call_over_five_rates():
    hzs = [8000, 11025, 16000, 44100, 48000]
    n = [hz * 3 // 10 + 7 * u for u, hz in enumerate(hzs)]
    check_batch(hzs, "kaldi", n, 300, raw=True, f64=True)
    check_batch(hzs, "snip", n, 300, raw_log=True, f64=True)


def test_other_grids_and_an_empty_call():
    n = short_lengths(16000, "snip")[3:8]
    check_batch(16000, "snip", n, 400, raw=True, f64=True, min_f0=399.0, max_f0=400.0, delta_pitch=0.002)  # 2 lags
    check_batch(16000, "snip", n[:2], 400, raw=True, f64=True, delta_pitch=0.002034)                       # 1024 lags
    check_batch(16000, "kaldi", n, 400, raw_log=True, f64=True, win_us=20000, hop_us=5000, norm_left=3, norm_right=1)
    assert J.pitch_pcm([], 16000, J.kaldi_pitch()) == ([], [])
    zeros, zidx = J.pitch_pcm([np.zeros(4000)], 16000, J.pitch(raw=True, f64=True))
    assert zeros[0].shape == (25, 2) and not zeros[0][:, 0].any() and np.all(zeros[0][:, 1] == 400.0) and not zidx[0].any()
