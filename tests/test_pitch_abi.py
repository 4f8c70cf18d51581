"""The pitch stage without a GPU (jbonsai_amd/csrc/jb_pitch.cpp): the options' refusals with their fields, the
geometry against the filterbank stage's, the lag grid, jb_pitch_host against the long double model of
tests/pitch_ref.py under the 8 times gate (the grid values, the path's cost, the columns), a known answer, and the
edge cases of the frame count, the normalisation window and the lag grid."""
import ctypes as C

import numpy as np
import pytest

import jbonsai_amd as J
from tests import pitch_ref as R

INVALID, UNSUPPORTED, BUFFER = -1, -2, -8
LD = np.longdouble
GATE = 8  # the ratio every sibling stage is held to


def refused(code, word, fn, *args):
    with pytest.raises(J.JbError) as e:
        fn(*args)
    assert e.value.code == code and word in str(e.value), (code, word, e.value.args)


@pytest.mark.parametrize("field,value", [
    ("grid", 2), ("flags", 8), ("flags", J.PITCH_RAW | J.PITCH_RAW_LOG), ("win_us", 25100), ("win_us", 1750),
    ("win_us", 128250), ("hop_us", 0), ("hop_us", 10001), ("min_f0", 0.0), ("min_f0", float("nan")), ("max_f0", 40.0),
    ("max_f0", 2500.0), ("delta_pitch", 0.0), ("delta_pitch", 2.0), ("penalty_factor", -1.0),
    ("soft_min_f0", float("inf")), ("nccf_ballast", -1.0), ("pov_scale", float("nan")), ("pitch_scale", float("inf")),
    ("delta_scale", float("nan")), ("norm_left", 4097), ("norm_right", 4097)])
def test_each_field_fault_names_its_field(field, value):
    o = J.kaldi_pitch()
    setattr(o, field, value)
    refused(INVALID, field, J.pitch_geometry, o, 16000, 16000)
    refused(INVALID, field, J.pitch_lags, o)
    refused(INVALID, field, J.pitch_host, np.zeros(16), 16000, o)


def test_limits_name_their_fields():
    o = J.kaldi_pitch()
    o.reserved[2] = 1
    refused(INVALID, "reserved", J.pitch_geometry, o, 16000, 0)
    refused(INVALID, "min_f0", J.pitch_geometry, J.pitch(min_f0=15.0), 16000, 0)  # an integer lag above 255
    refused(INVALID, "delta_pitch", J.pitch_geometry, J.pitch(delta_pitch=0.001), 16000, 0)  # above 1024 lags
    refused(INVALID, "hz", J.pitch_geometry, J.kaldi_pitch(), 3999, 0)
    refused(UNSUPPORTED, "JB_PITCH_MAX_DOWN", J.pitch_geometry, J.kaldi_pitch(), 44101, 0)
    assert J.lib().jb_pitch_geometry(None, 16000, 0, None) == INVALID
    assert C.sizeof(J.PitchOpts) == 112 and C.sizeof(J.PitchGeometry) == 56
    x = np.zeros(16000)
    out = np.zeros(8, dtype=np.float32)
    rc = J.lib().jb_pitch_host(x.ctypes.data, x.size, 16000, C.byref(J.kaldi_pitch()), out.ctypes.data, out.nbytes, None,
                               None, None)
    assert rc == BUFFER


def test_defaults():
    o = J.kaldi_pitch()
    assert (o.win_us, o.hop_us, o.min_f0, o.max_f0, o.delta_pitch, o.penalty_factor, o.soft_min_f0, o.nccf_ballast,
            o.pov_scale, o.pitch_scale, o.delta_scale, o.norm_left, o.norm_right, o.grid, o.flags) == \
        (25000, 10000, 50.0, 400.0, 0.005, 0.1, 10.0, 7000.0, 2.0, 2.0, 10.0, 75, 75, J.PITCH_KALDI, 0)
    g = J.pitch_geometry(o, 16000, 16000)
    assert (g.S, g.lag_first, g.lag_last, g.wl4, g.sh4, g.width, g.elem, g.choice_bytes) == (417, 7, 83, 100, 40, 3, 4, 834)
    lags = J.pitch_lags(o)
    want = R.lags(o)
    assert lags.size == 417 and R.lag_range(o) == (7, 83)
    assert np.array_equal(lags, want.astype(np.float64))  # the recipe, rounded once
    assert lags[0] == 1 / 400 and lags[-1] <= 1 / 50 < lags[-1] * 1.005


@pytest.mark.parametrize("hz", [8000, 16000, 44100, 48000])
@pytest.mark.parametrize("grid", ["snip", "kaldi"])
def test_T_is_the_filterbank_stages(hz, grid):
    o = J.pitch(grid=grid)
    fb = J.fbank(25, 10, n_mels=23)
    fr = J.frame(reflect=grid == "kaldi")
    wl, hop = J.fbank_geometry(hz, fb)[:2]
    for n in (0, 1, wl - 1, wl, wl + hop, wl + hop - 1, 3 * hop + hop // 2 - 1, 3 * hop + hop // 2):
        g = J.pitch_geometry(o, hz, n)
        want = J.fbank_framed_geometry(hz, fb, fr, n)
        assert (g.wl, g.hop, g.T) == (want[0], want[1], want[3]), (hz, grid, n)
        assert g.n4 == -(-n * 4000 // hz)
        rows, idx = J.pitch_host(np.ones(n), hz, o)
        assert rows.shape == (g.T, 3) and idx.shape == (g.T,)


def model(x, hz, o, T):
    """(Q, P) of the model in float64 and in long double"""
    out = {}
    for ft in (np.float64, LD):
        out[ft] = R.nccf(R.decimate(x, hz, ft), o, T, ft, energy=True)
    return out


CASES = [(16000, "kaldi", 11, 16000), (44100, "snip", 12, 30000), (8000, "kaldi", 13, 9000), (48000, "snip", 14, 40000)]
_measured = {}


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request):
    hz, grid, seed, n = request.param
    x = R.test_signal(seed, hz, n)
    o = J.pitch(grid=grid, f64=True, raw_log=True)
    rows, idx, Q, P = J.pitch_host(x, hz, o, grid=True)
    return dict(hz=hz, x=x, o=o, rows=rows, idx=idx, Q=Q, P=P, m=model(x, hz, o, rows.shape[0]))


def held(name, got, f64, ref):
    """max |got - ref| <= GATE max |f64 - ref|: the ratio, printed before it is asserted"""
    e, e64 = float(np.abs(got.astype(LD) - ref).max()), float(np.abs(f64.astype(LD) - ref).max())
    print(f"{name}: rule {e:.3e}  float64 model {e64:.3e}  ratio {e / e64 if e64 else float('inf'):.3f}")
    assert e <= GATE * e64, (name, e, e64)


def test_grid_values_against_long_double(case):
    (Q64, P64, _), (Qld, Pld, e0) = case["m"][np.float64], case["m"][LD]
    assert case["Q"].shape == Qld.shape and case["rows"].shape[0] > 50
    held(f"Q {case['hz']}", case["Q"], Q64, Qld)
    # p carries no ballast: over the silent stretch it is 0 / 0 in exact arithmetic and a quotient of rounding residues
    # in any other, so its error there is of order 1 in every precision: that figure is printed, not asserted.  The
    # frames whose energy the reference puts within 10^-12 of the loudest frame's are held
    print(f"p {case['hz']}, all frames: rule {float(np.abs(case['P'].astype(LD) - Pld).max()):.3e}  "
          f"float64 model {float(np.abs(P64.astype(LD) - Pld).max()):.3e}")
    well = e0 > LD(1e-12) * e0.max()
    assert well.size // 2 <= well.sum() < well.size
    held(f"p {case['hz']}, well-conditioned frames", case["P"][well], P64[well], Pld[well])


def test_path_cost_against_long_double(case):
    o, Qld = case["o"], case["m"][LD][0]
    local = R.local_costs(Qld, o, LD)
    best = R.viterbi(local, o, LD)
    T = best.size
    got, want = R.path_cost(local, case["idx"], o), R.path_cost(local, best, o)
    print(f"path cost {case['hz']}: rule {float(got):.15g}  optimum {float(want):.15g}  diff {float(got - want):.3e}"
          f"  gate {1e-10 * T:.1e}")
    assert abs(got - want) <= LD(1e-10) * T


def test_columns_against_long_double(case):
    o, idx = case["o"], case["idx"]
    T = idx.size
    assert np.array_equal(case["rows"][:, 3], np.log(LD(1) / R.lags(o)).astype(np.float64)[idx])
    # Step 6 on its own: the model is given the rule's lag indices and its p at them.  p itself is held by the grid
    # test above; over the silent stretch it is a quotient of rounding residues (p carries no ballast), which no
    # precision reproduces, so the columns are not asked to
    p = case["P"][np.arange(T), idx]
    ref, c64 = R.columns(idx, p.astype(LD), o, LD), R.columns(idx, p, o, np.float64)
    for c in range(3):
        held(f"column {c + 1} {case['hz']}", case["rows"][:, c], c64[:, c], ref[:, c])
    raw, ridx = J.pitch_host(case["x"], case["hz"], J.pitch(grid=o.grid, f64=True, raw=True))
    assert np.array_equal(ridx, idx) and np.array_equal(raw[:, 0], case["P"][np.arange(T), idx])
    assert np.array_equal(raw[:, 1], (LD(1) / R.lags(o)).astype(np.float64)[idx])
    f32, _ = J.pitch_host(case["x"], case["hz"], J.pitch(grid=o.grid))
    assert f32.dtype == np.float32 and np.array_equal(f32, case["rows"][:, :3].astype(np.float32))


@pytest.mark.parametrize("hz,grid", [(16000, "kaldi"), (44100, "snip")])
def test_columns_from_the_models_own_p(hz, grid):
    """Steps 1 to 4 feeding step 6: on a signal without a silent stretch the model is given the rule's lag indices
    alone and forms p itself, in float64 and in long double"""
    rng = np.random.default_rng(31)
    n = hz
    t = np.arange(n) / hz
    phase = 2 * np.pi * np.cumsum(110.0 + 90.0 * t) / hz
    x = 4000 * sum(np.cos(k * phase + k) / k for k in range(1, 6)) + 300 * rng.standard_normal(n) + 150.0
    o = J.pitch(grid=grid, f64=True, raw_log=True)
    rows, idx = J.pitch_host(x, hz, o)
    T = idx.size
    pld = R.nccf(R.decimate(x, hz, LD), o, T, LD)[1][np.arange(T), idx]
    p64 = R.nccf(R.decimate(x, hz, np.float64), o, T, np.float64)[1][np.arange(T), idx]
    ref, c64 = R.columns(idx, pld, o, LD), R.columns(idx, p64, o, np.float64)
    for c in range(3):
        held(f"own p, column {c + 1} {hz}", rows[:, c], c64[:, c], ref[:, c])


@pytest.mark.parametrize("grid", ["snip", "kaldi"])
@pytest.mark.parametrize("f0", [62.5, 100.0, 160.0, 250.0])
def test_known_answer(f0, grid):
    t = np.arange(16000) / 16000
    x = 3000 * sum(np.cos(2 * np.pi * k * f0 * t + k) for k in range(1, 64) if k * f0 < 900)
    raw, _ = J.pitch_host(x, 16000, J.pitch(grid=grid, raw=True, f64=True))
    mid = raw[3:-3]
    ratio = np.maximum(mid[:, 1] / f0, f0 / mid[:, 1]).max()
    print(f"f0 {f0} {grid}: pitch within {ratio:.4f}, p >= {mid[:, 0].min():.4f}")
    assert mid.shape[0] > 80 and ratio <= 1.005 ** 2 and mid[:, 0].min() >= 0.95


def test_all_zero_unit():
    o = J.pitch(f64=True, raw=True)
    raw, idx, Q, P = J.pitch_host(np.zeros(8000), 16000, o, grid=True)
    assert raw.shape[0] == 50 and not Q.any() and not P.any() and not idx.any()
    assert not raw[:, 0].any() and np.all(raw[:, 1] == 400.0)
    assert not np.signbit(Q).any() and not np.signbit(P).any()


@pytest.mark.parametrize("T", [0, 1, 2, 75, 76, 151, 152])
def test_frame_counts_at_the_window_edges(T):
    hz, o = 8000, J.pitch(grid="kaldi", f64=True, raw_log=True)
    n = T * 80
    x = R.test_signal(20 + T, hz, n)
    rows, idx, Q, P = J.pitch_host(x, hz, o, grid=True)
    assert rows.shape == (T, 4)
    if T == 0:
        return
    p = P[np.arange(T), idx]
    ref, c64 = R.columns(idx, p.astype(LD), o, LD), R.columns(idx, p, o, np.float64)
    for c in range(3):
        held(f"T {T} column {c + 1}", rows[:, c], c64[:, c], ref[:, c])
    if T == 1:
        assert rows[0, 1] == 0.0 and rows[0, 2] == 0.0


@pytest.mark.parametrize("kw,S", [(dict(min_f0=399.0, max_f0=400.0, delta_pitch=0.002), 2),
                                  (dict(min_f0=50.0, max_f0=400.0, delta_pitch=0.002034), 1024)])
def test_smallest_and_largest_lag_grids(kw, S):
    o = J.pitch(f64=True, raw=True, **kw)
    assert J.pitch_geometry(o, 16000, 0).S == S == J.pitch_lags(o).size == R.lags(o).size
    x = R.test_signal(5, 16000, 4800)
    raw, idx, Q, P = J.pitch_host(x, 16000, o, grid=True)
    assert Q.shape == (30, S) and idx.max() < S
    Qld, Pld = R.nccf(R.decimate(x, 16000, LD), o, 30, LD)
    Q64, P64 = R.nccf(R.decimate(x, 16000, np.float64), o, 30, np.float64)
    held(f"Q S={S}", Q, Q64, Qld)
    local = R.local_costs(Qld, o, LD)
    got, want = R.path_cost(local, idx, o), R.path_cost(local, R.viterbi(local, o, LD), o)
    assert abs(got - want) <= LD(1e-10) * 30
