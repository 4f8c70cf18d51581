"""Filterbank features on the host, without a GPU (jbonsai_amd/csrc/jb_fbank.cpp): the options' layout, the geometry
by rate, every refusal naming its field, the window and the mel weights against the reference's long double formulas
(tests/fbank_ref.py), and the host form of the rule under the precision gates.

The gates (tests/fbank_ref.py): with E_ld the long double model, e(X) = max |E_X - E_ld| / sum_k P_ld per frame;
  linear, f64:  e(host) <= 8 e(model_f64), model_f64 being numpy's own rfft in float64 on the same frames;
  log, f64:     |y - ln E_ld| <= 8 e(model_f64) sum_k P_ld / E_ld;
  log, f32:     the same plus one f32 ulp of the reference value.
The f64 log gate runs as stated with JB_FBANK_UNIT.  Its bound has no term for the rounding of the result itself: in
the 16-bit scale ln E lies in 16..32 for the loud filters of the gate signal, where half an ulp of f64 is 1.8e-15,
while the bound goes down to 1.1e-15 on the gate signal (Hamming, centre mode; 1.75e-15 with Hann) -- even ln E_ld
rounded correctly to f64 misses it there (by up to 1.55 times the bound at 48 and 8 kHz; the host form measured up to
1.10 at 8 kHz, 1.01 at 16 kHz).  With JB_FBANK_UNIT the same energies have |ln E| < 16, half an ulp is at most
8.9e-16, below the bound, and the gate tests what it is there for: the error of E under the logarithm.  The 16-bit
scale, what a caller gets by default, is gated in f64 too, with half an f64 ulp of the reference value added to the
bound -- the term the f32 gate carries for its own format -- and in f32."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import fbank_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, BUFFER = -1, -8
LD = np.longdouble


def test_opts_layout(tmp_path):
    fields = ("win_us", "hop_us", "n_fft", "n_mels", "f_min_hz", "f_max_hz", "log_floor", "window", "flags", "reserved")
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu\\n", sizeof(jb_fbank_opts));' +
                   "".join(f'printf("%zu\\n", offsetof(jb_fbank_opts, {f}));' for f in fields) +
                   'printf("%u %u %u %u %u %u\\n", JB_FBANK_HANN, JB_FBANK_HAMMING, JB_FBANK_CENTER, JB_FBANK_LINEAR, '
                   'JB_FBANK_UNIT, JB_FBANK_F64);return 0;}\n')
    want = [64, 0, 4, 8, 12, 16, 24, 32, 40, 44, 48, 0, 1, 1, 2, 4, 8]
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want
    assert C.sizeof(_ffi.FbankOpts) == 64
    assert [getattr(_ffi.FbankOpts, f).offset for f in fields] == want[1:11]
    assert (J.FBANK_HANN, J.FBANK_HAMMING, J.FBANK_CENTER, J.FBANK_LINEAR, J.FBANK_UNIT, J.FBANK_F64) == tuple(want[11:])


@pytest.mark.parametrize("hz,wl,hop,n_fft", [(8000, 200, 80, 256), (16000, 400, 160, 512), (22050, 551, 221, 1024),
                                             (48000, 1200, 480, 2048)])
def test_geometry_by_rate(hz, wl, hop, n_fft):
    o = J.fbank()
    assert J.fbank_geometry(hz, o)[:3] == (wl, hop, n_fft) == R.geometry(hz)
    assert J.fbank_geometry(hz, J.fbank(n_fft=4096))[:3] == (wl, hop, 4096)
    for center in (False, True):
        for f64 in (False, True):
            o = J.fbank(n_mels=40, center=center, f64=f64)
            for n in (0, 1, wl - 1, wl, wl + hop - 1, wl + hop, 10 * hop + wl + 7):
                T = R.n_frames(n, wl, hop, center)
                assert J.fbank_geometry(hz, o, n)[3:] == (T, T * 40 * (8 if f64 else 4)), (n, center)
    # T spelt out: snip mode counts whole windows, centre mode every started hop
    assert [R.n_frames(n, wl, hop, False) for n in (0, 1, wl - 1, wl, wl + hop - 1, wl + hop)] == [0, 0, 0, 1, 1, 2]
    assert [R.n_frames(n, wl, hop, True) for n in (0, 1, hop, hop + 1)] == [0, 1, 1, 2]


def _refused(hz, field, **kw):
    o = J.fbank(**kw)
    L = J.lib()
    assert L.jb_fbank_geometry(hz, C.byref(o), 100, None, None, None, None, None) == INVALID, kw
    assert field in L.jb_last_error().decode(), (field, L.jb_last_error())
    x = np.zeros(100)
    out = np.zeros(1 << 16, dtype=np.uint8)
    assert L.jb_fbank_host(x.ctypes.data, 100, hz, C.byref(o), out.ctypes.data, out.size) == INVALID
    assert field in L.jb_last_error().decode()


def test_every_refusal_names_its_field():
    _refused(16000, "win_us", win_ms=0.05)           # wl = 1
    _refused(16000, "win_us", win_ms=300)            # wl = 4800 above 4096
    _refused(16000, "win_us", win_ms=25, n_fft=256)  # wl = 400 above n_fft
    _refused(16000, "hop_us", hop_ms=0.02)           # hop = 0
    _refused(16000, "n_fft", n_fft=500)
    _refused(16000, "n_fft", n_fft=32)
    _refused(16000, "n_fft", n_fft=8192)
    _refused(16000, "n_fft", win_ms=1)               # wl = 16: the smallest power of two is below 64
    _refused(16000, "n_mels", n_mels=0)
    _refused(16000, "n_mels", n_mels=129)
    _refused(16000, "f_min_hz", f_min=-1.0)
    _refused(16000, "f_min_hz", f_min=4000.0, f_max=4000.0)
    _refused(16000, "f_min_hz", f_min=8000.0)        # against the default f_max = hz / 2
    _refused(16000, "f_max_hz", f_max=8000.5)
    _refused(16000, "f_max_hz", f_max=float("nan"))
    _refused(16000, "log_floor", log_floor=-1.0)
    _refused(16000, "log_floor", log_floor=float("inf"))
    _refused(16000, "window", window=2)
    L = J.lib()
    o = J.fbank()
    o.flags = 16
    assert L.jb_fbank_geometry(16000, C.byref(o), 0, None, None, None, None, None) == INVALID
    assert "flags" in L.jb_last_error().decode()
    for word in range(4):
        o = J.fbank()
        o.reserved[word] = 1
        assert L.jb_fbank_geometry(16000, C.byref(o), 0, None, None, None, None, None) == INVALID
        assert "reserved" in L.jb_last_error().decode()
    assert L.jb_fbank_geometry(16000, None, 0, None, None, None, None, None) == INVALID
    o = J.fbank()
    assert L.jb_fbank_geometry(16000, C.byref(o), 0, None, None, None, None, None) == 0  # every out pointer may be null
    # the limits themselves pass
    assert J.fbank_geometry(16000, J.fbank(win_ms=0.125, n_fft=64, hop_ms=0.0625, n_mels=128, f_max=8000.0))[:3] == (2, 1, 64)
    assert J.fbank_geometry(16000, J.fbank(win_ms=256, n_mels=1))[:3] == (4096, 160, 4096)
    # short buffers
    w = np.zeros(400)
    assert L.jb_fbank_window(16000, C.byref(o), w.ctypes.data, 399) == BUFFER
    assert L.jb_fbank_filterbank(16000, C.byref(o), w.ctypes.data, 400) == BUFFER
    x = np.zeros(400)
    assert L.jb_fbank_host(x.ctypes.data, 400, 16000, C.byref(o), w.ctypes.data, 80 * 4 - 1) == BUFFER


@pytest.mark.parametrize("hz", [8000, 16000, 22050, 48000])
def test_window_and_filterbank_are_the_long_double_formulas(hz):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    wl, _, n_fft = R.geometry(hz)
    for kind, name in ((R.HANN, "hann"), (R.HAMMING, "hamming")):
        w = J.fbank_window(hz, J.fbank(window=name))
        ref = R.window_ld(kind, wl)
        assert w.shape == (wl,) and np.all(np.abs(w - ref.astype(np.float64)) <= np.spacing(np.abs(w)))
    assert J.fbank_window(hz, J.fbank())[0] == 0.0 and J.fbank_window(hz, J.fbank(window="hamming"))[0] == pytest.approx(0.08)
    for n_mels, f_min, f_max in ((80, 0.0, 0.0), (23, 20.0, hz / 2 - 100.0), (128, 0.0, 0.0), (1, 0.0, 0.0)):
        W = J.fbank_filterbank(hz, J.fbank(n_mels=n_mels, f_min=f_min, f_max=f_max))
        ref = R.filterbank_ld(hz, n_fft, n_mels, f_min, f_max)
        assert W.shape == ref.shape == (n_mels, n_fft // 2 + 1)
        assert np.array_equal(W > 0, ref.astype(np.float64) > 0)
        assert np.all(np.abs(W - ref.astype(np.float64)) <= np.spacing(W)), (n_mels, f_min)
        assert W.min() >= 0.0 and W.max() <= 1.0


@pytest.mark.parametrize("hz,n_mels,n_fft", R.SHAPES)
@pytest.mark.parametrize("window", [R.HANN, R.HAMMING])
@pytest.mark.parametrize("center", [False, True])
def test_host_form_under_the_gates(hz, n_mels, n_fft, window, center):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.fbank_host(x, hz, o), hz, n_mels, window, center, "host", n_fft)


@pytest.mark.parametrize("hz,n_mels", [(16000, 80), (48000, 80), (8000, 23)])
def test_unit_impulse_gives_the_filters_sums(hz, n_mels):
    """x = 1 at the frame's first sample: X_k = w_0 for every k, so E_m = w_0^2 sum_k W[m][k] (Hamming: w_0 = 0.08;
    the periodic Hann window starts at 0)."""
    wl, hop, n_fft = R.geometry(hz)
    x = np.zeros(wl)
    x[0] = 1.0
    o = J.fbank(n_mels=n_mels, window="hamming", linear=True, f64=True)
    E = J.fbank_host(x, hz, o)
    w0 = J.fbank_window(hz, o)[0]
    want = w0 * w0 * J.fbank_filterbank(hz, o).sum(axis=1)
    assert E.shape == (1, n_mels) and np.allclose(E[0], want, rtol=1e-14, atol=0)
    assert np.all(J.fbank_host(x, hz, J.fbank(n_mels=n_mels, linear=True, f64=True)) == 0.0)


def test_a_filter_without_bins_yields_zero_and_the_floor():
    """128 filters on the 33 bins of n_fft = 64 at 8 kHz: the narrow low filters fall between two bins."""
    o = J.fbank(win_ms=8, hop_ms=4, n_mels=128, linear=True, f64=True)
    assert J.fbank_geometry(8000, o)[:3] == (64, 32, 64)
    W = J.fbank_filterbank(8000, o)
    empty = W.sum(axis=1) == 0
    assert 0 < empty.sum() < 128
    x = np.random.default_rng(5).normal(0, 3000, 400)
    E = J.fbank_host(x, 8000, o)
    assert np.all(E[:, empty] == 0.0) and np.all(E[:, ~empty] > 0.0)
    y = J.fbank_host(x, 8000, J.fbank(win_ms=8, hop_ms=4, n_mels=128, f64=True, log_floor=1e-3))
    assert np.all(y[:, empty] == float(np.log(LD(1e-3)))) and np.all(y[:, ~empty] > np.log(1e-3))


def test_frames_depend_on_their_own_samples_only():
    """Frame t of a long input equals frame 0 of its own window, bit for bit, and in centre mode the zero padding is
    explicit zeros."""
    hz, (wl, hop, _) = 16000, R.geometry(16000)
    x = R.gate_signal(hz, 9 * hop + wl)[6 * hop:]
    o = J.fbank(f64=True)
    y = J.fbank_host(x, hz, o)
    for t in range(y.shape[0]):
        assert np.array_equal(J.fbank_host(x[t * hop:t * hop + wl], hz, o)[0], y[t])
    oc = J.fbank(f64=True, center=True)
    yc = J.fbank_host(x, hz, oc)
    padded = np.concatenate([np.zeros(wl // 2), x, np.zeros(wl)])
    assert yc.shape[0] == -(-x.size // hop)
    assert np.array_equal(yc, J.fbank_host(padded, hz, o)[:yc.shape[0]])
