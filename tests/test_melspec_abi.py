"""Mel spectrograms on the host, without a GPU (jbonsai_amd/csrc/jb_melspec.cpp): the options' layout, every refusal
naming its field, the frame count of the three padding modes, the window and the mel weights against the long double
formulas (tests/melspec_ref.py), the host form of the rule -- the mixed-radix transform the kernel shares -- under the
precision gates, the framing against torch.stft, Whisper's preset against a float64 restatement of Whisper's published
steps, and the range clamp and the affine step as exact properties.

The gates (tests/melspec_ref.py): with E_ld the long double model and wmax the largest filter weight,
e(X) = max |E_X - E_ld| / (wmax sum_k S_ld) per frame;
  linear, f64:  e(host) <= 8 e(model_f64), model_f64 being numpy's own rfft in float64 on the same frames;
  log, f64:     |y - f(E_ld)| <= 8 e(model_f64) f'(E_ld) wmax sum_k S_ld + half an f64 ulp of f(E_ld);
  log, f32:     the same with one f32 ulp of the reference value.
Measured on the host over the ten shapes (reflect padding, power): e(model_f64) 1.5e-16 .. 3.4e-16, e(host) / e(model_f64)
0.66 .. 1.92, the smallest share of a filter in its frame 3.6e-8; the other padding modes and the magnitude spectrum
stay within 0.48 .. 1.72."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi
from tests import melspec_ref as R

ROOT = Path(__file__).resolve().parent.parent
INVALID, BUFFER = -1, -8
LD = np.longdouble


def test_opts_layout(tmp_path):
    fields = ("n_fft", "win_length", "hop_length", "n_mels", "f_min_hz", "f_max_hz", "floor", "range", "offset", "scale",
              "mel_scale", "norm", "pad", "log", "flags", "reserved")
    consts = ("JB_MEL_HTK", "JB_MEL_SLANEY", "JB_MEL_NORM_NONE", "JB_MEL_NORM_SLANEY", "JB_MEL_PAD_REFLECT",
              "JB_MEL_PAD_ZERO", "JB_MEL_PAD_NONE", "JB_MEL_LOG_NONE", "JB_MEL_LOG_LN", "JB_MEL_LOG_LOG10", "JB_MEL_LOG_DB",
              "JB_MEL_MAGNITUDE", "JB_MEL_DROP_LAST", "JB_MEL_F64")
    src = tmp_path / "lay.c"
    src.write_text('#include "jbonsai_amd.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){'
                   'printf("%zu\\n", sizeof(jb_melspec_opts));' +
                   "".join(f'printf("%zu\\n", offsetof(jb_melspec_opts, {f}));' for f in fields) +
                   "".join(f'printf("%u\\n", {c});' for c in consts) + "return 0;}\n")
    want = [96, 0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76, 80, 84, 0, 1, 0, 1, 0, 1, 2, 0, 1, 2, 3, 1, 2, 4]
    for cc, std, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        exe = tmp_path / ("lay_" + cc.replace("+", "p"))
        subprocess.run([cc, std, "-x", lang, "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
        got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
        assert got == want
    assert C.sizeof(_ffi.MelspecOpts) == 96
    assert [getattr(_ffi.MelspecOpts, f).offset for f in fields] == want[1:17]
    assert (J.MEL_HTK, J.MEL_SLANEY, J.MEL_NORM_NONE, J.MEL_NORM_SLANEY, J.MEL_PAD_REFLECT, J.MEL_PAD_ZERO,
            J.MEL_PAD_NONE, J.MEL_LOG_NONE, J.MEL_LOG_LN, J.MEL_LOG_LOG10, J.MEL_LOG_DB, J.MEL_MAGNITUDE,
            J.MEL_DROP_LAST, J.MEL_F64) == tuple(want[17:])


def _refused(hz, field, **kw):
    o = J.melspec(**{**dict(n_fft=400, hop=160), **kw})
    L = J.lib()
    assert L.jb_melspec_geometry(hz, C.byref(o), 1000, None, None, None, None, None) == INVALID, kw
    assert field in L.jb_last_error().decode(), (field, L.jb_last_error())
    x = np.zeros(1000)
    out = np.zeros(1 << 16, dtype=np.uint8)
    assert L.jb_melspec_host(x.ctypes.data, 1000, hz, C.byref(o), out.ctypes.data, out.size) == INVALID
    assert field in L.jb_last_error().decode()


def test_every_refusal_names_its_field():
    _refused(16000, "n_fft", n_fft=402)    # 2 * 3 * 67
    _refused(16000, "n_fft", n_fft=66)     # 2 * 3 * 11
    _refused(16000, "n_fft", n_fft=63)     # odd, and below 64
    _refused(16000, "n_fft", n_fft=75)     # odd
    _refused(16000, "n_fft", n_fft=4098)   # above 4096 (and 2 * 3 * 683)
    _refused(16000, "n_fft", n_fft=4500)   # 5-smooth, above 4096
    _refused(16000, "n_fft", n_fft=60)     # 5-smooth, below 64
    _refused(16000, "win_length", win=401)  # W > N
    _refused(16000, "win_length", win=1)
    _refused(16000, "hop_length", hop=0)
    _refused(16000, "n_mels", n_mels=0)
    _refused(16000, "n_mels", n_mels=129)
    _refused(16000, "f_min_hz", f_min=-1.0)
    _refused(16000, "f_min_hz", f_min=4000.0, f_max=4000.0)
    _refused(16000, "f_min_hz", f_min=8000.0)  # against the default f_max = hz / 2
    _refused(16000, "f_max_hz", f_max=8000.5)
    _refused(16000, "f_max_hz", f_max=float("nan"))
    _refused(16000, "floor", floor=-1.0)
    _refused(16000, "floor", floor=float("inf"))
    _refused(16000, "range", range=-1.0)
    _refused(16000, "range", range=float("nan"))
    _refused(16000, "offset", offset=float("inf"))
    _refused(16000, "scale", scale=float("nan"))
    _refused(16000, "mel_scale", mel_scale=2)
    _refused(16000, "norm", norm=2)
    _refused(16000, "pad", pad=3)
    _refused(16000, "log", log=4)
    _refused(16000, "flags", pad="none", drop_last=True)
    _refused(0, "rate")
    L = J.lib()
    o = J.melspec(n_fft=400, hop=160)
    o.flags = 8
    assert L.jb_melspec_geometry(16000, C.byref(o), 0, None, None, None, None, None) == INVALID
    assert "flags" in L.jb_last_error().decode()
    for word in range(3):
        o = J.melspec(n_fft=400, hop=160)
        o.reserved[word] = 1
        assert L.jb_melspec_geometry(16000, C.byref(o), 0, None, None, None, None, None) == INVALID
        assert "reserved" in L.jb_last_error().decode()
    assert L.jb_melspec_geometry(16000, None, 0, None, None, None, None, None) == INVALID
    assert L.jb_melspec_whisper(80, None) == INVALID
    w = J.MelspecOpts()
    assert L.jb_melspec_whisper(129, C.byref(w)) == INVALID and "n_mels" in L.jb_last_error().decode()
    o = J.melspec(n_fft=400, hop=160)
    assert L.jb_melspec_geometry(16000, C.byref(o), 0, None, None, None, None, None) == 0  # every out pointer may be null
    # the limits themselves pass
    assert J.melspec_geometry(16000, J.melspec(n_fft=64, win=2, hop=1, n_mels=128, f_max=8000.0))[:3] == (64, 2, 1)
    assert J.melspec_geometry(16000, J.melspec(n_fft=4096, hop=1 << 31, n_mels=1))[:3] == (4096, 4096, 1 << 31)
    for n_fft in (400, 480, 600, 800, 1024, 1200, 2048, 4000, 3888, 4050):
        assert J.melspec_geometry(48000, J.melspec(n_fft=n_fft, hop=7))[0] == n_fft
    # short buffers
    buf = np.zeros(80 * 201)
    assert L.jb_melspec_window(16000, C.byref(o), buf.ctypes.data, 399) == BUFFER
    assert L.jb_melspec_filterbank(16000, C.byref(o), buf.ctypes.data, 80 * 201 - 1) == BUFFER
    x = np.zeros(400)
    assert L.jb_melspec_host(x.ctypes.data, 400, 16000, C.byref(o), buf.ctypes.data, 3 * 80 * 4 - 1) == BUFFER


def test_python_converts_milliseconds():
    o = J.melspec(win_ms=25, hop_ms=10, rate=16000, n_mels=40)
    assert (o.n_fft, o.win_length, o.hop_length) == (400, 400, 160)
    o = J.melspec(n_fft=512, win_ms=25, hop_ms=10, rate=22050)
    assert (o.n_fft, o.win_length, o.hop_length) == (512, 551, 221)  # 551.25 and 220.5 samples
    # n_fft 0 with a window in milliseconds: the smallest even 5-smooth length of at least 64 that holds it
    got = [(J.melspec(win_ms=25, hop_ms=10, rate=hz).n_fft, J.melspec(win_ms=25, hop_ms=10, rate=hz).win_length)
           for hz in (8000, 22050, 44100, 48000)]
    assert got == [(200, 200), (576, 551), (1152, 1103), (1200, 1200)]  # 576 = 2^6 3^2, 1152 = 2^7 3^2
    assert J.melspec(win_ms=1, hop_ms=1, rate=8000).n_fft == 64
    for hz in (8000, 22050, 44100, 48000):  # (the stage takes them)
        o = J.melspec(win_ms=25, hop_ms=10, rate=hz)
        assert J.melspec_geometry(hz, o, hz)[:4] == (o.n_fft, o.win_length, o.hop_length, 1 + hz // o.hop_length)
    with pytest.raises(ValueError):
        J.melspec(win_ms=25, hop_ms=10)


def test_frame_counts():
    """T of the three padding modes and drop-last, around every edge: n = N / 2 (no frame under reflection, which needs
    n > N / 2), N / 2 + 1, n < H, whole hops."""
    N, H = 400, 160
    for pad, name in ((R.REFLECT, "reflect"), (R.ZERO, "zero"), (R.NONE, "none")):
        for drop in (False, True) if pad != R.NONE else (False,):
            for f64 in (False, True):
                o = J.melspec(n_fft=N, hop=H, n_mels=40, pad=name, drop_last=drop, f64=f64)
                for n in (0, 1, H - 1, H, N // 2 - 1, N // 2, N // 2 + 1, N - 1, N, N + H - 1, N + H, 10 * H + N + 7):
                    T = R.n_frames(n, N, H, pad, drop)
                    assert J.melspec_geometry(16000, o, n)[3:] == (T, T * 40 * (8 if f64 else 4)), (name, drop, n)
                    assert J.melspec_host(np.ones(n), 16000, o).shape == (T, 40)
    # T spelt out
    ns = (0, 1, 159, 160, 199, 200, 201, 320, 400, 559, 560)
    assert [R.n_frames(n, N, H, R.REFLECT) for n in ns] == [0, 0, 0, 0, 0, 0, 2, 3, 3, 4, 4]
    assert [R.n_frames(n, N, H, R.REFLECT, True) for n in ns] == [0, 0, 0, 0, 0, 0, 1, 2, 2, 3, 3]
    assert [R.n_frames(n, N, H, R.ZERO) for n in ns] == [1, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4]
    assert [R.n_frames(n, N, H, R.ZERO, True) for n in ns] == [0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3]
    assert [R.n_frames(n, N, H, R.NONE) for n in ns] == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2]
    # a hop longer than the unit
    assert J.melspec_geometry(16000, J.melspec(n_fft=64, hop=1000), 40)[3] == 1
    assert J.melspec_geometry(16000, J.melspec(n_fft=64, hop=1000, drop_last=True), 40)[3] == 0


@pytest.mark.parametrize("shape", R.SHAPES)
def test_window_and_filterbank_are_the_long_double_formulas(shape):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    hz, N, W, H, n_mels, slaney = shape
    w = J.melspec_window(hz, R.opts_of(shape))
    ref = R.window_ld(N, W).astype(np.float64)
    assert w.shape == (N,) and np.all(np.abs(w - ref) <= np.spacing(np.abs(ref)))
    lo = (N - W) // 2
    assert np.all(w[:lo + 1] == 0.0) and np.all(w[lo + W:] == 0.0) and np.all(w[lo + 1:lo + W] > 0.0)
    for scale, norm, f_min, f_max in ((slaney, slaney, 0.0, 0.0), (not slaney, False, 20.0, hz / 2 - 100.0),
                                      (True, False, 0.0, 0.0), (False, True, 50.0, 0.0)):
        o = J.melspec(n_fft=N, win=W, hop=H, n_mels=n_mels, mel_scale=int(scale), norm=int(norm), f_min=f_min,
                      f_max=f_max)
        Wt = J.melspec_filterbank(hz, o)
        ref = R.filterbank_ld(hz, N, n_mels, scale, norm, f_min, f_max).astype(np.float64)
        assert Wt.shape == ref.shape == (n_mels, N // 2 + 1)
        # (a weight next to a triangle's foot is a small difference of frequencies: its last bits follow those of the
        # mel points, which the two sides round alike but for libm's own last bit)
        assert np.all(np.abs(Wt - ref) <= 4 * np.spacing(ref.max(axis=1))[:, None]), (scale, norm)
        assert Wt.min() >= 0.0 and (norm or Wt.max() <= 1.0)


def test_slaney_points():
    """The Slaney scale's fixed points: 1 kHz is mel 15, 6.4 kHz is mel 42; Whisper's 80 filters peak where librosa's
    do (the first at 25 Hz: bin 1 of 201 gets the first filter's top)."""
    o = J.whisper_mel(80)
    W = J.melspec_filterbank(16000, o)
    assert W.shape == (80, 201) and W[0, 0] == 0.0 and W[0, 1] > 0.0 and np.all(W.sum(axis=1) > 0)
    pts = R.hz_ld(R.mel_ld(np.array([0.0, 1000.0, 6400.0, 8000.0]), True), True)
    assert np.allclose(pts.astype(np.float64), [0.0, 1000.0, 6400.0, 8000.0], rtol=1e-15)
    assert float(R.mel_ld(1000.0, True)) == 15.0 and abs(float(R.mel_ld(6400.0, True)) - 42.0) < 1e-15


@pytest.mark.parametrize("shape", R.SHAPES)
def test_host_form_under_the_gates(shape):
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.melspec_host(x, shape[0], o), shape, "host")


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[5], R.SHAPES[6], R.SHAPES[7]])
@pytest.mark.parametrize("pad,magnitude", [(R.ZERO, False), (R.NONE, False), (R.REFLECT, True), (R.NONE, True)])
def test_host_form_under_the_gates_other_modes(shape, pad, magnitude):
    """The zero-padded and unpadded frames and the magnitude spectrum; check_gates asserts the gate's conditions for
    each of these cases too (they hold: the smallest share is 2.4e-8, unpadded with 128 filters)."""
    if not R.have_long_double():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here")
    R.check_gates(lambda x, o: J.melspec_host(x, shape[0], o), shape, "host", pad, magnitude)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[6], R.SHAPES[5]])
@pytest.mark.parametrize("magnitude", [False, True])
def test_framing_is_torch_stft(shape, magnitude):
    """torch.stft(center=True, pad_mode="reflect", win_length=W) in float64 on the CPU, through the stage's own
    filterbank: the frame count, the reflection and the window's place inside the frame are torch's.  Both sides are
    float64 transforms of the same frames, each within GATE e(model_f64) of the long double model (the host form: gated
    above; torch: an ordinary float64 FFT, as numpy's is), so they lie within twice that of one another."""
    import torch

    hz, N, W, H, n_mels, slaney = shape
    x, E_ld, total, wmax, e64 = R.gate_case(shape, R.REFLECT, magnitude)
    o = R.opts_of(shape, log="none", f64=True, magnitude=magnitude)
    E = J.melspec_host(x, hz, o)
    X = torch.stft(torch.from_numpy(x * 2.0 ** -15), n_fft=N, hop_length=H, win_length=W,
                   window=torch.hann_window(W, periodic=True, dtype=torch.float64), center=True, pad_mode="reflect",
                   return_complex=True).numpy().T
    S = np.abs(X) if magnitude else X.real ** 2 + X.imag ** 2
    ref = S @ J.melspec_filterbank(hz, o).T
    assert E.shape == ref.shape == (1 + x.size // H, n_mels)
    diff = np.max(np.abs(E - ref) / (float(wmax) * total.astype(np.float64)[:, None]))
    print(f"{shape} magnitude {magnitude}: host against torch.stft {diff:.2e}, bound {2 * R.GATE * e64:.2e}")
    assert diff <= 2 * R.GATE * e64


def _whisper_restated(audio, n_mels):
    """Whisper's log_mel_spectrogram (openai/whisper, audio.py) in numpy float64: librosa's Slaney mel filters of
    sr 16000, n_fft 400; a centred, reflected STFT under a periodic Hann window; the last frame dropped; log10 clamped
    at 1e-10 and at the maximum minus 8; (y + 4) / 4.  Returns [T, n_mels]."""
    sr, n_fft, hop = 16000, 400, 160

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3))

    def mel_to_hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)

    fftfreqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    filters = np.zeros((n_mels, fftfreqs.size))
    for i in range(n_mels):
        filters[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    filters *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    window = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    padded = np.pad(audio, n_fft // 2, mode="reflect")
    T = 1 + audio.size // hop
    frames = padded[np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]] * window
    magnitudes = np.abs(np.fft.rfft(frames, axis=1))[:-1] ** 2
    mel_spec = magnitudes @ filters.T
    log_spec = np.log10(np.maximum(mel_spec, 1e-10))
    log_spec = np.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0, mel_spec


@pytest.mark.parametrize("n_mels", [80, 128])
def test_whisper_preset_is_whispers_front_end(n_mels):
    """The preset against the restatement on three signals: the gate signal (nothing is clamped), the same with its
    second half 100 dB down (those frames sit at the maximum minus 8) and silence.  The bound is the log gate's: both
    sides are float64 transforms, each within GATE * 1e-15 of the exact E relative to wmax sum_k S (e(model_f64) < 1e-15
    is asserted by the gate tests), which the derivative of log10(E) / 4 turns into a bound per element; the bound of
    the largest element once more for the clamp level, and two f64 ulps of the value for the logarithm and the affine
    step."""
    o = J.whisper_mel(n_mels, f64=True)
    assert (o.n_fft, o.win_length, o.hop_length, o.n_mels) == (400, 400, 160, n_mels)
    assert (o.f_min_hz, o.f_max_hz, o.floor, o.range, o.offset, o.scale) == (0.0, 8000.0, 1e-10, 8.0, 4.0, 0.25)
    assert (o.mel_scale, o.norm, o.pad, o.log) == (J.MEL_SLANEY, J.MEL_NORM_SLANEY, J.MEL_PAD_REFLECT, J.MEL_LOG_LOG10)
    assert o.flags == J.MEL_DROP_LAST | J.MEL_F64 and J.whisper_mel(n_mels).flags == J.MEL_DROP_LAST
    loud = R.gate_signal(16000, 4000)
    half = loud.copy()
    half[2000:] = np.round(half[2000:] * 1e-5)  # a few counts of noise: 100 dB down, far under max - 8
    n_clamped = []
    for x in (loud, half, np.zeros(1000)):
        y = J.melspec_host(x, 16000, o)
        ref, mel_spec = _whisper_restated(x * 2.0 ** -15, n_mels)
        assert y.shape == ref.shape == (x.size // 160, n_mels)
        if not x.any():
            assert np.all(y == (-10.0 + 4.0) * 0.25) and np.all(ref == -1.5)
            continue
        W = J.melspec_filterbank(16000, o)
        frames = np.pad(x * 2.0 ** -15, 200, mode="reflect")[np.arange(y.shape[0])[:, None] * 160 + np.arange(400)]
        total = (np.abs(np.fft.rfft(frames * J.melspec_window(16000, o), axis=1)) ** 2).sum(axis=1)
        rel = 2 * R.GATE * 1e-15 * W.max() * total[:, None] / np.maximum(mel_spec, 1e-10)
        bound = 0.25 / np.log(10.0) * rel + 2 * np.spacing(np.abs(ref) + 2.5)
        bound = bound + bound.flat[np.argmax(ref)]
        n_clamped.append(int(np.sum(ref == ref.max() - 8.0 / 4.0)))
        print(f"whisper {n_mels}: max |y - ref| {np.max(np.abs(y - ref)):.2e}, clamped elements {n_clamped[-1]}")
        assert np.all(np.abs(y - ref) <= bound)
        assert int(np.sum(y == y.max() - 8.0 / 4.0)) == n_clamped[-1]
    assert n_clamped[0] == 0 and n_clamped[1] > n_mels


@pytest.mark.parametrize("log", ["log10", "db", "ln", "none"])
def test_range_and_affine_are_exact(log):
    """range = r gives max(y0, max(y0) - r) of the range = 0 f64 output bit for bit, then (y + offset) * scale as numpy
    computes it in f64, bit for bit; the f32 element is one rounding of that."""
    shape = R.SHAPES[0]
    x = R.gate_signal(16000, 3000)
    x[1500:] *= 1e-4
    y0 = J.melspec_host(x, 16000, R.opts_of(shape, log=log, f64=True))
    for r in (0.5, 3.0, 8.0, 80.0, 1e-3 * float(y0.max() - y0.min())):
        want = np.maximum(y0, y0.max() - r)
        assert np.array_equal(J.melspec_host(x, 16000, R.opts_of(shape, log=log, f64=True, range=r)), want)
        for offset, scale in ((4.0, 0.25), (-1.7, 3.3), (0.0, 0.0), (1e-3, -1.0)):
            out = (want + offset) * (scale or 1.0)
            kw = dict(log=log, range=r, offset=offset, scale=scale)
            assert np.array_equal(J.melspec_host(x, 16000, R.opts_of(shape, f64=True, **kw)), out)
            assert np.array_equal(J.melspec_host(x, 16000, R.opts_of(shape, **kw)), out.astype(np.float32))
    assert np.any(np.maximum(y0, y0.max() - 0.5) != y0)  # (the clamp bites)
    # without a range the affine step alone
    assert np.array_equal(J.melspec_host(x, 16000, R.opts_of(shape, log=log, f64=True, offset=4.0, scale=0.25)),
                          (y0 + 4.0) * 0.25)


def test_silence_and_the_floor():
    """A silent unit is exactly 0 in every filter, or the floor's logarithm; so is a silent frame of a unit that is not
    silent everywhere (pad none: no neighbour leaks in)."""
    shape = R.SHAPES[6]
    hz, N, W, H, n_mels, _ = shape
    x = np.zeros(10 * H + N)
    assert np.all(J.melspec_host(x, hz, R.opts_of(shape, log="none", f64=True)) == 0.0)
    assert np.all(J.melspec_host(x, hz, R.opts_of(shape, log="log10", f64=True)) == -10.0)
    assert np.all(J.melspec_host(x, hz, R.opts_of(shape, log="db", f64=True)) == -100.0)
    assert np.all(J.melspec_host(x, hz, R.opts_of(shape, log="ln", f64=True, floor=1e-3)) == float(np.log(LD(1e-3))))
    x[5 * H + N:] = R.gate_signal(hz, 5 * H)
    y = J.melspec_host(x, hz, R.opts_of(shape, log="db", f64=True, pad="none"))
    assert np.all(y[:6] == -100.0) and np.all(y[7:] > -100.0)
    # the clamp under a unit's maximum lifts the silent frames with it
    yr = J.melspec_host(x, hz, R.opts_of(shape, log="db", f64=True, pad="none", range=60.0))
    assert np.all(yr[:6] == y.max() - 60.0)


def test_frames_depend_on_their_own_samples_only():
    """Frame t of a long input equals frame 0 of its own window (pad none), bit for bit; reflect and zero padding are
    the unpadded frames of the explicitly padded signal."""
    shape = R.SHAPES[5]
    hz, N, W, H, n_mels, _ = shape
    x = R.gate_signal(hz, 9 * H + N)
    o = R.opts_of(shape, f64=True, pad="none")
    y = J.melspec_host(x, hz, o)
    assert y.shape[0] == 10
    for t in range(y.shape[0]):
        assert np.array_equal(J.melspec_host(x[t * H:t * H + N], hz, o)[0], y[t])
    for name in ("reflect", "zero"):
        yp = J.melspec_host(x, hz, R.opts_of(shape, f64=True, pad=name))
        padded = np.pad(x, N // 2, mode="reflect" if name == "reflect" else "constant")
        assert yp.shape[0] == 1 + x.size // H
        assert np.array_equal(yp, J.melspec_host(padded, hz, o)[:yp.shape[0]])
        yd = J.melspec_host(x, hz, R.opts_of(shape, f64=True, pad=name, drop_last=True))
        assert np.array_equal(yd, yp[:-1])
