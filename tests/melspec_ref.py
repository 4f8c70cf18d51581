"""The mel spectrogram rule of include/jbonsai_amd.h ("Mel spectrograms") restated twice in numpy, and the gates.

model_f64 follows the rule with numpy.fft.rfft in float64 (it takes any N); model_ld with a direct DFT, the window, the
filterbank and the sums in numpy.longdouble (a 64-bit mantissa on x86-64).  The tests hold the library to

    e(X) = max over t, m of |E_X - E_ld| / (wmax * sum_k S_ld[t][k])  <=  GATE * e(model_f64)

with wmax the largest filter weight, so that the area normalisation (weights of 1e-3 and below) does not slacken the
gate: the bound is the error of an ordinary float64 transform of the same frames, not a number picked by hand.  GATE is
the project's (tests/fbank_ref.py): a different radix schedule and summation order at the same precision.
"""
import functools

import numpy as np

from tests import fbank_ref

LD = np.longdouble
GATE = fbank_ref.GATE
REFLECT, ZERO, NONE = 0, 1, 2
# (hz, N, W, H, n_mels, Slaney scale and norm): Whisper's two, each radix alone (1024 = 2^10, 486 = 2 3^5, 250 = 2 5^3),
# mixed radices, a window shorter than the transform, the largest sizes (4000 = 2^5 5^3, 3888 = 2^4 3^5) and the smallest
SHAPES = ((16000, 400, 400, 160, 80, True), (16000, 400, 400, 160, 128, True), (48000, 1200, 1200, 480, 80, True),
          (22050, 1024, 1024, 256, 80, False), (8000, 64, 64, 16, 10, True), (24000, 486, 486, 120, 40, True),
          (16000, 250, 200, 80, 40, False), (48000, 4000, 2400, 480, 128, True), (48000, 3888, 3888, 960, 80, True),
          (16000, 96, 96, 40, 20, True))

have_long_double = fbank_ref.have_long_double


def n_frames(n, N, H, pad=REFLECT, drop_last=False):
    if pad == NONE:
        return 1 + (n - N) // H if n >= N else 0
    if pad == REFLECT and n <= N // 2:
        return 0
    return max(0, 1 + n // H - int(drop_last))


def window_ld(N, W=0):
    """[N]: the periodic Hann window of W points at (N - W) / 2, zeros around it."""
    W = W or N
    two_pi = 2 * np.arccos(LD(-1))
    w = np.zeros(N, dtype=LD)
    lo = (N - W) // 2
    w[lo:lo + W] = LD("0.5") - LD("0.5") * np.cos(two_pi * np.arange(W, dtype=LD) / LD(W))
    return w


_STEP = np.log(LD("6.4")) / LD(27)


def mel_ld(f, slaney):
    f = np.asarray(f, dtype=LD)
    if not slaney:
        return LD(2595) * np.log10(LD(1) + f / LD(700))
    return np.where(f < 1000, LD(3) * f / LD(200), LD(15) + np.log(np.maximum(f, LD(1)) / LD(1000)) / _STEP)


def hz_ld(m, slaney):
    m = np.asarray(m, dtype=LD)
    if not slaney:
        return LD(700) * (LD(10) ** (m / LD(2595)) - LD(1))
    return np.where(m < 15, LD(200) * m / LD(3), LD(1000) * np.exp((m - LD(15)) * _STEP))


def filterbank_ld(hz, N, n_mels, slaney=True, norm=None, f_min=0.0, f_max=0.0):
    """[n_mels, N / 2 + 1] in long double; norm None: Slaney's with the Slaney scale."""
    norm = slaney if norm is None else norm
    f_max = f_max or hz / 2
    lo, hi = mel_ld(f_min, slaney), mel_ld(f_max, slaney)
    f = hz_ld(lo + (hi - lo) * np.arange(n_mels + 2, dtype=LD) / LD(n_mels + 1), slaney)
    nu = np.arange(N // 2 + 1, dtype=LD) * LD(hz) / LD(N)
    W = np.zeros((n_mels, nu.size), dtype=LD)
    for m in range(n_mels):
        W[m] = np.maximum(LD(0), np.minimum((nu - f[m]) / (f[m + 1] - f[m]), (f[m + 2] - nu) / (f[m + 2] - f[m + 1])))
        if norm:
            W[m] *= LD(2) / (f[m + 2] - f[m])
    return W


def frames_of(x, N, H, pad, drop_last, dtype):
    """[T, N]: the frames of x * 2^-15 (exact in either type)."""
    x = np.asarray(x, dtype=dtype) * dtype(2.0 ** -15)
    T = n_frames(x.size, N, H, pad, drop_last)
    if T == 0:
        return np.zeros((0, N), dtype=dtype)
    if pad == REFLECT:
        xp = np.pad(x, N // 2, mode="reflect")
    elif pad == ZERO:
        xp = np.pad(x, N // 2)
    else:
        xp = x
    return xp[np.arange(T)[:, None] * H + np.arange(N)[None, :]]


@functools.lru_cache(maxsize=None)
def _dft_ld(N):
    two_pi = 2 * np.arccos(LD(-1))
    # (the angle reduced in integers first: j k mod N is exact)
    jk = (np.arange(N)[:, None] * np.arange(N // 2 + 1)[None, :]) % N
    ang = two_pi * jk.astype(LD) / LD(N)
    return np.cos(ang), -np.sin(ang)


def model_ld(x, hz, N, W, H, n_mels, slaney, pad=REFLECT, magnitude=False, drop_last=False):
    """(E [T, n_mels], sum_k S_k per frame [T], wmax) in long double."""
    fr = frames_of(x, N, H, pad, drop_last, LD) * window_ld(N, W)[None, :]
    c, s = _dft_ld(N)
    re, im = fr @ c, fr @ s
    S = re * re + im * im
    if magnitude:
        S = np.sqrt(S)
    Wt = filterbank_ld(hz, N, n_mels, slaney)
    return S @ Wt.T, S.sum(axis=1), Wt.max()


def model_f64(x, hz, N, W, H, n_mels, slaney, pad=REFLECT, magnitude=False, drop_last=False):
    """E [T, n_mels] in float64 through numpy.fft.rfft."""
    fr = frames_of(x, N, H, pad, drop_last, np.float64) * window_ld(N, W).astype(np.float64)[None, :]
    X = np.fft.rfft(fr, n=N, axis=1)
    S = X.real * X.real + X.imag * X.imag
    if magnitude:
        S = np.sqrt(S)
    return S @ filterbank_ld(hz, N, n_mels, slaney).astype(np.float64).T


def rel_err(E, E_ld, total, wmax):
    """e(X); frames without power (all zero) must be exactly zero and do not enter."""
    E = np.asarray(E, dtype=LD)
    live = total > 0
    assert np.all(E[~live] == 0)
    if not live.any():
        return 0.0
    return float(np.max(np.abs(E[live] - E_ld[live]) / (wmax * total[live, None])))


def gate_signal(hz, n, seed=20):
    """fbank_ref.gate_signal's tone plus noise -- 137 Hz at amplitude 8000 under a slow 3 Hz modulation, white noise of
    rms 300 -- without its silent head (that one is 60 ms long: more than the whole signal of the small shapes).  Every
    filter of every frame then carries a share of its frame's spectrum far above the rounding error."""
    t = np.arange(n, dtype=np.float64) / hz
    x = 8000.0 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * 137.0 * t)
    return x + np.random.default_rng(seed).normal(0.0, 300.0, n)


def gate_length(N, H):
    return 14 * H + N // 2 + 3


@functools.lru_cache(maxsize=None)
def gate_case(shape, pad=REFLECT, magnitude=False):
    """The gate signal of a shape, the long double model of it and e(model_f64); computed once per case and shared."""
    hz, N, W, H, n_mels, slaney = shape
    x = gate_signal(hz, gate_length(N, H))
    x.setflags(write=False)
    E_ld, total, wmax = model_ld(x, hz, N, W, H, n_mels, slaney, pad, magnitude)
    e64 = rel_err(model_f64(x, hz, N, W, H, n_mels, slaney, pad, magnitude), E_ld, total, wmax)
    return x, E_ld, total, wmax, e64


def opts_of(shape, **kw):
    import jbonsai_amd as J

    hz, N, W, H, n_mels, slaney = shape
    return J.melspec(n_fft=N, win=W, hop=H, n_mels=n_mels, mel_scale="slaney" if slaney else "htk",
                     norm="slaney" if slaney else "none", **kw)


_LOGS = (("ln", lambda e: np.log(e), LD(1)), ("log10", lambda e: np.log10(e), LD(1) / np.log(LD(10))),
         ("db", lambda e: LD(10) * np.log10(e), LD(10) / np.log(LD(10))))


def check_gates(run, shape, who, pad=REFLECT, magnitude=False, lines=None):
    """run(x, opts) -> [T, n_mels]: the linear gate in f64 and its f32 rounding; the three log gates, built as
    fbank_ref.check_gates builds them -- the linear bound through the logarithm's derivative, plus half an f64 ulp (f64
    elements) or one f32 ulp (f32 elements) of the reference value."""
    x, E_ld, total, wmax, e64 = gate_case(shape, pad, magnitude)
    kw = dict(pad=("reflect", "zero", "none")[pad], magnitude=magnitude)
    live = total > 0
    silent = ~live
    # the conditions the gate stands on: a float64 transform's error is there and small, every filter covers a bin and
    # carries, in every live frame, a share of the frame's spectrum far above the gate
    assert live.sum() >= 8 and 0 < e64 < 1e-15
    assert np.all(filterbank_ld(*shape[:2], shape[4], shape[5]).sum(axis=1) > 0)
    share = float(np.min(E_ld[live] / (wmax * total[live, None])))
    assert share > 2e-8
    E = run(x, opts_of(shape, log="none", f64=True, **kw))
    e = rel_err(E, E_ld, total, wmax)
    line = (f"{who} {shape} pad {kw['pad']} magnitude {magnitude}: e(model_f64) {e64:.2e}  e {e:.2e}  "
            f"ratio {e / e64:.2f}  smallest share {share:.1e}")
    print(line)
    if lines is not None:
        lines.append(line)
    assert E.dtype == np.float64 and E.shape == E_ld.shape and e <= GATE * e64
    E32 = run(x, opts_of(shape, log="none", **kw))
    assert E32.dtype == np.float32 and np.array_equal(E32, E.astype(np.float32))
    rel = GATE * e64 * (wmax * total[live, None] / E_ld[live])
    for name, fn, slope in _LOGS:
        ref = fn(E_ld[live])
        floor = float(fn(LD(1e-10)))
        y = run(x, opts_of(shape, log=name, f64=True, **kw))
        half_ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD) / 2
        assert np.all(y[silent] == floor)
        assert np.all(np.abs(y[live].astype(LD) - ref) <= rel * slope + half_ulp), name
        y32 = run(x, opts_of(shape, log=name, **kw))
        ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(LD)
        assert y32.dtype == np.float32 and np.all(y32[silent] == np.float32(floor))
        assert np.all(np.abs(y32[live].astype(LD) - ref) <= rel * slope + ulp), name
    # an explicit floor above every energy
    yf = run(x, opts_of(shape, log="ln", f64=True, floor=1e30, **kw))
    assert np.all(yf == float(np.log(LD(1e30))))
