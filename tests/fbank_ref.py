"""The filterbank rule of include/jbonsai_amd.h ("Filterbank features") restated twice in numpy, and the gate signal.

model_f64 follows the rule with numpy.fft.rfft in float64; model_ld with a direct DFT, the window, the filterbank and
the sums in numpy.longdouble (a 64-bit mantissa on x86-64).  The tests hold the library to

    e(X) = max over t, m of |E_X - E_ld| / sum_k P_ld[t][k]  <=  GATE * e(model_f64)

so the bound is the error of an ordinary float64 transform of the same frames, not a number picked by hand.
"""
import functools

import numpy as np

LD = np.longdouble
GATE = 8.0  # a different radix schedule and summation order at the same precision: a small factor, not orders
HANN, HAMMING = 0, 1
# (rate, filters, forced n_fft) of the gate: n_fft 256, 512, 1024, 2048 by the rate, 4096 forced, and one filter alone
SHAPES = ((8000, 23, 0), (16000, 80, 0), (22050, 128, 0), (48000, 80, 0), (48000, 80, 4096), (16000, 1, 0))


def have_long_double():
    return np.finfo(LD).eps < 2e-19


def geometry(hz, win_us=25000, hop_us=10000, n_fft=0):
    wl = (hz * win_us + 500000) // 1000000
    hop = (hz * hop_us + 500000) // 1000000
    if not n_fft:
        n_fft = 1
        while n_fft < wl:
            n_fft *= 2
    return wl, hop, n_fft


def n_frames(n, wl, hop, center):
    if center:
        return -(-n // hop)
    return 1 + (n - wl) // hop if n >= wl else 0


def window_ld(kind, wl):
    two_pi = 2 * np.arccos(LD(-1))
    j = np.arange(wl, dtype=LD)
    if kind == HAMMING:
        return LD("0.54") - LD("0.46") * np.cos(two_pi * j / LD(wl - 1))
    return LD("0.5") - LD("0.5") * np.cos(two_pi * j / LD(wl))


def mel_ld(f):
    return LD(1127) * np.log(LD(1) + np.asarray(f, dtype=LD) / LD(700))


def filterbank_ld(hz, n_fft, n_mels, f_min=0.0, f_max=0.0):
    """[n_mels, n_fft / 2 + 1] in long double."""
    f_max = f_max or hz / 2
    lo, hi = mel_ld(f_min), mel_ld(f_max)
    mu = mel_ld(np.arange(n_fft // 2 + 1, dtype=LD) * LD(hz) / LD(n_fft))
    W = np.zeros((n_mels, mu.size), dtype=LD)
    for m in range(n_mels):
        l, c, r = (lo + (hi - lo) * LD(m + i) / LD(n_mels + 1) for i in range(3))
        W[m] = np.maximum(LD(0), np.minimum((mu - l) / (c - l), (r - mu) / (r - c)))
    return W


def frames_of(x, wl, hop, center, dtype):
    """[T, wl]: the frames of x, zeros outside it."""
    x = np.asarray(x, dtype=dtype)
    T = n_frames(x.size, wl, hop, center)
    pad = wl // 2 if center else 0
    xp = np.concatenate([np.zeros(pad, dtype=dtype), x, np.zeros(wl + hop, dtype=dtype)])
    idx = np.arange(T)[:, None] * hop + np.arange(wl)[None, :]
    return xp[idx] if T else np.zeros((0, wl), dtype=dtype)


@functools.lru_cache(maxsize=None)
def _dft_ld(n_fft, wl):
    two_pi = 2 * np.arccos(LD(-1))
    # (the angle reduced in integers first: j k mod n_fft is exact)
    jk = (np.arange(wl)[:, None] * np.arange(n_fft // 2 + 1)[None, :]) % n_fft
    ang = two_pi * jk.astype(LD) / LD(n_fft)
    return np.cos(ang), -np.sin(ang)


def model_ld(x, hz, n_mels, window=HANN, center=False, unit=False, n_fft=0, f_min=0.0, f_max=0.0,
             win_us=25000, hop_us=10000):
    """(E [T, n_mels], total power per frame [T]) in long double."""
    wl, hop, n_fft = geometry(hz, win_us, hop_us, n_fft)
    fr = frames_of(x, wl, hop, center, LD)
    if unit:
        fr = fr * LD(2) ** -15
    fr = fr * window_ld(window, wl)[None, :]
    c, s = _dft_ld(n_fft, wl)
    re, im = fr @ c, fr @ s
    P = re * re + im * im
    return P @ filterbank_ld(hz, n_fft, n_mels, f_min, f_max).T, P.sum(axis=1)


def model_f64(x, hz, n_mels, window=HANN, center=False, unit=False, n_fft=0, f_min=0.0, f_max=0.0,
              win_us=25000, hop_us=10000):
    """E [T, n_mels] in float64 through numpy.fft.rfft."""
    wl, hop, n_fft = geometry(hz, win_us, hop_us, n_fft)
    fr = frames_of(x, wl, hop, center, np.float64)
    if unit:
        fr = fr * 2.0 ** -15
    fr = fr * window_ld(window, wl).astype(np.float64)[None, :]
    X = np.fft.rfft(fr, n=n_fft, axis=1)
    P = X.real * X.real + X.imag * X.imag
    return P @ filterbank_ld(hz, n_fft, n_mels, f_min, f_max).astype(np.float64).T


def rel_err(E, E_ld, total):
    """e(X); frames without power (all zero) must be exactly zero and do not enter."""
    E = np.asarray(E, dtype=LD)
    live = total > 0
    assert np.all(E[~live] == 0)
    if not live.any():
        return 0.0
    return float(np.max(np.abs(E[live] - E_ld[live]) / total[live, None]))


def gate_signal(hz, n, seed=20):
    """A 137 Hz tone of amplitude 8000 under a slow 3 Hz amplitude modulation, plus white noise of rms 300; the first
    six hops are exactly zero.  Every bin of every non-silent frame then carries a share of its frame's power far
    above the rounding error, so no bin is left out of a comparison."""
    t = np.arange(n, dtype=np.float64) / hz
    x = 8000.0 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * 137.0 * t)
    x += np.random.default_rng(seed).normal(0.0, 300.0, n)
    x[:6 * geometry(hz)[1]] = 0.0
    return x


def gate_case(hz, n_mels, window, center, n_fft=0, frames=12):
    wl, hop, _ = geometry(hz)
    x = gate_signal(hz, (6 + frames) * hop + wl + 3)
    E_ld, total = model_ld(x, hz, n_mels, window=window, center=center, n_fft=n_fft)
    e64 = rel_err(model_f64(x, hz, n_mels, window=window, center=center, n_fft=n_fft), E_ld, total)
    return x, E_ld, total, e64


def check_gates(run, hz, n_mels, window, center, who, n_fft=0):
    """run(x, opts) -> [T, n_mels]: the linear gate in f64; the log gate in f64, in unit scale as stated and in 16-bit
    scale with half an f64 ulp of the reference value added (the rounding of the result itself: see
    tests/test_fbank_abi.py); the log gate in f32 in both scales."""
    import jbonsai_amd as J

    x, E_ld, total, e64 = gate_case(hz, n_mels, window, center, n_fft)
    kw = dict(n_mels=n_mels, window=window, center=center, n_fft=n_fft)
    silent = total == 0
    live = ~silent
    assert silent.sum() >= 3 and live.sum() >= 8 and 0 < e64 < 1e-15
    # a filter that covers no bin (narrow filters on a coarse grid) is exactly 0, or the floor; of the others none is
    # left out: each carries, in every live frame, a share of the frame's power far above the gate
    covered = filterbank_ld(hz, geometry(hz, n_fft=n_fft)[2], n_mels).sum(axis=1) > 0
    assert covered.sum() >= min(n_mels, 16) and np.all(E_ld[:, ~covered] == 0)
    assert np.min(E_ld[live][:, covered] / total[live, None]) > 2e-8
    E = run(x, J.fbank(linear=True, f64=True, **kw))
    e = rel_err(E, E_ld, total)
    print(f"{who} {hz} Hz n_fft {geometry(hz, n_fft=n_fft)[2]} {n_mels} mels window {window} center {center}: "
          f"e(model_f64) {e64:.2e}  e {e:.2e}  ratio {e / e64:.2f}")
    assert E.dtype == np.float64 and E.shape == E_ld.shape and e <= GATE * e64
    assert np.all(E[:, ~covered] == 0.0)
    # JB_FBANK_UNIT under LINEAR: every value scaled by exactly 2^-30
    Eu = run(x, J.fbank(linear=True, f64=True, unit=True, **kw))
    assert np.array_equal(Eu, E * 2.0 ** -30)
    E32 = run(x, J.fbank(linear=True, **kw))
    assert E32.dtype == np.float32 and np.array_equal(E32, E.astype(np.float32))
    ln_floor = float(np.log(LD(2.0 ** -52)))
    pick = np.ix_(live, covered)
    bound = GATE * e64 * (total[live, None] / E_ld[pick])
    ref = {False: np.log(E_ld[pick]), True: np.log(E_ld[pick] * LD(2) ** -30)}
    for unit in (True, False):
        # log, f64: the stated bound in unit scale; in 16-bit scale plus half an f64 ulp of the reference value
        y = run(x, J.fbank(f64=True, unit=unit, **kw))
        half_ulp = 0 if unit else np.spacing(np.abs(ref[unit].astype(np.float64))).astype(LD) / 2
        assert np.all(y[silent] == ln_floor) and np.all(y[:, ~covered] == ln_floor)
        assert np.all(np.abs(y[pick].astype(LD) - ref[unit]) <= bound + half_ulp), unit
        # log, f32: plus one f32 ulp of the reference value
        y32 = run(x, J.fbank(unit=unit, **kw))
        ulp = np.spacing(np.abs(ref[unit].astype(np.float32))).astype(LD)
        assert y32.dtype == np.float32 and np.all(y32[silent] == np.float32(ln_floor))
        assert np.all(y32[:, ~covered] == np.float32(ln_floor))
        assert np.all(np.abs(y32[pick].astype(LD) - ref[unit]) <= bound + ulp), unit
    # an explicit floor
    yf = run(x, J.fbank(f64=True, log_floor=1e30, **kw))
    assert np.all(yf == float(np.log(LD(1e30))))
