"""The frame conditioning rule of include/jbonsai_amd.h ("Frame conditioning") restated twice in numpy, on top of
tests/fbank_ref.py: the reflected index table, the five windows, DC removal, the raw energy, pre-emphasis.

model_ld works in numpy.longdouble throughout (the mean, the energy and the DFT in their natural order); model_f64 in
float64 with numpy's own sums and numpy.fft.rfft.  Neither follows the stated summation order: the library is held to

    e(X) = max over t, m of |E_X - E_ld| / sum_k P_ld[t][k]  <=  GATE * e(model_f64)

as in tests/fbank_ref.py, so the bound is again the error of an ordinary float64 computation of the same frames.
"""
import numpy as np

from tests import fbank_ref as R

LD = np.longdouble
GATE = R.GATE
WINDOW_OPTS, POVEY, HANN_SYM, RECT, BLACKMAN = range(5)
WINDOWS = (WINDOW_OPTS, POVEY, HANN_SYM, RECT, BLACKMAN)
NAMES = {WINDOW_OPTS: None, POVEY: "povey", HANN_SYM: "hann_sym", RECT: "rect", BLACKMAN: "blackman"}


def n_frames(n, wl, hop, center=False, reflect=False):
    return (n + hop // 2) // hop if reflect else R.n_frames(n, wl, hop, center)


def reflect_index(k, n):
    while k < 0 or k >= n:
        k = -k - 1 if k < 0 else 2 * n - 1 - k
    return k


def index_table(n, wl, hop, center=False, reflect=False):
    """[T, wl]: the sample each value of each frame reads; -1: a zero outside the unit."""
    T = n_frames(n, wl, hop, center, reflect)
    idx = np.full((T, wl), -1, dtype=np.int64)
    for t in range(T):
        k0 = t * hop + (hop // 2 - wl // 2 if reflect else -(wl // 2) if center else 0)
        for i in range(wl):
            k = k0 + i
            if reflect:
                idx[t, i] = reflect_index(k, n)
            elif 0 <= k < n:
                idx[t, i] = k
    return idx


def window_ld(kind, wl, fbank_window=R.HANN):
    if kind == WINDOW_OPTS:
        return R.window_ld(fbank_window, wl)
    a = 2 * np.arccos(LD(-1)) / LD(wl - 1)
    j = np.arange(wl, dtype=LD)
    h = LD("0.5") - LD("0.5") * np.cos(a * j)
    if kind == POVEY:
        return np.power(h, LD("0.85"))
    if kind == HANN_SYM:
        return h
    if kind == BLACKMAN:
        return LD("0.42") - LD("0.5") * np.cos(a * j) + LD("0.08") * np.cos(2 * a * j)
    return np.ones(wl, dtype=LD)


def frames_of(x, idx, dtype):
    x = np.asarray(x, dtype=dtype)
    xz = np.concatenate([x, np.zeros(1, dtype=dtype)])  # (index -1: the zero)
    return xz[idx] if idx.size else np.zeros(idx.shape, dtype=dtype)


def condition(fr, win, preemph, remove_dc, dtype):
    """(z [T, wl], energy [T]): steps 2 to 5 of the rule in `dtype`."""
    v = fr.astype(dtype)
    if remove_dc and v.shape[0]:
        v = v - (v.sum(axis=1) / dtype(v.shape[1]))[:, None]
    energy = (v * v).sum(axis=1)
    if preemph > 0:
        prev = np.concatenate([v[:, :1], v[:, :-1]], axis=1)
        v = v - dtype(preemph) * prev
    return v * win.astype(dtype)[None, :], energy


def _spectra(x, hz, window, center, reflect, unit, preemph, remove_dc, n_fft, win_us, hop_us, fbank_window, dtype):
    wl, hop, n_fft = R.geometry(hz, win_us, hop_us, n_fft)
    fr = frames_of(x, index_table(len(x), wl, hop, center, reflect), dtype)
    if unit:
        fr = fr * dtype(2) ** -15
    z, energy = condition(fr, window_ld(window, wl, fbank_window), preemph, remove_dc, dtype)
    return z, energy, wl, n_fft


def model_ld(x, hz, n_mels, window=WINDOW_OPTS, center=False, reflect=False, unit=False, preemph=0.0, remove_dc=False,
             n_fft=0, f_min=0.0, f_max=0.0, win_us=25000, hop_us=10000, fbank_window=R.HANN):
    """(E [T, n_mels], total power per frame [T], raw energy per frame [T]) in long double."""
    z, energy, wl, n_fft = _spectra(x, hz, window, center, reflect, unit, preemph, remove_dc, n_fft, win_us, hop_us,
                                    fbank_window, LD)
    c, s = R._dft_ld(n_fft, wl)
    re, im = z @ c, z @ s
    P = re * re + im * im
    return P @ R.filterbank_ld(hz, n_fft, n_mels, f_min, f_max).T, P.sum(axis=1), energy


def model_f64(x, hz, n_mels, window=WINDOW_OPTS, center=False, reflect=False, unit=False, preemph=0.0,
              remove_dc=False, n_fft=0, f_min=0.0, f_max=0.0, win_us=25000, hop_us=10000, fbank_window=R.HANN):
    """E [T, n_mels] in float64 through numpy.fft.rfft."""
    z, _, wl, n_fft = _spectra(x, hz, window, center, reflect, unit, preemph, remove_dc, n_fft, win_us, hop_us,
                               fbank_window, np.float64)
    X = np.fft.rfft(z, n=n_fft, axis=1)
    P = X.real * X.real + X.imag * X.imag
    return P @ R.filterbank_ld(hz, n_fft, n_mels, f_min, f_max).astype(np.float64).T


def gate_signal(hz, n, hop, offset=0.0):
    """fbank_ref.gate_signal with its first six hops of `hop` samples exactly zero (whatever the geometry) and a DC
    offset on the live part."""
    lead = 6 * R.geometry(hz)[1]
    x = R.gate_signal(hz, n + lead)[lead - 6 * hop:][:n].copy()
    assert np.all(x[:6 * hop] == 0)
    x[6 * hop:] += offset
    return x


def opts_of(J, n_mels, window=WINDOW_OPTS, center=False, reflect=False, preemph=0.0, remove_dc=False, n_fft=0,
            win_us=25000, hop_us=10000, fbank_window=R.HANN, **kw):
    """(FbankOpts, FrameOpts) of a model call; kw: further keywords of J.fbank."""
    f = J.fbank(win_ms=win_us / 1000.0, hop_ms=hop_us / 1000.0, n_mels=n_mels, n_fft=n_fft, window=fbank_window,
                center=center, **kw)
    return f, J.frame(preemph=preemph, window=NAMES[window], remove_dc=remove_dc, reflect=reflect)


def check_gate(run, x, hz, n_mels, who, min_live=1, **kw):
    """run(x, fopts, fr) -> [T, n_mels]: the linear f64 gate of the rule on x; kw: the model's keywords.  Returns
    (e, e64).  The preconditions of tests/fbank_ref.py's check_gates hold: the float64 model's own error is small and
    not zero, every covered filter keeps a share of its frame's power far above the rounding error, and a frame
    without power is exactly zero (rel_err), so no element is left out."""
    import jbonsai_amd as J

    E_ld, total, _ = model_ld(x, hz, n_mels, **kw)
    e64 = R.rel_err(model_f64(x, hz, n_mels, **kw), E_ld, total)
    live = total > 0
    assert live.sum() >= min_live and 0 < e64 < 1e-15, (who, e64)
    n_fft = R.geometry(hz, kw.get("win_us", 25000), kw.get("hop_us", 10000), kw.get("n_fft", 0))[2]
    covered = R.filterbank_ld(hz, n_fft, n_mels).sum(axis=1) > 0
    assert covered.any() and np.all(E_ld[:, ~covered] == 0)
    share = float(np.min(E_ld[live][:, covered] / total[live, None]))
    assert share > 2e-8, (who, share)
    f, fr = opts_of(J, n_mels, linear=True, f64=True, **kw)
    E = run(x, f, fr)
    assert E.dtype == np.float64 and E.shape == E_ld.shape
    e = R.rel_err(E, E_ld, total)
    print(f"{who} {hz} Hz n_fft {n_fft} {kw}: silent {int((~live).sum())} live {int(live.sum())} share {share:.1e} "
          f"e(model_f64) {e64:.2e}  e {e:.2e}  ratio {e / e64:.2f}")
    assert np.all(E[:, ~covered] == 0.0)
    assert e <= GATE * e64, (who, e / e64)
    return e, e64
