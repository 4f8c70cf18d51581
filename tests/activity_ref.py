"""The speech-activity rule (include/jbonsai_amd.h "Speech activity") in numpy float64, written from the text: the four
grids, the frame energy as 64 strided partials folded 32, 16, .., 1, the gate, and the three smoothing steps the naive
way.  Shares no code with jbonsai_amd/csrc/jb_activity.h.  Also the cases the host and the GPU tests share."""
import numpy as np

SNIP, CENTER, KALDI, STFT = range(4)
GRIDS = {"snip": SNIP, "center": CENTER, "kaldi": KALDI, "stft": STFT}
WINDOWS = [2, 63, 64, 65, 400, 1200, 4096]


def hops_of(wl):
    return sorted({1, wl, wl + 7, 160})


def lengths_of(wl, hop):
    return sorted({0, 1, wl - 1, wl, wl + 1, wl + hop})


def frames(grid, n, wl, hop):
    """(T, s_0): frame t starts at s_0 + t hop"""
    if n == 0:
        return 0, 0
    if grid == SNIP:
        return (1 + (n - wl) // hop if n >= wl else 0), 0
    if grid == CENTER:
        return -(-n // hop), -(wl // 2)
    if grid == KALDI:
        return (n + hop // 2) // hop, hop // 2 - wl // 2
    return 1 + n // hop, -(wl // 2)


def energies(x, start, n_unit, grid, wl, hop):
    """E[T] of the column that holds x at `start` within a unit of n_unit samples and 0 elsewhere"""
    x = np.asarray(x, dtype=np.float64)
    T, s0 = frames(grid, n_unit, wl, hop)
    E = np.zeros(T, dtype=np.float64)
    lo = max(wl, -s0) + 1
    col = np.zeros(lo + max(n_unit, s0 + (T - 1) * hop + wl if T else 0) + wl + 1, dtype=np.float64)
    col[lo + start:lo + start + x.size] = x
    for t0 in range(0, T, 128):
        t1 = min(T, t0 + 128)
        idx = lo + s0 + np.arange(t0, t1)[:, None] * hop + np.arange(wl)[None, :]
        v = col[idx]
        p = np.zeros((t1 - t0, 64), dtype=np.float64)
        for k in range(0, wl, 64):
            seg = v[:, k:k + 64]
            p[:, :seg.shape[1]] = p[:, :seg.shape[1]] + seg * seg
        w = 32
        while w:
            p[:, :w] = p[:, :w] + p[:, w:2 * w]
            w //= 2
        E[t0:t1] = p[:, 0]
    return E


def ratio(gate_db):
    return float(np.power(np.longdouble(10), -np.longdouble(gate_db) / np.longdouble(10)))


def abs_threshold(gate_db, wl):
    return float(np.longdouble(wl) * np.longdouble(1073741824) *
                 np.power(np.longdouble(10), -np.longdouble(gate_db) / np.longdouble(10)))


def gate(E, gate_db, wl, reference="peak"):
    """(raw bits, peak, thr)"""
    peak = float(E.max()) if E.size and E.max() > 0 else 0.0
    thr = abs_threshold(gate_db, wl) if reference == "abs" else ratio(gate_db) * peak
    return ((E > 0) & (E >= thr)).astype(np.uint8), peak, thr


def smooth(r, min_speech=0, min_gap=0, hang_before=0, hang_after=0):
    """close, open, hang -- each as the text says it, frame by frame"""
    r = np.asarray(r, dtype=np.uint8)
    T = r.size
    on = np.flatnonzero(r)
    c = r.copy()
    for t in range(T):
        if r[t]:
            continue
        a, b = on[on < t], on[on > t]
        if a.size and b.size and b[0] - a[-1] - 1 <= min_gap:
            c[t] = 1
    o = c.copy()
    t = 0
    while t < T:
        if not c[t]:
            t += 1
            continue
        e = t
        while e < T and c[e]:
            e += 1
        if e - t < min_speech:
            o[t:e] = 0
        t = e
    h = np.zeros(T, dtype=np.uint8)
    for s in np.flatnonzero(o):
        h[max(0, s - hang_before):min(T, s + hang_after + 1)] = 1
    return h


def column(x, start, n_unit, grid, wl, hop, gate_db=40.0, reference="peak", **lengths):
    """(labels [T], report dict) of one column"""
    E = energies(x, start, n_unit, grid, wl, hop)
    r, peak, thr = gate(E, gate_db, wl, reference)
    lab = smooth(r, **lengths) if any(lengths.values()) else r
    return lab, report_of(lab, peak, thr)


def report_of(lab, peak=None, thr=None):
    on = np.flatnonzero(lab)
    rep = {"active": int(on.size), "first": int(on[0]) if on.size else lab.size,
           "last": int(on[-1]) if on.size else lab.size}
    if peak is not None:
        rep.update(peak=peak, thr=thr)
    return rep


def unit_report_of(mat):
    k = mat.sum(axis=1) if mat.size else np.zeros(mat.shape[0])
    return {"frames": mat.shape[0], "none": int((k == 0).sum()), "one": int((k == 1).sum()), "many": int((k >= 2).sum())}


def same_report(rep, want):
    got = {k: getattr(rep, k) for k in want}
    assert got == want, (got, want)


def speechy(n, seed, i16=False):
    """n samples of noise under an envelope of loud and quiet stretches, so that a 40 dB gate cuts through it"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 3000.0
    if n:
        env = np.repeat(rng.choice([1.0, 1e-3, 0.0, 0.3], size=n // 97 + 1), 97)[:n]
        x = x * env
    return np.trunc(np.clip(x, -32768, 32767)).astype(np.int16) if i16 else x


def pattern_pcm(bits, wl, amp=1000.0):
    """PCM on the snip grid with hop = wl whose raw bits under a peak gate are exactly `bits` (at least one set): frame t
    holds a constant `amp` where bits[t] is set and 0 elsewhere"""
    return np.repeat(np.asarray(bits, dtype=np.float64) * amp, wl)
