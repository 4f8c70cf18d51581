"""numpy evaluation of the group and R128 rules (include/jbonsai_amd.h "loudness", steps 6 to 8) on top of
tests/loudness_ref.py: the hop energies of an utterance, a group's gated loudness, peak and gain, the largest
momentary and short-term loudness and the loudness range.  Independent of the library: plain sums, a sort.

Every comparison against a gate asserts the precondition of the tests first: no block or window within MARGIN LU of
the gate it is compared with (there the last bits of a sum could decide membership)."""
import math

import numpy as np

from tests.loudness_ref import FULL_SCALE, gain_db, k_filter, k_weight

MARGIN = 1e-6


def loud(ms):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(ms)


def hop_energies(x, hz):
    """z_j of x at hz (full hops only) and the hop H."""
    x = np.asarray(x, dtype=np.float64)
    H = k_filter(hz)[2]
    nh = x.size // H
    if nh == 0:
        return np.zeros(0), H
    y = k_weight(x[: nh * H], hz)
    return np.sum((y * y).reshape(nh, H), axis=1), H


def block_ms(z, H):
    z = np.asarray(z, dtype=np.float64)
    if z.size < 4:
        return np.zeros(0)
    return (z[:-3] + z[1:-2] + z[2:-1] + z[3:]) / (4.0 * H)


def window_ms(z, H):
    z = np.asarray(z, dtype=np.float64)
    if z.size < 30:
        return np.zeros(0)
    return np.lib.stride_tricks.sliding_window_view(z, 30).sum(axis=1) / (30.0 * H)


def _clear_of(l, gate):
    assert not np.any(np.abs(l - gate) < MARGIN), ("a value within %g LU of the gate %r" % (MARGIN, gate))


def _gated(ms, rel):
    """(values above both gates, the relative gate); the relative gate is `rel` LU under the loudness of the mean of
    the values above -70."""
    l = loud(ms)
    _clear_of(l, -70.0)
    keep = l > -70.0
    if not keep.any():
        return ms[:0], -math.inf
    gamma = float(loud(math.fsum(ms[keep]) / int(keep.sum()))) + rel
    _clear_of(l[keep], gamma)
    return ms[keep & (l > gamma)], gamma


def db(peak):
    return 20.0 * math.log10(peak / FULL_SCALE) if peak > 0 else -math.inf


def group(zs, H, peaks, true_peaks=None, target=math.nan, ceiling=math.inf):
    """The group of members with hop energies zs[m] and largest magnitudes peaks[m] (true_peaks[m] in true-peak
    mode): dict of lufs, sample_peak_dbfs, true_peak_dbtp, gain_db."""
    ms = np.concatenate([block_ms(z, H) for z in zs]) if len(zs) else np.zeros(0)
    kept, _ = _gated(ms, -10.0)
    L = float(loud(math.fsum(kept) / kept.size)) if kept.size else -math.inf
    P = db(max(peaks, default=0.0))
    TP = math.nan if true_peaks is None else db(max(max(peaks, default=0.0), max(true_peaks, default=0.0)))
    return {"lufs": L, "sample_peak_dbfs": P, "true_peak_dbtp": TP,
            "gain_db": gain_db(L, P if true_peaks is None else TP, target, ceiling)}


def r128(zs, H):
    """The R128 fields of the set of members zs: dict as jb_loudness_r128."""
    bl = np.concatenate([block_ms(z, H) for z in zs]) if len(zs) else np.zeros(0)
    w = np.concatenate([window_ms(z, H) for z in zs]) if len(zs) else np.zeros(0)
    out = {"max_momentary_lufs": float(loud(bl.max())) if bl.size else -math.inf,
           "max_short_term_lufs": float(loud(w.max())) if w.size else -math.inf}
    kept, _ = _gated(w, -20.0)
    kept = np.sort(kept)
    n = int(kept.size)
    out["n_windows"] = n
    if n == 0:
        out.update(lra_lu=0.0, lra_low_lufs=math.nan, lra_high_lufs=math.nan)
        return out
    lo = float(kept[int(math.floor((n - 1) * 0.10 + 0.5))])
    hi = float(kept[int(math.floor((n - 1) * 0.95 + 0.5))])
    out.update(lra_lu=10.0 * math.log10(hi / lo), lra_low_lufs=float(loud(lo)), lra_high_lufs=float(loud(hi)))
    return out


def group_of_pcm(pcms, hz, true_peaks=None, target=math.nan, ceiling=math.inf):
    """group() and r128() of PCM: (group dict, set r128 dict, [member r128 dicts])."""
    zs, H = [], k_filter(hz)[2]
    for x in pcms:
        zs.append(hop_energies(x, hz)[0])
    peaks = [float(np.max(np.abs(x))) if len(x) else 0.0 for x in pcms]
    return group(zs, H, peaks, true_peaks, target, ceiling), r128(zs, H), [r128([z], H) for z in zs]
