"""numpy evaluation of the loudness definition (include/jbonsai_amd.h "loudness"; ITU-R BS.1770-4 / EBU R128):
K-weighting by a direct-form recursion, hops, blocks, both gates, the sample peak and the gain.  Independent of the
library: the coefficients come from the formula here, not from jb_loudness_filter."""
import math

import numpy as np

FULL_SCALE = 32768.0


def k_filter(hz):
    """(b, a) as [2][3] arrays (shelf, then high-pass) and the hop H at hz."""
    fs = float(hz)

    def stage(fc, Q, shelf):
        K = math.tan(math.pi * fc / fs)
        a0 = 1.0 + K / Q + K * K
        if shelf:
            Vh = 10.0 ** (3.999843853973347 / 20.0)
            Vb = Vh ** 0.4996667741545416
            b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
        else:
            b = [1.0, -2.0, 1.0]
        return b, [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]

    b1, a1 = stage(1681.974450955533, 0.7071752369554196, True)
    b2, a2 = stage(38.13547087602444, 0.5003270373238773, False)
    return np.array([b1, b2]), np.array([a1, a2]), (int(hz) + 5) // 10


def _biquad(x, b, a):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], zero initial state (direct form I)."""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for n, xn in enumerate(x):
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        y[n] = yn
        x2, x1, y2, y1 = x1, xn, y1, yn
    return y


def k_weight(x, hz):
    b, a, _ = k_filter(hz)
    xs = (np.asarray(x, dtype=np.float64) / FULL_SCALE).tolist()
    return np.array(_biquad(_biquad(xs, b[0], a[0]), b[1], a[1]))


def integrated(x, hz):
    """(L, P) of x at hz: integrated loudness (LUFS, -inf when no block survives) and sample peak (dBFS)."""
    x = np.asarray(x, dtype=np.float64)
    _, _, H = k_filter(hz)
    peak = float(np.max(np.abs(x))) if x.size else 0.0
    with np.errstate(divide="ignore"):
        P = 20.0 * math.log10(peak / FULL_SCALE) if peak > 0 else -math.inf
    N = x.size
    nh = N // H
    if nh < 4:
        return -math.inf, P
    y = k_weight(x[: nh * H], hz)
    z = np.sum((y * y).reshape(nh, H), axis=1)
    ms = (z[:-3] + z[1:-2] + z[2:-1] + z[3:]) / (4.0 * H)
    with np.errstate(divide="ignore"):
        lb = -0.691 + 10.0 * np.log10(ms)
    keep = lb > -70.0
    if not keep.any():
        return -math.inf, P
    gamma = -0.691 + 10.0 * math.log10(float(np.mean(ms[keep]))) - 10.0
    keep &= lb > gamma
    if not keep.any():
        return -math.inf, P
    return -0.691 + 10.0 * math.log10(float(np.mean(ms[keep]))), P


def gain_db(L, P, target, ceiling):
    terms = [v for v in (target - L, ceiling - P) if math.isfinite(v)]
    return min(terms) if terms else 0.0
