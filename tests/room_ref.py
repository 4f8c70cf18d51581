"""An independent model of the room responses (include/jbonsai_amd.h "Room responses"), numpy only.

model_ld     the rule as stated: the tables (long double, rounded once to doubles) and every sum in numpy.longdouble
model_f64    the same in float64, vectorised, in numpy's own order: the yardstick of the accuracy gate
model_exact  a plain loop over the images (n, p) with numpy.sinc and the Hann window directly: no tables, no sorting

A room is a dict: size, source, mic (3 floats each), beta (6), c, hz, n_taps, unit (bool)."""
import numpy as np

LD = np.longdouble
WH, Q = 32, 128
TOP = Q * WH
PI = np.arccos(LD(-1))


def room(size, source, mic, beta, hz=8000, n_taps=513, c=343.0, unit=True):
    b = [float(beta)] * 6 if np.isscalar(beta) else [float(v) for v in beta]
    return dict(size=[float(v) for v in size], source=[float(v) for v in source], mic=[float(v) for v in mic], beta=b,
                c=float(c), hz=int(hz), n_taps=int(n_taps), unit=bool(unit))


def lowpass_ld():
    """F[0 .. Q Wh + 2] in long double, in the header's well-conditioned forms."""
    q = np.arange(TOP + 1)
    n, rq = q // Q, q % Q
    sign = np.where(n % 2 == 1, LD(-1), LD(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = sign * np.sin(PI * (rq.astype(LD) / Q)) / (PI * (q.astype(LD) / Q))
    sinc[rq == 0] = 0
    sinc[0] = 1
    s = np.sin(PI * (TOP - q).astype(LD) / LD(2 * TOP))
    return np.concatenate([sinc * (s * s), np.zeros(2, dtype=LD)])


def lowpass_direct(t):
    """sinc(t) times the Hann window of half-width Wh, float64, straight from the formula."""
    t = np.asarray(t, dtype=np.float64)
    return np.sinc(t) * 0.5 * (1.0 + np.cos(np.pi * t / WH))


def axis_table(L, s, r, b0, b1, Rmax):
    """(D2, g) of one axis as float64 arrays: entries sorted by |D|, ties by (n, p); g == 0 left out."""
    L, s, r, b0, b1 = LD(L), LD(s), LD(r), LD(b0), LD(b1)
    Na = int(np.ceil(Rmax / (2 * L))) + 1
    rows = []
    for n in range(-Na, Na + 1):
        for p in (0, 1):
            D = (LD(1 - 2 * p) * s + LD(2) * LD(n) * L) - r
            g = float(b0 ** abs(n - p) * b1 ** abs(n))
            if g == 0.0:
                continue
            rows.append((abs(D), n, p, float(D * D), g))
    rows.sort(key=lambda e: (e[0], e[1], e[2]))
    return np.array([e[3] for e in rows]), np.array([e[4] for e in rows])


def tables(rm):
    """The rule's tables and constants of a room."""
    c = LD(rm["c"] if rm["c"] else 343.0)
    K, hz = rm["n_taps"], rm["hz"]
    Rmax = c * LD(K + WH) / LD(hz)
    D2, g = [], []
    for a in range(3):
        d2, ga = axis_table(rm["size"][a], rm["source"][a], rm["mic"][a], rm["beta"][2 * a], rm["beta"][2 * a + 1], Rmax)
        D2.append(d2)
        g.append(ga)
    kappa = float(LD(hz) / c)
    fourpi = float(4 * PI)
    D2o = [float((LD(rm["source"][a]) - LD(rm["mic"][a])) ** 2) for a in range(3)]
    d0 = float(np.sqrt((D2o[0] + D2o[1]) + D2o[2]))
    return dict(D2=D2, g=g, kappa=kappa, fourpi=fourpi, d0=d0, direct=int(np.floor(d0 * kappa + 0.5)), K=K,
                unit=rm["unit"], entries=[len(x) for x in D2])


def _model(rm, dtype):
    tb = tables(rm)
    K = tb["K"]
    F = lowpass_ld().astype(np.float64).astype(dtype)  # the table is rounded once: part of the rule
    D2x, D2y, D2z = (x.astype(dtype) for x in tb["D2"])
    gx, gy, gz = (x.astype(dtype) for x in tb["g"])
    s2 = ((D2x[:, None, None] + D2y[None, :, None]) + D2z[None, None, :]).reshape(-1)  # i major, m minor
    w = ((gx[:, None, None] * gy[None, :, None]) * gz[None, None, :]).reshape(-1)
    d = np.sqrt(s2)
    tau = d * dtype(tb["kappa"])
    A = w / (d / dtype(tb["d0"])) if tb["unit"] else w / (dtype(tb["fourpi"]) * d)
    keep = tau < K + WH
    tau, A = tau[keep], A[keep]
    base = np.floor(tau).astype(np.int64)
    k = base[:, None] + np.arange(-WH, WH + 1)[None, :]
    t = k.astype(dtype) - tau[:, None]
    ok = (np.abs(t) < WH) & (k >= 0) & (k < K)
    u = np.abs(t) * Q
    i0 = np.minimum(np.floor(u).astype(np.int64), TOP)
    f = u - i0.astype(dtype)
    lp = f * (F[i0 + 1] - F[i0]) + F[i0]
    term = A[:, None] * lp
    h, S, SA = np.zeros(K, dtype=dtype), np.zeros(K, dtype=dtype), np.zeros(K, dtype=dtype)
    np.add.at(h, k[ok], term[ok])
    np.add.at(S, k[ok], np.abs(term[ok]))
    np.add.at(SA, k[ok], np.abs(np.broadcast_to(A[:, None], term.shape)[ok]))
    return h, S, SA


def model_ld(rm):
    """(h, S, SA) in long double: the taps, S_k = sum |A lp| and SA_k = sum |A| over tap k's terms."""
    return _model(rm, LD)


def model_f64(rm):
    """The taps in float64, numpy's own order."""
    return _model(rm, np.float64)[0]


def model_exact(rm):
    """The taps from the images directly: every (n, p) of every axis, numpy.sinc and the Hann window, float64."""
    c = rm["c"] if rm["c"] else 343.0
    K, hz = rm["n_taps"], rm["hz"]
    Rmax = c * (K + WH) / hz
    ax = []
    for a in range(3):
        L, s, r, b0, b1 = rm["size"][a], rm["source"][a], rm["mic"][a], rm["beta"][2 * a], rm["beta"][2 * a + 1]
        Na = int(np.ceil(Rmax / (2 * L))) + 1
        D, g = [], []
        for n in range(-Na, Na + 1):
            for p in (0, 1):
                D.append((1 - 2 * p) * s + 2 * n * L - r)
                g.append(b0 ** abs(n - p) * b1 ** abs(n))
        ax.append((np.array(D), np.array(g)))
    d0 = np.sqrt(sum((rm["source"][a] - rm["mic"][a]) ** 2 for a in range(3)))
    kk = np.arange(K, dtype=np.float64)
    h = np.zeros(K)
    (Dx, gx), (Dy, gy), (Dz, gz) = ax
    for i in range(len(Dx)):
        for j in range(len(Dy)):
            d = np.sqrt(Dx[i] ** 2 + Dy[j] ** 2 + Dz ** 2)
            w = gx[i] * gy[j] * gz
            A = w * d0 / d if rm["unit"] else w / (4 * np.pi * d)
            tau = d * hz / c
            for m in np.nonzero((tau < K + WH) & (w != 0))[0]:
                t = kk - tau[m]
                near = np.abs(t) < WH
                h[near] += A[m] * lowpass_direct(t[near])
    return h


def metric(h, h_ld, S):
    """max_k |h - model_ld| / max_k S_k, as a float."""
    return float(np.max(np.abs(np.asarray(h, dtype=LD) - h_ld)) / np.max(S))


def gate(rm, ref=None):
    """(h_ld, S, SA, bound): the long-double taps and the accuracy gate 8 e_np (e_np at least 2^-52)."""
    h_ld, S, SA = ref if ref is not None else model_ld(rm)
    e_np = max(metric(model_f64(rm), h_ld, S), 2.0 ** -52)
    return h_ld, S, SA, 8.0 * e_np
