"""A numpy model of the pitch stage, written from the rule in jbonsai_amd/csrc/jb_pitch.h (include/jbonsai_amd.h
"Pitch features"), in two precisions:

- `ft = np.longdouble`: the reference.  The tables are kept in long double as the formulas give them and every sum is
  numpy's in long double.
- `ft = np.float64`: the yardstick of the 8 times gate.  The tables are the long double ones rounded once (as the rule
  hands them to its arithmetic), every sum is numpy's own in float64 (not the rule's order).

Neither restates the rule's summation orders: what they share with the library is the mathematics alone.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
R = 4000
UP = 5
PI = LD("3.14159265358979323846264338327950288")


def ld(v):
    return LD(float(v)) if not isinstance(v, LD) else v


def filt(c, w, t):
    """f(t) = 2c sinc(2ct) (1 + cos(2 pi c t / w)) / 2 inside |t| < w / (2c), else 0; long double arrays."""
    t = np.asarray(t, dtype=LD)
    x = 2 * LD(c) * t
    safe = np.where(x == 0, LD(1), x)
    s = np.where(x == 0, LD(1), np.sin(PI * safe) / (PI * safe))
    f = 2 * LD(c) * s * LD(0.5) * (1 + np.cos(2 * PI * LD(c) * t / LD(w)))
    return np.where(np.abs(t) < LD(w) / (2 * LD(c)), f, LD(0))


def lags(o):
    """The lag grid in long double by the recipe: lag_0 = 1 / max_f0, lag_{i+1} = lag_i (1 + delta)."""
    out, l, top, step = [], LD(1) / ld(o.max_f0), LD(1) / ld(o.min_f0), LD(1) + ld(o.delta_pitch)
    while l <= top:
        out.append(l)
        l = l * step
    return np.array(out, dtype=LD)


def lag_range(o):
    a = max(0, math.floor(LD(R) / ld(o.max_f0) - LD(UP) / 2))
    b = math.ceil(LD(R) / ld(o.min_f0) + LD(UP) / 2)
    return int(a), int(b)


def decimate(x, hz, ft):
    """y[m] = (1 / hz) sum_k x[k] f(k / hz - m / r), m < ceil(n r / hz)."""
    x = np.asarray(x, dtype=ft)
    n = x.size
    n4 = (n * R + hz - 1) // hz
    y = np.zeros(n4, dtype=ft)
    if n4 == 0:
        return y
    m = np.arange(n4, dtype=np.int64)
    centre = (m * hz) // R
    D = (hz + 1999) // 2000 + 1
    for d in range(-D, D + 1):
        k = centre + d
        t = (k.astype(LD) * R - m.astype(LD) * hz) / (LD(hz) * R)  # k / hz - m / r, from exact integers
        w = (filt(1000, 1, t) / LD(hz)).astype(ft)
        ok = (k >= 0) & (k < n)
        y = y + np.where(ok, x[np.clip(k, 0, n - 1)] * w, ft(0))
    return y


def grid_weights(o, ft):
    """g_i[L] dense over [S][b - a + 1]."""
    lg = lags(o)
    a, b = lag_range(o)
    L = np.arange(a, b + 1).astype(LD)
    t = L[None, :] / LD(R) - lg[:, None]
    return (filt(R / 2, UP, t) / LD(R)).astype(ft)


def nccf(y, o, T, ft, energy=False):
    """(Q, P): [T][S] the two NCCFs of every frame over the lag grid; energy=True: and e_0 [T]."""
    y = np.asarray(y, dtype=ft)
    n4 = y.size
    wl4, sh4 = o.win_us // 250, o.hop_us // 250
    a, b = lag_range(o)
    kaldi = o.grid == 1
    off = sh4 // 2 - wl4 // 2 if kaldi else 0
    k = np.arange(T)[:, None] * sh4 + off + np.arange(wl4 + b)[None, :]
    ok = (k >= 0) & (k < n4)
    v = np.where(ok, y[np.clip(k, 0, max(n4 - 1, 0))] if n4 else ft(0), ft(0)).astype(ft)
    v = v - (v[:, :wl4].sum(axis=1) / ft(wl4))[:, None]
    if n4:
        mean = y.sum() / ft(n4)
        sigma2 = (y * y).sum() / ft(n4) - mean * mean
    else:
        sigma2 = ft(0)
    s = sigma2 * ft(wl4)
    B = ft(o.nccf_ballast) * (s * s)
    e0 = (v[:, :wl4] ** 2).sum(axis=1)
    nl = b - a + 1
    q = np.zeros((T, nl), dtype=ft)
    p = np.zeros((T, nl), dtype=ft)
    for L in range(a, b + 1):
        inner = (v[:, :wl4] * v[:, L:L + wl4]).sum(axis=1)
        eL = (v[:, L:L + wl4] ** 2).sum(axis=1)
        for dst, den in ((q, e0 * eL + B), (p, e0 * eL)):
            nz = den != 0
            dst[:, L - a] = np.where(nz, inner / np.sqrt(np.where(nz, den, ft(1))), ft(0))
    G = grid_weights(o, ft)
    return (q @ G.T, p @ G.T, e0) if energy else (q @ G.T, p @ G.T)


def local_costs(Q, o, ft):
    soft = (ld(o.soft_min_f0) * lags(o)).astype(ft)
    return (1 - Q) + soft[None, :] * Q


def kappa(o):
    k = np.log(LD(1) + ld(o.delta_pitch))
    return ld(o.penalty_factor) * k * k


def viterbi(local, o, ft):
    """The optimal lag indices of the local costs [T][S] (ties to the smallest index)."""
    T, S = local.shape
    i = np.arange(S)
    pen = (ft(kappa(o)) * ((i[:, None] - i[None, :]) ** 2).astype(ft))
    F = np.zeros(S, dtype=ft)
    back = np.zeros((T, S), dtype=np.int64)
    for t in range(T):
        c = F[None, :] + pen
        back[t] = np.argmin(c, axis=1)
        F = c[i, back[t]] + local[t]
        F = F - F.min()
    idx = np.zeros(T, dtype=np.int64)
    s = int(np.argmin(F))
    for t in range(T - 1, -1, -1):
        idx[t] = s
        s = back[t, s]
    return idx


def path_cost(local, idx, o):
    """The total cost of a path over long double local costs, in long double (F_{-1} = 0: the first state is free)."""
    idx = np.asarray(idx, dtype=np.int64)
    T = idx.size
    if T == 0:
        return LD(0)
    c = local[np.arange(T), idx].astype(LD).sum()
    d = np.diff(idx).astype(LD)
    return c + kappa(o) * (d * d).sum()


def columns(idx, p, o, ft, width=4):
    """The processed columns [T][width] from the frames' lag indices and p at them."""
    idx = np.asarray(idx, dtype=np.int64)
    T = idx.size
    p = np.asarray(p, dtype=ft)
    logp = np.log(LD(1) / lags(o)).astype(ft)[idx]
    c = np.clip(p, ft(-1), ft(1))
    pov = ft(o.pov_scale) * ((ft(1.0001) - c) ** ft(0.15) - 1)  # 1.0001 and 0.15: the doubles the rule names
    a = np.minimum(np.abs(p), ft(1))
    rho = (ft(-5.2) + ft(5.4) * np.exp(ft(7.5) * (a - 1)) + ft(4.8) * a - ft(2) * np.exp(ft(-10) * a) +
           ft(4.2) * np.exp(ft(20) * (a - 1)))
    w = 1 / (1 + np.exp(-rho))
    out = np.zeros((T, 4), dtype=ft)
    for t in range(T):
        j0, j1 = max(0, t - o.norm_left), min(T - 1, t + o.norm_right)
        ws = w[j0:j1 + 1]
        out[t, 1] = ft(o.pitch_scale) * (logp[t] - (ws * logp[j0:j1 + 1]).sum() / ws.sum())
        d = sum(ft(k) * logp[min(max(t + k, 0), T - 1)] for k in range(-2, 3))
        out[t, 2] = ft(o.delta_scale) * (d / ft(10))
    out[:, 0] = pov
    out[:, 3] = logp
    return out[:, :width]


def test_signal(seed, hz, n):
    """A seeded mixture of a gliding harmonic part, noise, a silent stretch and a DC offset, in the 16-bit scale."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / hz
    f0 = rng.uniform(80, 140) + rng.uniform(40, 120) * t / max(t[-1], 1e-9) if n else np.zeros(0)
    phase = 2 * np.pi * np.cumsum(f0) / hz
    x = np.zeros(n)
    for k in range(1, 6):
        x += np.cos(k * phase + k) / k
    x = 4000 * x + 300 * rng.standard_normal(n) + 150.0
    if n >= 8:
        a = int(rng.integers(n // 4, n // 2))
        x[a:a + n // 8] = 150.0
    return x


test_signal.__test__ = False
