"""Dense extended-precision reference of parameter generation: the equation W' U^-1 W c = W' U^-1 mu itself, built as
dense matrices and solved in numpy.longdouble.  numpy only: no GPU, no oracle, and no code shape shared with the band
accumulation of mlpg.rs:25-70 (which oracle/jbo_hot.c and jb_mlpg.hip both restate).

What it follows of the reference: the mask and the boundary distances (mask.rs:20-28,51-82), with_ivar in f64
(mean_vari.rs:21-31), the zeroed inverse variance of a dynamic window at an MSD boundary (mod.rs:69-80), the
compaction to voiced frames (mod.rs:81) and the GV ascent (mlpg.rs:168-292).

What it does NOT follow: the `break` of mlpg.rs:53-55, which sits in a reversed iteration and drops in-range terms
near the end of the sequence.  Those terms carry a zeroed inverse variance for every dynamic window, so the two agree
unless the FIRST window has more than one tap (tests/test_mlpg_dense.py records that case)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np

LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of f64, the arithmetic under test
NODATA = -1e10  # src/constants.rs:13


@dataclass
class Stream:
    """State-level image of one stream of one utterance (ModelStream): mean, var [S][W*L] (window-major: column
    L*w + d), msd [S] or None for a stream without MSD, gv_mean, gv_var [L] and gv_switch [S] or None without GV."""
    L: int
    windows: List[List[float]]
    mean: np.ndarray
    var: np.ndarray
    msd: Optional[np.ndarray] = None
    msd_threshold: float = 0.5
    gv_mean: Optional[np.ndarray] = None
    gv_var: Optional[np.ndarray] = None
    gv_switch: Optional[np.ndarray] = None
    gv_weight: float = 1.0

    @property
    def is_msd(self):
        return self.msd is not None

    @property
    def use_gv(self):
        return self.gv_mean is not None


def with_ivar(var):
    """MeanVari::with_ivar in f64 (mean_vari.rs:21-31)."""
    var = np.asarray(var, dtype=np.float64)
    with np.errstate(divide="ignore"):
        iv = 1.0 / var
    return np.where(np.abs(var) > 1e19, 0.0, np.where(np.abs(var) < 1e-19, 1e38, iv))


def voiced_mask(stream: Stream, durations):
    """[T] bool: msd[state] > threshold (strict), expanded by durations; all true without MSD."""
    durations = np.asarray(durations, dtype=np.int64)
    if not stream.is_msd:
        return np.ones(int(durations.sum()), dtype=bool)
    return np.repeat(np.asarray(stream.msd, dtype=np.float64) > stream.msd_threshold, durations)


def boundary_distances(mask):
    """(left, right): frames between a voiced frame and the first / last frame of its voiced run (mask.rs:51-82)."""
    mask = np.asarray(mask, dtype=bool)
    T = len(mask)
    left, right = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    # each run once, by its two ends
    edges = np.flatnonzero(np.diff(np.concatenate(([False], mask, [False])).astype(np.int8)))
    for first, past in zip(edges[0::2], edges[1::2]):
        left[first:past] = np.arange(past - first)
        right[first:past] = np.arange(past - first)[::-1]
    return left, right


def window_matrix(coef, N):
    """W_i, N x N: row tau holds the taps at columns tau + k - lw that are inside [0, N)."""
    coef = np.asarray(coef, dtype=LD)
    width = len(coef)
    lw = width // 2
    Wm = np.zeros((N, N), dtype=LD)
    for k in range(width):
        off = k - lw
        rows = np.arange(max(0, -off), min(N, N - off))
        Wm[rows, rows + off] = coef[k]
    return Wm


def normal_equations(Wm, ivar, mu, sparse=True):
    """(W' diag(ivar) W, W' (ivar * mu)) in long double.  sparse=True evaluates the same product row by row over each
    row's non-zero columns (a sum of outer products), which is the same sum without the N^3 multiplications by zero;
    tests/test_mlpg_dense.py holds the two forms together."""
    N = len(ivar)
    if not sparse:
        return Wm.T @ (ivar[:, None] * Wm), Wm.T @ (ivar * mu)
    A, b = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD)
    for tau in range(N):
        nz = np.flatnonzero(Wm[tau])
        w = Wm[tau, nz]
        A[np.ix_(nz, nz)] += ivar[tau] * np.outer(w, w)
        b[nz] += w * (ivar[tau] * mu[tau])
    return A, b


def dense_system(stream: Stream, durations, dims=None):
    """(voiced_idx, [(A_d, b_d) for d in dims]) in long double; dims defaults to range(L)."""
    durations = np.asarray(durations, dtype=np.int64)
    state = np.repeat(np.arange(len(durations)), durations)
    mask = voiced_mask(stream, durations)
    left, right = boundary_distances(mask)
    voiced_idx = np.flatnonzero(mask)
    N, L = len(voiced_idx), stream.L
    mats = [window_matrix(w, N) for w in stream.windows]
    out = []
    for d in (range(L) if dims is None else dims):
        A, b = np.zeros((N, N), dtype=LD), np.zeros(N, dtype=LD)
        for i, coef in enumerate(stream.windows):
            width = len(coef)  # the DECLARED width, zero taps included
            lw = width // 2
            rw = width - lw - 1
            ivar = with_ivar(stream.var[state, i * L + d]).astype(LD)  # f64, then widened
            if i != 0:
                ivar = np.where((left < lw) | (right < rw), LD(0), ivar)
            mu = np.asarray(stream.mean, dtype=np.float64)[state, i * L + d].astype(LD)
            Ai, bi = normal_equations(mats[i], ivar[voiced_idx], mu[voiced_idx])
            A += Ai
            b += bi
        out.append((A, b))
    return voiced_idx, out


def solve(A, b):
    """Cholesky A = G G' and the two substitutions, in long double."""
    n = len(b)
    G = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = A[j:, j] - G[j:, :j] @ G[j, :j]
        G[j:, j] = col / np.sqrt(col[0])
    y = np.zeros(n, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - G[i, :i] @ y[:i]) / G[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - G[i + 1:, i] @ x[i + 1:]) / G[i, i]
    return x


def gv_switch_frames(stream: Stream, durations, voiced_idx):
    """[N] bool: the per-state gv_switch expanded by durations and filtered by the mask (mlpg.rs:128-133)."""
    durations = np.asarray(durations, dtype=np.int64)
    return np.repeat(np.asarray(stream.gv_switch).astype(bool), durations)[voiced_idx]


def gv_ascent(A, b, c, switch, gv_mean, gv_var, n_windows):
    """The GV ascent (mlpg.rs:168-292) in long double on the dense system: (parameters, min_i |obj_i - obj_{i-1}| /
    |obj_i|).  gv_mean is the stream's gv_mean[d] * gv_weight (mlpg.rs:135-137).  No switched-on frame: c unchanged
    and inf."""
    par = np.array(c, dtype=LD)
    n = len(par)
    switch = np.asarray(switch, dtype=bool)
    glen = int(switch.sum())
    if glen == 0:
        return par, float("inf")
    gv_mean, gv_var = LD(gv_mean), LD(gv_var)

    def calc_gv():
        m = par[switch].sum() / LD(glen)
        return m, ((par[switch] - m) ** 2).sum() / LD(glen)

    m, v = calc_gv()  # conv_gv
    par[switch] = np.sqrt(gv_mean / v) * (par[switch] - m) + m
    step, prev, w = LD(0.1), LD(0), LD(1) / LD(n_windows * n)
    diagA = np.diag(A)
    margin = float("inf")
    for i in range(1, 6):  # GV_MAX_ITERATION
        m, v = calc_gv()
        gvobj = LD(-0.5) * v * gv_var * (v - 2 * gv_mean)
        g = A @ par
        hmmobj = (w * par * (b - LD(0.5) * g)).sum()
        obj = -(hmmobj + gvobj)
        if i > 1:
            margin = min(margin, float(abs(obj - prev) / abs(obj)))
            if obj > prev:
                step *= LD(0.5)  # STEPDEC
            elif obj < prev:
                step *= LD(1.2)  # STEPINC
        dv = -2 * gv_var * (v - gv_mean) / LD(n)
        h = -w * diagA - LD(2) / LD(n * n) * (LD(n - 1) * gv_var * (v - gv_mean) + 2 * gv_var * (par - m) ** 2)
        par = par + step * (w * (b - g) + np.where(switch, dv * (par - m), LD(0))) / h
        prev = obj
    return par, margin


def norm_inf(M):
    M = np.abs(np.asarray(M, dtype=LD))
    if M.size == 0:
        return LD(0)
    return M.sum(axis=1).max() if M.ndim == 2 else M.max()


def backward_error(A, b, c):
    """||b - A c||inf / (||A||inf ||c||inf + ||b||inf) in long double; 0 when the residual is 0."""
    c = np.asarray(c, dtype=LD)
    r = norm_inf(b - A @ c)
    return 0.0 if r == 0 else float(r / (norm_inf(A) * norm_inf(c) + norm_inf(b)))


def cond_inf(A):
    """||A||inf ||A^-1||inf.  The inverse is LAPACK's in f64: with cond <= 1e8 it is good to ~1e-8 relative, and the
    number only scales a bound."""
    if len(A) == 0:
        return 0.0
    return float(np.linalg.cond(np.asarray(A, dtype=np.float64), np.inf))


def rel_inf(got, want):
    """||got - want||inf / ||want||inf (0 for two empty vectors)."""
    want = np.asarray(want, dtype=LD)
    if want.size == 0:
        return 0.0
    return float(norm_inf(np.asarray(got, dtype=LD) - want) / norm_inf(want))
