"""The cepstral rule of include/jbonsai_amd.h ("Cepstral features") restated twice in numpy from given log-mel frames,
and the inputs of its tests.

model_ld follows the rule in numpy.longdouble (a 64-bit mantissa on x86-64); model_f64 in float64 with numpy's own
tools: matrix products, numpy.mean / numpy.var, numpy.convolve.  model_ld also returns each element's magnitude bound:
the same pipeline run on absolute values -- |D| |L|, the lifter, |c| + |mu|, the same 1 / sigma, sum |s_q| | . | -- so
that the cancellation in c - mu does not hide in a small denominator.  The tests hold the library to

    e(X) = max over t, column of |X - X_ld| / bound  <=  GATE * e(model_f64)

so the bound is the error of an ordinary float64 evaluation of the same frames in another summation order, not a
number picked by hand.
"""
import functools

import numpy as np

from tests import fbank_ref

LD = np.longdouble
GATE = fbank_ref.GATE  # another summation order at the same precision: a small factor, not orders
NONE, MEAN, MEAN_VAR = 0, 1, 2
have_long_double = fbank_ref.have_long_double


def dct_ld(n_mels, n_ceps):
    """[n_ceps, n_mels] the orthonormal DCT-II in long double (the angle's integer part reduced first, exactly)."""
    pi = np.arccos(LD(-1))
    N = LD(n_mels)
    k = (np.arange(n_ceps)[:, None] * (2 * np.arange(n_mels)[None, :] + 1)) % (4 * n_mels)
    D = np.sqrt(LD(2) / N) * np.cos(pi * k.astype(LD) / (LD(2) * N))
    if n_ceps:
        D[0, :] = np.sqrt(LD(1) / N)
    return D


def lifter_ld(n_ceps, Q):
    if not Q > 0:
        return np.ones(n_ceps, dtype=LD)
    pi = np.arccos(LD(-1))
    return LD(1) + (LD(Q) / LD(2)) * np.sin(pi * np.arange(n_ceps).astype(LD) / LD(Q))


def delta_kernel_ld(q, N):
    """s_q[-qN..qN] in long double: s_0 = [1], s_q = s_{q-1} * g, the products added in the order a, then k."""
    den = LD(0)
    for j in range(-N, N + 1):
        den += LD(j) * LD(j)
    cur = [LD(1)]
    for _ in range(q):
        nxt = [LD(0)] * (len(cur) + 2 * N)
        for a, v in enumerate(cur):
            for k in range(-N, N + 1):
                nxt[a + k + N] += v * (LD(k) / den)
        cur = nxt
    return np.array(cur, dtype=LD)


def _rows(c, order, N, kernels, dtype):
    """[T, d (order + 1)]: c and its delta rows with clamped ends."""
    T = c.shape[0]
    out = [c]
    for q in range(1, order + 1):
        s = kernels[q]
        acc = np.zeros_like(c)
        for j in range(-q * N, q * N + 1):
            acc = acc + s[j + q * N] * c[np.clip(np.arange(T) + j, 0, T - 1)]
        out.append(acc)
    return np.concatenate(out, axis=1).astype(dtype)


def model_ld(L, n_ceps, lifter=22.0, order=0, N=2, cmvn=NONE, var_floor=0.0):
    """(rows [T, width], bound [T, width]) in long double."""
    L = np.asarray(L, dtype=LD)
    T, n_mels = L.shape
    if n_ceps:
        D, l = dct_ld(n_mels, n_ceps), lifter_ld(n_ceps, lifter)
        c = (L @ D.T) * l[None, :]
        b = (np.abs(L) @ np.abs(D).T) * np.abs(l)[None, :]
    else:
        c, b = L.copy(), np.abs(L)
    if T and cmvn != NONE:
        mu = c.sum(axis=0) / LD(T)
        c = c - mu[None, :]
        b = b + np.abs(mu)[None, :]
        if cmvn == MEAN_VAR:
            var = (c * c).sum(axis=0) / LD(T)
            isd = LD(1) / np.sqrt(np.maximum(var, LD(var_floor or 2.0 ** -52)))
            c = c * isd[None, :]
            b = b * isd[None, :]
    ker = {q: delta_kernel_ld(q, N) for q in range(1, order + 1)}
    return _rows(c, order, N, ker, LD), _rows(b, order, N, {q: np.abs(s) for q, s in ker.items()}, LD)


def model_f64(L, n_ceps, lifter=22.0, order=0, N=2, cmvn=NONE, var_floor=0.0):
    """rows [T, width] in float64: matrix products, numpy.mean / var, numpy.convolve."""
    L = np.asarray(L, dtype=np.float64)
    T, n_mels = L.shape
    if n_ceps:
        c = (L @ dct_ld(n_mels, n_ceps).astype(np.float64).T) * lifter_ld(n_ceps, lifter).astype(np.float64)[None, :]
    else:
        c = L.copy()
    if T and cmvn != NONE:
        c = c - np.mean(c, axis=0)[None, :]
        if cmvn == MEAN_VAR:
            c = c / np.sqrt(np.maximum(np.var(c, axis=0), var_floor or 2.0 ** -52))[None, :]
    out = [c]
    g = np.arange(-N, N + 1, dtype=np.float64) / float(sum(j * j for j in range(-N, N + 1)))
    s = np.ones(1)
    for q in range(1, order + 1):
        s = np.convolve(s, g)
        pad = np.pad(c, ((q * N, q * N), (0, 0)), mode="edge") if T else c
        # (numpy.convolve flips its kernel: out[t] = sum_j s[j] pad[t + qN + j] is a correlation)
        out.append(np.stack([np.convolve(pad[:, i], s[::-1], mode="valid") for i in range(c.shape[1])], axis=1)
                   if T else c)
    return np.concatenate(out, axis=1)


def rel_err(X, X_ld, bound):
    """e(X): every element enters, each divided by its own magnitude bound."""
    X = np.asarray(X, dtype=LD)
    assert X.shape == X_ld.shape
    if X.size == 0:
        return 0.0
    assert np.all(bound > 0)
    return float(np.max(np.abs(X - X_ld) / bound))


@functools.lru_cache(maxsize=None)
def logmel(n_mels, frames=300, hz=16000):
    """[frames, n_mels] f64 log-mel frames of fbank_ref.gate_signal through jb_fbank_host: all finite, the silent
    frames in front at the floor ln(2^-52).  Shared and read-only."""
    import jbonsai_amd as J

    wl, hop, _ = fbank_ref.geometry(hz)
    x = fbank_ref.gate_signal(hz, (frames - 1) * hop + wl)
    L = J.fbank_host(x, hz, J.fbank(n_mels=n_mels, f64=True))
    assert L.shape == (frames, n_mels) and L.dtype == np.float64 and np.all(np.isfinite(L))
    floor = float(np.log(LD(2.0 ** -52)))
    # (narrow low filters on a coarse grid cover no bin: their columns sit at the floor throughout)
    covered = fbank_ref.filterbank_ld(hz, fbank_ref.geometry(hz)[2], n_mels).sum(axis=1) > 0
    assert covered.sum() >= min(n_mels, 16) and np.all(L[:, ~covered] == floor)
    assert np.all(L[:4] == floor) and np.all(L[8:][:, covered] > floor)
    L.setflags(write=False)
    return L


def no_arithmetic(n_mels, n_ceps, delta_order=0, cmvn="none", **_):
    """The rows are the log-mel values themselves (no DCT, or the 1 x 1 one, which is [[1]] with l_0 = 1; no CMVN, no
    deltas): nothing rounds, so every model's error is exactly 0 and the gate asks for exactly that."""
    return (n_ceps == 0 or n_mels == 1) and delta_order == 0 and cmvn == "none"


def errors(X, L, **kw):
    """(e(X), e(model_f64)) of rows X of the frames L under the options kw of J.mfcc."""
    args = (kw["n_ceps"], kw.get("lifter", 22.0), kw.get("delta_order", 0), kw.get("delta_window", 2),
            {"none": NONE, "mean": MEAN, "mean_var": MEAN_VAR}[kw.get("cmvn", "none")], kw.get("var_floor", 0.0))
    X_ld, bound = model_ld(L, *args)
    return rel_err(X, X_ld, bound), rel_err(model_f64(L, *args), X_ld, bound)


def gate(run, L, who, **kw):
    """run(L, opts) -> rows, f64: under the gate against the two models; returns (e, e64)."""
    import jbonsai_amd as J

    X = run(L, J.mfcc(f64=True, **kw))
    e, e64 = errors(X, L, **kw)
    print(f"{who} T {L.shape[0]} n_mels {L.shape[1]} {kw}: e(model_f64) {e64:.2e}  e {e:.2e}  "
          f"ratio {e / e64 if e64 else 0:.2f}")
    assert X.dtype == np.float64
    if no_arithmetic(L.shape[1], **kw):
        assert e == 0.0 and e64 == 0.0
    else:
        # (one filter alone with the dyadic table of N = 1 can come out exact in every model: then e must be 0 too,
        # which e <= GATE * 0 says; everywhere else a float64 model that is exact would make the bound vacuous)
        assert (0 < e64 or L.shape[1] == 1) and e64 < 1e-14 and e <= GATE * e64
    return e, e64
