"""The frame-to-frame part of the vocoder in numpy.longdouble: pitch interpolation, the low-pass mixed excitation and
the synthesis filters with every coefficient interpolating.  It is the reference that tests/test_vocoder_tv_ref.py holds
the oracle to and tests/test_gpu_vocoder_tv.py holds the kernels to, on the table of tests/vocoder_tv_cases.py.  numpy
only: no GPU, and of oracle/ nothing but the noise stream a caller hands in (O.noise, which the goldens pin).

Why it is independent.  The oracle (oracle/jbo_hot.c) and the kernels (jb_vocoder.hip, jb_mglsa.hip) restate
excitation.rs, mlsa.rs and mglsa.rs: a ring buffer that scatters, fir()'s unrolled `rem` chain, dff()'s in-place sweep.
None of the three is restated here.

  * Filters.  tests/mlsa_ref.py derives that the delay lines hold time-invariant images of a stage's own signal --
    fir(): d[k] = Phi_k v, dff(): d[k-1] = Phi_k out, df1: d11[i] = Phi_1 d12[i-1] -- and that the coefficients enter
    only as the weights of a sum over them.  That holds sample by sample whatever the weights do, so with phi_k the
    impulse response of Phi_k = Phi_1 A^(k-1) (strictly causal: every Phi_k carries the z^-1 of Phi_1)

      MGLSA, one stage     out[n] = x[n] - sum_{k=1}^{m-1} c_k(n) (phi_k * out)[n]        cascaded; x[n] = c_0(n) e[n]
      Stage::Zero, df1     v_i[n] = b_1(n) (phi_1 * v_(i-1))[n],                 v_0 = w   (d12[i] keeps the product
                                                                                            with THIS sample's b_1)
                   df2     v_i[n] = sum_{k=2}^{m-1} b_k(n) (phi_k * v_(i-1))[n],  v_0 = w   (the z^-1 between Pade
                                                                                            stages is Phi_1's own)
                   both    w[n] = x[n] - sum_{i=1}^{5} P_i (-1)^i v_i[n],   out[n] = w[n] + sum_i P_i v_i[n]
                           x[n] = exp(b_0(n)) e[n] in front of df1, df1's out in front of df2

    all explicit in n.  The phi_k are realised as ONE dense matrix: s[n] = M s[n-1] + g u[n-1] with s_k = phi_k * u,
    from the first-order sections s_1[n] = a s_1[n-1] + (1 - a^2) u[n-1], s_k[n] + a s_(k-1)[n] = a s_k[n-1] +
    s_(k-1)[n-1]: (I + a L) s[n] = (a I + L) s[n-1] + (1 - a^2) e_1 u[n-1], L the shift, (I + a L)^-1 = sum (-a)^j L^j,
    so M is lower-triangular Toeplitz with a on the diagonal and (1 - a^2) (-a)^(d-1) on sub-diagonal d, and g_k =
    (1 - a^2) (-a)^(k-1) (warp_operator; checked against mlsa_ref.warped_sum on the unit circle).
  * Coefficients.  c(n) is the schedule of vocoder/mod.rs:116-140,156-175 in closed form (schedule): sample i of frame
    t uses prev + i (c[t] - prev) / fperiod, prev = c[t-1], or the FIRST row for t = 0 (mod.rs:87-88,103: unfiltered, so
    with beta > 0 frame 0 already moves); the target is reached at the next frame's sample 0.
  * Excitation.  The ring buffer scatters what this gathers (mixed_excitation):
        e[n] = noise[n - D] [n >= D] + sum_{i=0}^{nlpf-1} c[n - i] lpf_frame(n-i)[i],   D = (nlpf - 1) div 2,
    c[m] = pulse[m] - noise[m] in a voiced frame and 0 in an unvoiced one; the noise is drawn on every sample.
    nlpf = 0: the pulse on voiced samples, the next value of the noise stream on unvoiced ones.
  * Pitch.  The one thing that is a walk by definition (excitation.rs:25-33,73-81,102-104): the counter.  It is walked
    in long double with the period of a sample in closed form, start + i inc (the f64 loop accumulates it), and the
    smallest |counter - p| over all comparisons is returned: the f64 loops agree with this one only when every
    comparison stays clear of a tie.

Volume is applied last."""
from __future__ import annotations

import numpy as np

from tests import mlsa_ref as R

LD = R.LD
MIN_LF0, MAX_LF0 = 2.995732273553991, 9.903487552536127  # src/constants.rs:4-6
PADE = np.array(R.PPADE[1:], dtype=LD)                                   # P_1 .. P_5
PADE_ALT = PADE * np.array([-1, 1, -1, 1, -1], dtype=LD)                 # P_i (-1)^i


# ---- pitch and pulses ---------------------------------------------------------------------------------------------
def periods(lf0, fs):
    """[T] long double: the period of every frame (vocoder/mod.rs:73-77): NODATA -> 0, lf0 clamped."""
    lf0 = np.asarray(lf0, dtype=np.float64).reshape(-1)
    p = np.zeros(len(lf0), dtype=LD)
    v = lf0 != R.NODATA
    p[v] = LD(fs) / np.exp(np.clip(lf0[v], MIN_LF0, MAX_LF0).astype(LD))
    return p


def pulses(p, fperiod):
    """(pulse [T * fperiod] long double, margin): sqrt(period) where the counter fires, 0 elsewhere, from the frames'
    periods p [T] (0: unvoiced).  A voiced frame behind a voiced one glides from the old period to the new one, which
    it reaches only by the snap at its end; behind an unvoiced one (or at the start) it is flat and the counter restarts
    at p, so the first sample fires.  margin: the smallest |counter - period| over all comparisons."""
    p = np.asarray(p, dtype=LD)
    out = np.zeros(len(p) * fperiod, dtype=LD)
    margin, prev, counter, one = float("inf"), LD(0), LD(0), LD(1)
    steps = np.arange(fperiod, dtype=LD)
    for t, cur in enumerate(p):
        if prev != 0 and cur != 0:
            at = prev + steps * ((cur - prev) / LD(fperiod))
        else:
            at = np.full(fperiod, cur, dtype=LD)
            counter = cur
        if cur != 0:
            for i in range(fperiod):
                counter = counter + one
                margin = min(margin, float(abs(counter - at[i])))
                if counter >= at[i]:
                    counter = counter - at[i]
                    out[t * fperiod + i] = np.sqrt(at[i])
        prev = cur
    return out, margin


# ---- mixed excitation ---------------------------------------------------------------------------------------------
def mixed_excitation(pulse, voiced, fperiod, lpf, noise):
    """[T * fperiod] long double.  pulse: pulses()'s; voiced [T] bool; lpf [T][nlpf] (nlpf = 0: no ring buffer);
    noise: at least T * fperiod samples of the stream."""
    voiced = np.asarray(voiced, dtype=bool)
    N = len(voiced) * fperiod
    vs = np.repeat(voiced, fperiod)
    lpf = np.zeros((len(voiced), 0)) if lpf is None else np.asarray(lpf, dtype=LD).reshape(len(voiced), -1)
    nlpf = lpf.shape[1]
    e = np.zeros(N, dtype=LD)
    if nlpf == 0:
        e[vs] = pulse[vs]
        e[~vs] = np.asarray(noise[:int((~vs).sum())], dtype=LD)
        return e
    nz = np.asarray(noise[:N], dtype=LD)
    D = (nlpf - 1) // 2
    e[D:] = nz[:max(N - D, 0)]
    c = np.where(vs, pulse - nz, LD(0))
    frame = np.arange(N) // fperiod
    for i in range(min(nlpf, N)):
        e[i:] += c[:N - i] * lpf[frame[:N - i], i]
    return e


def excitation(lf0, fs, fperiod, lpf, noise):
    """(e [T * fperiod] long double, margin) of one utterance from its lf0 track."""
    p = periods(lf0, fs)
    pulse, margin = pulses(p, fperiod)
    return mixed_excitation(pulse, p != 0, fperiod, lpf, noise), margin


# ---- coefficients -------------------------------------------------------------------------------------------------
def schedule(rows, first, fperiod):
    """[T * fperiod][m] long double: the coefficients every sample is filtered with, from the frames' target rows
    [T][m] and the row the first frame starts from [m]."""
    rows = np.asarray(rows, dtype=LD)
    prev = np.concatenate((np.asarray(first, dtype=LD)[None, :], rows[:-1]))
    i = np.arange(fperiod, dtype=LD)
    out = prev[:, None, :] + i[None, :, None] * ((rows - prev) / LD(fperiod))[:, None, :]
    return out.reshape(len(rows) * fperiod, rows.shape[1])


def zero_rows(mc, alpha, beta):
    """(rows [T][m], first [m]) long double of Stage::Zero from a mel-cepstrum track: mc2b, behind the long-double
    post-filter of tests/coef_ref.py where beta > 0; the first row is unfiltered."""
    mc = np.asarray(mc, dtype=np.float64)
    first = R.mc2b(mc[0], alpha)
    if beta > 0.0 and mc.shape[1] > 2:
        from tests import coef_ref
        return np.array([coef_ref.postfilter(row, alpha, beta)["b"] for row in mc], dtype=LD), first
    return np.array([R.mc2b(row, alpha) for row in mc], dtype=LD), first


# ---- the warped delay line as one matrix --------------------------------------------------------------------------
def warp_operator(K, alpha):
    """(M [K][K], g [K]) long double with s[n] = M s[n-1] + g u[n-1] for s_k = phi_k * u, k = 1..K."""
    a = LD(alpha)
    d = np.arange(K)[:, None] - np.arange(K)[None, :]
    M = np.where(d > 0, (1 - a * a) * np.power(-a, np.maximum(d - 1, 0)), np.where(d == 0, a, LD(0))).astype(LD)
    g = ((1 - a * a) * np.power(-a, np.arange(K))).astype(LD)
    return M, g


def _stack(xs, cs):
    """Utterances of different lengths side by side: x [U][N], c [U][N][m], zero input and the last row behind an end."""
    N, m = max(len(x) for x in xs), cs[0].shape[1]
    x, c = np.zeros((len(xs), N), dtype=LD), np.zeros((len(xs), N, m), dtype=LD)
    for u, (xu, cu) in enumerate(zip(xs, cs)):
        assert len(xu) == len(cu) and len(xu) > 0
        x[u, :len(xu)], c[u, :len(xu)], c[u, len(xu):] = xu, cu, cu[-1]
    return x, c


def mlsa_tv(es, bs, alpha):
    """Stage::Zero with per-sample coefficients.  es: excitations [N_u]; bs: schedules [N_u][m]; -> list of [N_u]."""
    x, b = _stack(es, bs)
    U, N, m = b.shape
    a, K = LD(alpha), m - 1
    x = x * np.exp(b[:, :, 0])
    Mt, g = warp_operator(K, alpha)
    Mt = np.ascontiguousarray(Mt.T)
    s1, v1 = np.zeros((U, 5), dtype=LD), np.zeros((U, 5), dtype=LD)        # v: [w, v_1 .. v_4] of the sample before
    s2, v2 = np.zeros((U, 5, K), dtype=LD), np.zeros((U, 5), dtype=LD)
    out = np.zeros((U, N), dtype=LD)
    for n in range(N):
        s1 = a * s1 + (1 - a * a) * v1
        v = s1 * b[:, n, 1:2]
        w = x[:, n] - v @ PADE_ALT
        y = w + v @ PADE
        v1[:, 0], v1[:, 1:] = w, v[:, :4]
        if K >= 2:
            s2 = s2 @ Mt + v2[:, :, None] * g
            v = np.einsum("uik,uk->ui", s2[:, :, 1:], b[:, n, 2:])
            w = y - v @ PADE_ALT
            y = w + v @ PADE
            v2[:, 0], v2[:, 1:] = w, v[:, :4]
        out[:, n] = y
    return [out[u, :len(e)] for u, e in enumerate(es)]


def mglsa_tv(es, cs, alpha, stage):
    """The MGLSA cascade with per-sample coefficients, same shapes as mlsa_tv."""
    x, c = _stack(es, cs)
    U, N, m = c.shape
    x = x * c[:, :, 0]
    Mt, g = warp_operator(m - 1, alpha)
    Mt = np.ascontiguousarray(Mt.T)
    s, prev = np.zeros((U, stage, m - 1), dtype=LD), np.zeros((U, stage), dtype=LD)
    out = np.zeros((U, N), dtype=LD)
    for n in range(N):
        s = s @ Mt + prev[:, :, None] * g
        y = np.einsum("ujk,uk->uj", s, c[:, n, 1:])
        prev = x[:, n, None] - np.cumsum(y, axis=1)  # stage j takes stage j-1's output of this sample
        out[:, n] = prev[:, -1]
    return [out[u, :len(e)] for u, e in enumerate(es)]


def synthesize(es, rows, firsts, fperiod, alpha, volume, stage=0):
    """PCM [N_u] long double of a batch of utterances: excitations, per-frame target rows [T_u][m], first rows [m]."""
    cs = [schedule(r, f, fperiod) for r, f in zip(rows, firsts)]
    out = mglsa_tv(es, cs, alpha, stage) if stage else mlsa_tv(es, cs, alpha)
    return [o * LD(volume) for o in out]
