"""The synthesis filters as rational functions of z, in numpy.longdouble: the reference the vocoder is held to where no
golden of the reference reaches (orders other than 34, other alphas and frame periods, the MGLSA cascade).  numpy only:
no GPU, and of oracle/ only O.noise (the unvoiced excitation, which the goldens pin).  No recursion is restated here --
the oracle (oracle/jbo_hot.c) and the kernels (jb_vocoder.hip, jb_mglsa.hip) both restate mlsa.rs / mglsa.rs sample by
sample; this module evaluates the transfer function those recursions realise on a grid of the unit circle, takes the
impulse response by an inverse FFT and convolves it with the excitation.

With coefficients held constant the filters are linear and time-invariant.  Write a = alpha, and on |z| = 1

    Phi_1(z) = (1 - a^2) z^-1 / (1 - a z^-1),    A(z) = (z^-1 - a) / (1 - a z^-1),    Phi_k = Phi_1 A^(k-1).

Stage::Zero (mlsa.rs).  df1 (mlsa.rs:54-66) walks i = 5..1 and reads d12[i-1] BEFORE this sample's update of it, so
d11[i] = (1 - a^2) z^-1 / (1 - a z^-1) d12[i-1] = Phi_1 d12[i-1] and d12[i] = b_1 Phi_1 d12[i-1] = u^i w with
u = b_1 Phi_1 and w = d12[0].  The loop adds +P_i u^i w to x for odd i and -P_i u^i w for even i and stores the sum as
w: w = x - sum_{i>=1} P_i (-u)^i w, i.e. w sum_i P_i (-u)^i = x (P_0 = 1).  The output is w + sum_{i>=1} P_i u^i w, so

    df1 = R(b_1 Phi_1),    R(u) = sum_i P_i u^i / sum_i P_i (-u)^i.

df2 (mlsa.rs:69-79) is the same loop with fir() (mlsa.rs:127-163) in the place of b_1 Phi_1.  fir is fed d22[i-1] of
the PREVIOUS sample (the one-sample delay between Pade stages), x' = z^-1 x.  Inside, d[1] = (1 - a^2) / (1 - a z^-1)
x' = Phi_1 x, and d[k] <- (1 - a^2) rem + a d[k], rem <- -a rem + d[k]_old gives d[k] = A d[k-1]: d[k] = Phi_k x.  The
4-way unrolled body is that step taken four times (with its remainder loop for (nmcp - 2) % 4 taps); the result is
sum_{k=2}^{nmcp-1} b_k d[k].  With the input gain x *= exp(b_0) (vocoder/mod.rs:129-131):

    H(z) = exp(b_0) R(b_1 Phi_1) R(sum_{k=2}^{nmcp-1} b_k Phi_k),    b = mc2b(mc, a): b_last = mc_last, b_i = mc_i - a b_(i+1).

MGLSA (mglsa.rs:15-41), one stage: y = sum_{k=1}^{n-1} c_k d[k-1], out = x - y, then the line shifts and
d[0] <- a d[0] + (1 - a^2) out.  Read at the next sample d[0] = Phi_1 out; the in-place step d[i] += a (d[i+1] - d[i-1])
with d[i-1] already updated and the shift make d[k-1] = Phi_k out.  So out = x / (1 + sum c_k Phi_k), and with the input
gain x *= c_0 (vocoder/mod.rs:166)

    H(z) = c_0 (1 / (1 + sum_{k=1}^{n-1} c_k Phi_k))^stage.

Two facts reach the time-varying code without restating a recursion: b_0 enters as a per-sample input gain only, so if
mc_0 alone varies between frames the output is h * (e[n] exp(c_0[n])) with c_0[n] the interpolation schedule in closed
form (gain_schedule); and the excitation of an unvoiced frame is the noise stream."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53  # unit roundoff of f64, the arithmetic under test
NODATA = -1e10  # src/constants.rs:13
# mlsa.rs:31, the f64 nearest to each literal, widened
PPADE = tuple(LD(x) for x in (1.0, 0.4999391, 0.1107098, 0.01369984, 0.0009564853, 0.00003041721))
PI = LD(4) * np.arctan(LD(1))
ALIAS_TOL = 1e-16  # of the response's peak: N against 2N, and the tail
N_MIN, N_MAX = 1 << 11, 1 << 19


def wide_enough():
    """numpy.longdouble carries more digits than f64 (x87 extended: eps 1.08e-19)."""
    return np.finfo(LD).eps <= 2.0 ** -63


def mc2b(mc, alpha):
    """cepstrum.rs:139-149 in long double."""
    b = np.array(mc, dtype=LD)
    a = LD(alpha)
    for i in range(len(b) - 2, -1, -1):
        b[i] = b[i] - a * b[i + 1]
    return b


def unit_circle(N):
    """z^-1 at the N grid points, long double."""
    return np.exp(CLD(-2j) * PI * np.arange(N, dtype=LD) / LD(N))


def warped_sum(c, alpha, zi):
    """sum_{k >= 1} c[k - 1] Phi_k on the grid zi (c = the coefficients of Phi_1, Phi_2, ...)."""
    a = LD(alpha)
    den = 1 - a * zi
    phi = (1 - a * a) * zi / den
    ap = (zi - a) / den
    s = np.zeros(len(zi), dtype=CLD)
    for ck in np.asarray(c, dtype=LD):
        s += ck * phi
        phi = phi * ap
    return s


def pade(u):
    num, den = np.zeros(len(u), dtype=CLD), np.zeros(len(u), dtype=CLD)
    p, q = np.ones(len(u), dtype=CLD), np.ones(len(u), dtype=CLD)
    for P in PPADE:
        num += P * p
        den += P * q
        p, q = p * u, q * (-u)
    return num / den


def mlsa_response(b, alpha, N, gain=True):
    """Stage::Zero on the N-point grid.  gain=False leaves exp(b_0) out (the gain-ramp cases apply it per sample)."""
    b = np.asarray(b, dtype=LD)
    zi = unit_circle(N)
    H = pade(warped_sum(b[1:2], alpha, zi))
    if len(b) > 2:
        H = H * pade(warped_sum(np.concatenate(([LD(0)], b[2:])), alpha, zi))
    return H * np.exp(b[0]) if gain else H


def mglsa_response(c, alpha, stage, N):
    """Stage::NonZero on the N-point grid."""
    c = np.asarray(c, dtype=LD)
    zi = unit_circle(N)
    return c[0] * (1 / (1 + warped_sum(c[1:], alpha, zi))) ** int(stage)


def _ifft(H):
    h = np.fft.ifft(H)
    assert h.dtype == CLD, h.dtype  # numpy.fft keeps long double (pocketfft, numpy >= 2)
    return h


def impulse_response(response, n_min=N_MIN):
    """(h [N] long double, N, dict of margins).  `response(N)` is H on the N-point grid.  The grid is doubled until the
    response on N points and on 2N points agree to ALIAS_TOL of the peak and what lies behind N is under ALIAS_TOL of
    the peak: h_N[n] = sum_m h[n + m N], so both say that nothing of h wraps around."""
    N = n_min
    h = _ifft(response(N))
    while True:
        h2 = _ifft(response(2 * N))
        peak = float(np.abs(h2.real).max())
        agree = float(np.abs(h.real - h2.real[:N]).max()) / peak
        tail = float(np.abs(h2.real[N:]).max()) / peak
        imag = float(np.abs(h2.imag).max()) / peak
        if agree <= ALIAS_TOL and tail <= ALIAS_TOL:
            assert imag <= ALIAS_TOL, imag  # H is Hermitian: what is left is the transform's rounding
            return h.real.astype(LD), N, dict(N=N, agree=agree, tail=tail, imag=imag, peak=peak)
        assert 2 * N <= N_MAX, ("the response does not decay", N, agree, tail)
        N, h = 2 * N, h2


def convolve(x, h):
    """The first len(x) samples of x * h, long double, by FFT on a grid that holds the whole linear convolution."""
    x, h = np.asarray(x, dtype=LD), np.asarray(h, dtype=LD)
    if len(x) == 0:
        return np.zeros(0, dtype=LD)
    M = 1 << int(np.ceil(np.log2(len(x) + len(h))))
    X, Hh = np.fft.rfft(x, M), np.fft.rfft(h, M)
    assert X.dtype == CLD
    return np.fft.irfft(X * Hh, M)[:len(x)]


# ---- excitation -------------------------------------------------------------------------------------------------
def pitch_of(lf0, fs):
    """The period the vocoder takes from a voiced frame's lf0 (vocoder/mod.rs:73-77; the clamp is not reached here)."""
    assert 2.995732273553991 < lf0 < 9.903487552536127
    return float(fs) / float(np.exp(np.float64(lf0)))


def pulse_positions(p, n):
    """Constant pitch p from a start with pitch_counter = p (excitation.rs:25-33,90-96): a pulse on sample 0, then
    wherever 1 + m >= k p first holds, m = ceil(k p) - 1.  The loop keeps the counter by repeated subtraction in f64:
    k p must stay clear of an integer for the two to agree, which is asserted (1e-6)."""
    pos = [0]
    k = 1
    while True:
        kp = k * p
        assert abs(kp - round(kp)) >= 1e-6, (p, k)
        m = int(np.ceil(kp)) - 1
        if m >= n:
            break
        pos.append(m)
        k += 1
    return np.asarray(pos, dtype=np.int64)


def excitation(voiced, fperiod, p, nlpf, noise):
    """[T * fperiod] f64: the excitation of frames `voiced` [T] bool at constant pitch p, without a ring buffer
    (nlpf = 0) or with nlpf = 1 and lpf = [1.0], where the ring buffer of one cell passes pulse and noise through.
    Voiced run: pulses of sqrt(p), the first on the run's first sample (the pitch restarts after an unvoiced frame,
    excitation.rs:25-33).  Unvoiced frame: the noise stream -- drawn on unvoiced samples only when nlpf = 0, on every
    sample when nlpf >= 1 (excitation.rs:87-88 against 69).  `noise`: at least T * fperiod samples of O.noise."""
    voiced = np.asarray(voiced, dtype=bool)
    T = len(voiced)
    e = np.zeros(T * fperiod)
    edges = np.flatnonzero(np.diff(np.concatenate(([False], voiced, [False])).astype(np.int8)))
    for first, past in zip(edges[0::2], edges[1::2]):
        n = (past - first) * fperiod
        e[first * fperiod + pulse_positions(p, n)] = np.sqrt(np.float64(p))
    un = np.repeat(~voiced, fperiod)
    if nlpf == 0:
        e[un] = noise[:int(un.sum())]
    else:
        e[un] = noise[:T * fperiod][un]
    return e


def gain_schedule(b0, fperiod):
    """c_0 at every sample, [T * fperiod] long double, from the per-frame b_0 [T] (vocoder/mod.rs:79-89,116-140):
    frame 0 is flat; sample i of frame t >= 1 uses b0[t-1] + i (b0[t] - b0[t-1]) / fperiod -- the target is reached
    only at the next frame's sample 0."""
    b0 = np.asarray(b0, dtype=LD)
    prev = np.concatenate((b0[:1], b0[:-1]))
    i = np.arange(fperiod, dtype=LD) / LD(fperiod)
    return (prev[:, None] + i[None, :] * (b0 - prev)[:, None]).reshape(-1)


# ---- a case -> its PCM -----------------------------------------------------------------------------------------
def case_response(case, coef=None):
    """(h, N, margins) of a case (tests/mlsa_cases.py).  MGLSA: from `coef` (the coefficients the filter was given --
    the oracle's or the device's own, the LSP conversion being ill-conditioned)."""
    if case.stage:
        c = np.asarray(coef, dtype=np.float64)
        return impulse_response(lambda N: mglsa_response(c, case.alpha, case.stage, N))
    b = mc2b(case.mc[0], case.alpha)
    return impulse_response(lambda N: mlsa_response(b, case.alpha, N, gain=not case.ramp))


def expected_pcm(case, nlpf, noise, coef=None, response=None):
    """[T * fperiod] long double: the PCM of `case` with the excitation of `nlpf` (0 or 1)."""
    h = (response or case_response(case, coef))[0]
    e = excitation(case.voiced, case.fperiod, pitch_of(case.lf0, case.fs), nlpf, noise).astype(LD)
    if case.ramp:
        b0 = np.array([mc2b(row, case.alpha)[0] for row in case.mc], dtype=LD)
        e = e * np.exp(gain_schedule(b0, case.fperiod))
    return convolve(e, h) * LD(case.volume)


# ---- the post-filter's energy (coefficients.rs:75-78) ------------------------------------------------------------
def b2mc(b, alpha):
    """coefficients.rs:65-73 in long double."""
    b = np.asarray(b, dtype=LD)
    mc = b.copy()
    for i in range(len(b) - 2, -1, -1):
        mc[i] = b[i] + LD(alpha) * b[i + 1]
    return mc


def reversed_energy(b, alpha, M):
    """What b2en sums, without its truncation to 576 terms: b2en is the energy of the impulse response of
    exp(C(z)), C the linear-frequency cepstrum that freqt(-alpha) makes of mc = b2mc(b).  The reference's freqt feeds
    self[i] in ASCENDING order (cepstrum.rs:159) where the recursion wants the highest coefficient first, so C is the
    transform of the REVERSED sequence: C(z) = sum_k mc[n-1-k] A(z)^k.  By Parseval the energy is the mean over the
    unit circle of |exp(C)|^2 = exp(2 Re C), here on M points in long double."""
    mc = b2mc(b, alpha)[::-1]
    zi = unit_circle(M)
    ap = (zi - LD(alpha)) / (1 - LD(alpha) * zi)
    Cw, pw = np.zeros(M, dtype=CLD), np.ones(M, dtype=CLD)
    for ck in mc:
        Cw += ck * pw
        pw = pw * ap
    return np.exp(2 * Cw.real).sum() / LD(M)


def postfiltered_b(b, alpha, beta):
    """The coefficients whose energy postfilter_mcp compares with the input's (cepstrum.rs:28-32), long double."""
    b2 = np.array(b, dtype=LD)
    b2[1] -= LD(beta) * LD(alpha) * b2[2]
    b2[2:] *= 1 + LD(beta)
    return b2
