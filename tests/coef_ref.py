"""The two kernels that turn a spectrum frame into filter coefficients, restated in extended precision: the reference
that tests/test_coef_ref.py holds the oracle to and tests/test_gpu_coef_ref.py holds k_postfilter / k_pf_table
(jb_postfilter.hip) and k_stage_coef (jb_mglsa.hip) to.  numpy (and mpmath where it imports) only: no GPU, no oracle.

Post-filter (cepstrum.rs:23-37,153-186, coefficients.rs:65-78), numpy.longdouble.  postfilter_mcp compares the energy
of two impulse responses, b2en(b) = sum(c2ir(freqt(b2mc(b), 575, -alpha), 576)^2), before and after the emphasis of b,
and moves b[0] by half the log of their ratio.  freqt is followed as written -- it is fed its input in ASCENDING order
(cepstrum.rs:159) -- and, being linear with a zero start state, is a constant [576][nmcp] operator of (nmcp, alpha),
built once (freqt_operator).  A row then costs one matrix-vector product and c2ir's 576 dot products.

The closed form that keeps this from being the recurrence retyped (closed_form_ir): with w = z^-1 on the unit circle
and t = (w + a) / (1 + a w), a the alpha freqt is called with, G(w) = sum_k mc[n-1-k] t^k has freqt's outputs as its
Taylor coefficients in w, and exp(G) has c2ir's.  Radius 1: a radius of 0.9 would amplify the transform's rounding by
0.9^-576.  N = 32768: the coefficients decay like k^(n-2) |a|^k, and at order 64 and alpha 0.77 what wraps around a
grid of 8192 points is still 1e-10 of the peak (1e-17 at 16384).

Stage::NonZero (lsp.rs:27-165, generalized.rs:6-38, cepstrum.rs:69-103,139-149, mod.rs:92-106,148-156), written once
over a small number kit (conversion, cos, exp, log, sqrt, pi) and run in numpy.longdouble (LDK) and, where mpmath
imports, at 50 digits (mp_kit()).  stage_coefficients records every comparison check_lsp_stability makes with its
margin |tmp - min|, so that a table can assert that f64 and the reference take the same branches.  lsp2lpc has a
closed form too (lsp2lpc_closed): the recursion realises A(z) = prod (1 - 2 cos(w_i) z^-1 + z^-2) over the
even-indexed entries and B(z) over the odd-indexed ones, times (1 + z^-1) and (1 - z^-1) for an even count and 1 and
(1 - z^-1)(1 + z^-1) for an odd one, and returns the first m + 1 coefficients of (A + B) / 2.  ALL m entries of the
buffer count as frequencies, the gain slot included, as the reference reads them.

The gate both test files share is within(): e_got <= 4 e_oracle + floor, the project's margin for re-associated sums
(tests/test_gpu_mlpg_dense.py)."""
from __future__ import annotations

import functools

import numpy as np

from tests import mlsa_ref as M

LD = np.longdouble
U = M.U
IRLENG = 576  # coefficients.rs:76
wide_enough = M.wide_enough

PF_FLOOR_GAIN = 64 * U   # times max(1, |b'[0]|): the shift is the log of a ratio of two 576-term sums
PF_FLOOR_REST = 16 * U   # times max |b'|: b'[1:] is one multiplication and the b2mc / mc2b round trip
STAGE_FLOOR = 64 * U     # relative, inf-norm over the row


def within(e_got, e_oracle, floor, factor=4.0):
    """The gate: e_got <= factor e_oracle + floor.  e_oracle is the oracle's worst error over the rows of the class
    (never one row's lucky zero); the factor is 4 unless a class states another one with its cause."""
    return bool(e_got <= factor * e_oracle + floor)


# ---- post-filter ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def freqt_operator(nmcp, alpha):
    """[576][nmcp] long double: column i is freqt(e_i, 575, alpha) (cepstrum.rs:153-173), the recurrence run on all unit
    inputs side by side.  `alpha` is the argument freqt gets (b2en passes -alpha of the voice)."""
    a = LD(alpha)
    aa = 1 - a * a
    g = np.zeros((IRLENG, nmcp), dtype=LD)
    eye = np.eye(nmcp, dtype=LD)
    for i in range(nmcp):
        f = g.copy()
        g[0] = eye[i] + a * f[0]
        g[1] = aa * f[0] + a * f[1]
        for j in range(2, IRLENG):
            g[j] = f[j - 1] + a * (f[j] - g[j - 1])
    g.setflags(write=False)
    return g


def c2ir(g, n=IRLENG):
    """cepstrum.rs:175-186: ir[0] = exp(g[0]), n ir[n] = sum_{k=1..n} k g[k] ir[n-k]."""
    g = np.asarray(g, dtype=LD)
    kg = np.arange(len(g), dtype=LD) * g
    ir = np.zeros(n, dtype=LD)
    ir[0] = np.exp(g[0])
    for i in range(1, n):
        k = min(len(g) - 1, i)
        ir[i] = np.dot(kg[1:k + 1], ir[i - k:i][::-1]) / LD(i)
    return ir


def impulse_response(b, alpha):
    """What b2en squares and sums (coefficients.rs:75-78), [576] long double."""
    b = np.asarray(b, dtype=LD)
    return c2ir(freqt_operator(len(b), -float(alpha)) @ M.b2mc(b, alpha))


def tail_over_peak(ir):
    """How much of the response the truncation at 576 still sees: the last 16 samples against the peak."""
    return float(np.abs(ir[-16:]).max() / np.abs(ir).max())


def postfilter(c, alpha, beta):
    """One frame: dict(b = what Batch.coefficients reports, mc2b(postfilter_mcp(c)) [nmcp] long double -- b2mc then
    mc2b is the identity --, plain = mc2b(c), shift, e1, e2, tail = the larger tail/peak of the two responses)."""
    plain = M.mc2b(c, alpha)
    if not (beta > 0.0 and len(plain) > 2):
        return dict(b=plain, plain=plain, shift=LD(0), e1=None, e2=None, tail=0.0)
    ir1 = impulse_response(plain, alpha)
    b = M.postfiltered_b(plain, alpha, beta)
    ir2 = impulse_response(b, alpha)
    e1, e2 = np.sum(ir1 * ir1), np.sum(ir2 * ir2)
    shift = np.log(e1 / e2) / 2
    b[0] += shift
    return dict(b=b, plain=plain, shift=shift, e1=e1, e2=e2, tail=max(tail_over_peak(ir1), tail_over_peak(ir2)))


def closed_form_ir(mc, alpha, N=1 << 15):
    """(g [576], ir [576], noise [2]): the Taylor coefficients of G(w) = sum_k mc[n-1-k] t^k and of exp(G), t =
    (w + a) / (1 + a w), by a long-double FFT on |w| = 1, and the scale of this evaluation's own absolute error in
    each of the two.  (In f64 the Horner evaluation of G, not the transform, limits it: 1e-10 of the peak at order 64.)
    `alpha`: freqt's argument."""
    a = LD(alpha)
    w = M.unit_circle(N)  # exp(-2 pi i j / N): the coefficient of w^k is then numpy's ifft
    t = (w + a) / (1 + a * w)
    G = np.zeros(N, dtype=M.CLD)
    for ck in np.asarray(mc, dtype=LD):  # Horner from the highest power: mc[0] multiplies t^(n-1)
        G = G * t + ck
    E = np.exp(G)
    g, ir = np.fft.ifft(G), np.fft.ifft(E)
    assert ir.dtype == M.CLD  # numpy.fft keeps long double (pocketfft, numpy >= 2)
    # what the evaluation (one rounding per Horner step) and the transform (log2 N) leave in each coefficient
    noise = float(np.finfo(LD).eps) * (len(mc) + np.log2(N)) * np.array([float(np.abs(G).max()), float(np.abs(E).max())])
    return g.real[:IRLENG], ir.real[:IRLENG], noise


def pf_errors(got, ref):
    """(e of b'[0], e of b'[1:], floor of b'[0], floor of b'[1:]) of one row, absolute, evaluated in long double."""
    ref = np.asarray(ref, dtype=LD)
    d = np.abs(np.asarray(got, dtype=LD) - ref)
    return (float(d[0]), float(d[1:].max()), PF_FLOOR_GAIN * max(1.0, float(abs(ref[0]))),
            PF_FLOOR_REST * float(np.abs(ref).max()))


# ---- Stage::NonZero ------------------------------------------------------------------------------------------------
class Kit:
    """The arithmetic a restatement runs in."""

    def __init__(self, name, conv, cos, exp, log, sqrt, pi):
        self.name, self.c, self.cos, self.exp, self.log, self.sqrt, self.pi = name, conv, cos, exp, log, sqrt, pi


LDK = Kit("long double", LD, np.cos, np.exp, np.log, np.sqrt, M.PI)
# the arithmetic under test: what the same text gives in f64 is the scale of an f64 restatement's error
F64K = Kit("f64", np.float64, np.cos, np.exp, np.log, np.sqrt, np.float64(np.pi))


def mp_kit(dps=50):
    """The 50-digit kit; ImportError where mpmath is not installed."""
    import mpmath as mp

    mp.mp.dps = dps
    return Kit("mpmath %d digits" % dps, mp.mpf, mp.cos, mp.exp, mp.log, mp.sqrt, mp.pi)


def to_kit(x, K):
    """A long double (or f64) exactly in kit K."""
    hi = float(x)
    return K.c(hi) + K.c(float(LD(x) - LD(hi)))


def lsp2lpc(l, K, swap_pq=False):
    """lsp.rs:27-91.  swap_pq: the even- and odd-indexed cosines exchanged (what a test breaks on purpose)."""
    m = len(l)
    mh1, mh2 = (m // 2, m // 2) if m % 2 == 0 else ((m + 1) // 2, (m - 1) // 2)
    p = [-2 * K.cos(x) for x in l[0::2]]
    q = [-2 * K.cos(x) for x in l[1::2]]
    if swap_pq:
        p[:mh2], q = q, p[:mh2]
    z = K.c(0)
    a0, a1, a2 = [z] * (mh1 + 1), [z] * (mh1 + 1), [z] * (mh1 + 1)
    b0, b1, b2 = [z] * (mh2 + 1), [z] * (mh2 + 1), [z] * (mh2 + 1)
    xff = xf = z
    out = [z] * (m + 1)
    for k in range(m + 1):
        xx = K.c(1 if k == 0 else 0)
        if m % 2 == 1:
            a0[0], b0[0] = xx, xx - xff
            xff, xf = xf, xx
        else:
            a0[0], b0[0] = xx + xf, xx - xf
            xf = xx
        for i in range(mh1):
            a0[i + 1] = a0[i] + p[i] * a1[i] + a2[i]
            a2[i], a1[i] = a1[i], a0[i]
        for i in range(mh2):
            b0[i + 1] = b0[i] + q[i] * b1[i] + b2[i]
            b2[i], b1[i] = b1[i], b0[i]
        if k > 0:
            out[k - 1] = -(a0[mh1] + b0[mh2]) / 2
    for i in range(m - 1, -1, -1):
        out[i + 1] = -out[i]
    out[0] = K.c(1)
    return out


def _polymul(x, y, K):
    out = [K.c(0)] * (len(x) + len(y) - 1)
    for i, xi in enumerate(x):
        for j, yj in enumerate(y):
            out[i + j] = out[i + j] + xi * yj
    return out


def lsp2lpc_closed(l, K):
    """The first m + 1 coefficients of (A(z) + B(z)) / 2 (module docstring), multiplied out factor by factor."""
    m, one = len(l), K.c(1)
    A, B = [one], [one]
    for x in l[0::2]:
        A = _polymul(A, [one, -2 * K.cos(x), one], K)
    for x in l[1::2]:
        B = _polymul(B, [one, -2 * K.cos(x), one], K)
    if m % 2 == 0:
        A, B = _polymul(A, [one, one], K), _polymul(B, [one, -one], K)
    else:
        B = _polymul(_polymul(B, [one, -one], K), [one, one], K)
    assert len(A) == len(B) == m + 2
    return [(x + y) / 2 for x, y in zip(A[:m + 1], B[:m + 1])]


def gnorm(c, g):
    """generalized.rs:6-21, gamma != 0."""
    k = 1 + g * c[0]
    return [k ** (1 / g)] + [x / k for x in c[1:]]


def ignorm(c, g):
    """generalized.rs:23-38, gamma != 0."""
    k = c[0] ** g
    return [(k - 1) / g] + [x * k for x in c[1:]]


def gc2gc(c1, g1, m2, g2, K):
    """cepstrum.rs:69-94."""
    c = [K.c(0)] * (m2 + 1)
    c[0] = c1[0]
    for i in range(1, m2 + 1):
        s1 = s2 = K.c(0)
        for k in range(1, min(len(c1), i)):
            cc = c1[k] * c[i - k]
            s1 = s1 + (i - k) * cc
            s2 = s2 + k * cc
        c[i] = (c1[i] if i < len(c1) else K.c(0)) + (g2 * s2 - g1 * s1) / i
    return c


def lsp2mgc(l, log_gain, stage, K, swap_pq=False):
    """lsp.rs:93-105; the LPC's alpha is the target's, so mgc2mgc (cepstrum.rs:96-103) is gnorm, gc2gc, ignorm."""
    g = -K.c(1) / stage
    lpc = lsp2lpc(l, K, swap_pq)
    lpc[0] = K.exp(l[0]) if log_gain else l[0]
    lpc = ignorm(lpc, g)
    lpc = [lpc[0]] + [-stage * x for x in lpc[1:]]
    return ignorm(gc2gc(gnorm(lpc, g), g, len(l) - 1, g, K), g)


def stage_coefficients(sp, alpha, beta, log_gain, stage, K=LDK, filtered=True, flip=None, swap_pq=False):
    """One frame of Stage::NonZero: (coefficients [n] in K's numbers, trace).  filtered=True is what every frame
    interpolates to (mod.rs:148-156), False what the first frame starts from (mod.rs:92-106).
    trace: cmp = [(pass, kind, index, fired, margin)] of check_lsp_stability, kind "gap" / "low" / "high" and margin the
    distance of the compared value from its bound; passes = how many of the four ran; unfinished = the last pass that
    ran still moved something; en = |en1 / en2 - 1| (None where the post-filter moves no frequency: both energies
    are then one computation twice); den = the smallest d1^2 + d2^2.
    flip = k inverts the outcome of comparison k (what a test breaks on purpose)."""
    l = [K.c(float(x)) for x in sp]
    n, a, be, g = len(l), K.c(float(alpha)), K.c(float(beta)), -K.c(1) / stage
    trace = dict(cmp=[], passes=0, unfinished=False, en=None, den=None)
    if filtered:
        if beta > 0 and n > 2:
            e1 = sum(x * x for x in lsp2mgc(l, log_gain, stage, K, swap_pq))
            t = list(l)
            for i in range(2, n - 1):
                d1, d2 = be * (l[i + 1] - l[i]), be * (l[i] - l[i - 1])
                den = d2 * d2 + d1 * d1
                trace["den"] = float(den) if trace["den"] is None else min(trace["den"], float(den))
                t[i] = l[i - 1] + d2 + (d2 * d2 * ((l[i + 1] - l[i - 1]) - (d1 + d2))) / den
            l = t
            if n > 3:  # (n = 3: no frequency moved, en1 == en2 as one computation done twice, the gain stays)
                e2 = sum(x * x for x in lsp2mgc(l, log_gain, stage, K, swap_pq))
                trace["en"] = float(abs(e1 / e2 - 1))
                if log_gain:
                    l[0] = l[0] + K.log(e1 / e2) / 2
                else:
                    l[0] = l[0] * K.sqrt(e1 / e2)
        mn, last = K.pi / 4 / n, n - 1

        def decide(kind, j, value, bound, fired):
            k = len(trace["cmp"])
            trace["cmp"].append((trace["passes"], kind, j, bool(fired), float(abs(value - bound))))
            return (not fired) if flip == k else fired

        for _ in range(4):
            trace["passes"] += 1
            find = False
            for j in range(1, last):
                tmp = l[j + 1] - l[j]
                if decide("gap", j, tmp, mn, tmp < mn):
                    l[j], l[j + 1] = l[j] - (mn - tmp) / 2, l[j + 1] + (mn - tmp) / 2
                    find = True
            if decide("low", 1, l[1], mn, l[1] < mn):
                l[1], find = mn, True
            if decide("high", last, l[last], K.pi - mn, l[last] > K.pi - mn):
                l[last], find = K.pi - mn, True
            trace["unfinished"] = find
            if not find:
                break
    m = lsp2mgc(l, log_gain, stage, K, swap_pq)
    cc = list(m)
    if alpha != 0:
        for i in range(n - 2, -1, -1):
            cc[i] = m[i] - a * cc[i + 1]
    cc = gnorm(cc, g)
    return [cc[0]] + [g * x for x in cc[1:]], trace


def decisive(trace, margin):
    """The comparisons of a trace that moved something and were at least `margin` clear of a tie: (pass, kind, index).
    (A pass that only repeats the comparisons of the one before at a margin of rounding may or may not run.)"""
    return [(p, kind, j) for p, kind, j, fired, m in trace["cmp"] if fired and m >= margin]


def as_ld(row):
    return np.array(row, dtype=LD)


def rel_inf(got, ref):
    """max |got - ref| / max |ref| in long double (ref: long double row)."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max() / np.abs(ref).max())


def rel_inf_kit(got, ref, K):
    """The same against a reference row in kit K's numbers (got: long double or f64 values), evaluated in K."""
    return float(max(abs(to_kit(x, K) - y) for x, y in zip(got, ref)) / max(abs(y) for y in ref))
