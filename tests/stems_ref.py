"""The stems of a mix in numpy (include/jbonsai_amd.h "Stems of a mix"), on tests/mix_ref.py: the members of one
programme under one stem id form one stem, a unit of the programme's length behind the programmes -- numbered by
programme, within one by the first member of each stem -- whose sample k is the mix rule over the stem's own members
alone; with the fit, acc * s_p of the PROGRAMME's scale and no clamp; the 16-bit sink.  And the levels: the three sums
in the stage's order (tiles of 1,024 samples, 256 strided partials whose first term is the product and whose later
terms are fused on, the tree h = 128 .. 1, the tile sums added in ascending order), and the three dB values in long
double.  Written from the rule's statement, not from the C++."""
import math

import numpy as np

from tests import mix_ref as M

TILE, LANES = 1024, 256


def number(req, stem_of):
    """(P, stems): stems[s] = (programme, id, members) in unit order (unit P + s); stem_of[u] None: no stem"""
    req = M.norm(req)
    _, members = M.R.number([r[0] for r in req])
    stems = []
    for p, mem in enumerate(members):
        seen = {}
        for u in mem:  # ascending utterance index: a stem is numbered where its first member stands
            if stem_of[u] is None:
                continue
            if stem_of[u] not in seen:
                seen[stem_of[u]] = len(stems)
                stems.append((p, stem_of[u], []))
            stems[seen[stem_of[u]]][2].append(u)
    return len(members), stems


def extent(req, lengths, gains, mem):
    """[first, end) over the unmuted members of at least one sample; (0, 0) without one"""
    req = M.norm(req)
    live = [u for u in mem if gains[u] != 0.0 and lengths[u]]
    if not live:
        return 0, 0
    return min(req[u][1] for u in live), max(req[u][1] + lengths[u] for u in live)


def stems(pcms, req, stem_of, gains, fit=False, ceiling=0.0, scale=None):
    """(units, sums, peaks, scales): the P programmes by mix_ref.mix and the S stems behind them; sums: each unit's
    float64 sum in front of the scale and the sink; scales: [P]"""
    req = M.norm(req)
    dtype = np.asarray(pcms[0]).dtype if len(pcms) else np.float64
    out, sums, peaks, scales, _ = M.mix(pcms, req, gains, fit=fit, ceiling=ceiling, scale=scale)
    P, st = number(req, stem_of)
    for p, _, mem in st:
        n = sums[p].size
        acc = np.zeros(n, dtype=np.float64)
        have = np.zeros(n, dtype=bool)
        for u in mem:
            x = np.asarray(pcms[u])
            if gains[u] == 0.0 or x.size == 0:
                continue
            t = M.term(x, req[u][4], req[u][5], gains[u])
            s = slice(req[u][1], req[u][1] + x.size)
            with np.errstate(all="ignore"):
                acc[s] = np.where(have[s], acc[s] + t, t)
            have[s] = True
        with np.errstate(all="ignore"):
            peaks.append(float(np.fmax.reduce(np.abs(acc), initial=0.0)))
            y = acc * np.float64(scales[p]) if fit and scales[p] != 1.0 else acc
        out.append(M.sink16(y) if dtype == np.int16 else y.copy())
        sums.append(acc)
    return out, sums, peaks, scales


def fma(a, b, c):
    """fma(a, b, c) of float64 scalars, rounded once: the exact value in rationals"""
    from fractions import Fraction

    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:
        return a * b + c  # (the sign of a zero as IEEE has it; no rounding happens)
    return float(v)  # (Fraction -> float rounds to nearest even, once)


def level_sum(a, b, first=0, end=None):
    """sum a[k] b[k] over the tiles that touch [first, end), in the stage's order"""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    n = a.size
    end = n if end is None else end
    if end <= first:
        return 0.0
    S = None
    for i in range(first // TILE, (end + TILE - 1) // TILE):
        p = [0.0] * LANES
        for l in range(LANES):
            have = False
            for k in range(i * TILE + l, min((i + 1) * TILE, n), LANES):
                p[l] = fma(float(a[k]), float(b[k]), p[l]) if have else float(a[k]) * float(b[k])
                have = True
        h = LANES // 2
        while h:
            for l in range(h):
                p[l] = p[l] + p[l + h]
            h //= 2
        S = p[0] if S is None else S + p[0]
    return S


def levels(stem, mix, first=0, end=None):
    """(E_s, D, E_p)"""
    return level_sum(stem, stem, first, end), level_sum(stem, mix, first, end), level_sum(mix, mix)


def db(e_s, d, e_p):
    """(level_db, sir_db, si_sdr_db) of three sums, in long double"""
    L = np.longdouble
    es, dd, ep = L(e_s), L(d), L(e_p)

    def ratio(num, den):
        if e_s == 0.0:
            return -math.inf
        if not den > 0:
            return math.inf
        with np.errstate(divide="ignore"):
            return float(L(10) * np.log10(num / den))

    a = dd * dd / es if e_s != 0.0 else L(0)
    return ratio(es, ep), ratio(es, ep - 2 * dd + es), ratio(a, ep - a)


def db_model(stem, mix):
    """The three dB values of whole signals with every sum taken in long double: the model the gate measures against"""
    L = np.longdouble
    s, m = np.asarray(stem).astype(L), np.asarray(mix).astype(L)
    return db_sums(np.sum(s * s), np.sum(s * m), np.sum(m * m))


def db_sums(es, dd, ep):
    """The dB values of sums of any float type, evaluated in long double (no special cases: the gate's cases have none)"""
    L = np.longdouble
    es, dd, ep = L(es), L(dd), L(ep)
    a = dd * dd / es
    return (float(10 * np.log10(es / ep)), float(10 * np.log10(es / (ep - 2 * dd + es))),
            float(10 * np.log10(a / (ep - a))))


def seq_sums(stem, mix):
    """A plain sequential float64 evaluation of the three sums: what the gate's allowance is measured on"""
    s, m = np.asarray(stem).astype(np.float64), np.asarray(mix).astype(np.float64)
    es = dd = ep = 0.0
    for a, b in zip(s.tolist(), m.tolist()):
        es += a * a
        dd += a * b
        ep += b * b
    return es, dd, ep
