"""The mix stage in numpy (include/jbonsai_amd.h "Mix"), on tests/join_ref.py: programmes numbered by first member, each
the sum of its unmuted members in ascending index -- every member at its start, under the join's fades in float64 (an
int16 sample enters as its float64; nothing is truncated per member) and under its gain where that is not 1 -- the first
term starting the sum, +0.0 under no member; the fit; the 16-bit sink.  What jb_mix_host, the device seam and the batch
path are held to, bit for bit.  The gain g comes from the library (jb_mix_gain), as the rule says tests take it."""
import numpy as np

from tests import join_ref as R


def norm(req):
    """req[u] = (programme, start, gain_db, pad_after, fade_in, fade_out), missing trailing entries 0"""
    return [tuple(r) + (0,) * (6 - len(r)) for r in req]


def term(x, fade_in, fade_out, g):
    """A member's terms in float64: x * s_in * s_out in that order where the fades reach, then * g where g != 1"""
    x = np.asarray(x)
    n = x.size
    v = x.astype(np.float64)  # (a copy: float64 samples outside the fades keep their bits)
    k = np.arange(n, dtype=np.int64)
    fin = k < fade_in
    fout = (n - 1 - k) < fade_out
    if fin.any():
        v[fin] = v[fin] * R.weight(k[fin], fade_in)
    if fout.any():
        v[fout] = v[fout] * R.weight((n - 1 - k)[fout], fade_out)
    if g != 1.0:
        v = v * np.float64(g)
    return v


def sink16(v):
    """The 16-bit sink: fmin(v, 32767), fmax(., -32768) (a NaN goes to 32767), truncation toward zero"""
    v = np.fmax(np.fmin(v, 32767.0), -32768.0)
    return np.trunc(v).astype(np.int16)


def geometry(lengths, req, gains):
    """(programme_of, members per programme, samples [P], depth [P], overlap [P])"""
    req = norm(req)
    prog_of, members = R.number([r[0] for r in req])
    ns, depth, overlap = [], [], []
    for mem in members:
        n = max([req[u][1] + lengths[u] + req[u][3] for u in mem] + [0])
        cover = np.zeros(n, dtype=np.int64)
        for u in mem:
            if gains[u] != 0.0:
                cover[req[u][1]:req[u][1] + lengths[u]] += 1
        ns.append(n)
        depth.append(int(cover.max()) if n else 0)
        overlap.append(int((cover >= 2).sum()))
    return prog_of, members, ns, depth, overlap


def mix(pcms, req, gains, fit=False, ceiling=0.0, scale=None):
    """gains[u] = jb_mix_gain(gain_db[u]); ceiling in sample units; scale: one given s per programme, or None for the
    rule's.  Returns (programmes, sums in float64 in front of the fit and the sink, peaks, scales, programme_of)."""
    req = norm(req)
    dtype = np.asarray(pcms[0]).dtype if len(pcms) else np.float64
    prog_of, members, ns, _, _ = geometry([np.asarray(x).size for x in pcms], req, gains)
    out, sums, peaks, scales = [], [], [], []
    for p, mem in enumerate(members):
        acc = np.zeros(ns[p], dtype=np.float64)
        have = np.zeros(ns[p], dtype=bool)
        for u in mem:  # ascending utterance index, whatever the starts
            g = gains[u]
            x = np.asarray(pcms[u])
            if g == 0.0 or x.size == 0:
                continue
            t = term(x, req[u][4], req[u][5], g)
            s = slice(req[u][1], req[u][1] + x.size)
            first = ~have[s]
            with np.errstate(all="ignore"):
                both = acc[s] + t
            acc[s] = np.where(first, t, both)  # the first term starts the sum: its bits, -0.0 and NaN payloads kept
            have[s] = True
        with np.errstate(all="ignore"):
            M = float(np.fmax.reduce(np.abs(acc), initial=0.0))
        c = float(ceiling)
        s_p = float(scale[p]) if scale is not None else (c / M if (fit and M > c) else 1.0)
        y = acc
        if fit and s_p != 1.0:
            with np.errstate(all="ignore"):
                y = np.fmin(np.fmax(acc * np.float64(s_p), -c), c)
        out.append(sink16(y) if dtype == np.int16 else y.copy())
        sums.append(acc)
        peaks.append(M)
        scales.append(s_p)
    return out, sums, peaks, scales, prog_of


def from_join(req, lengths):
    """A join request (join_ref's tuples) as the mix request with the join's starts, at 0 dB: programme by programme
    the members one after the other, each start the running sum plus its pad_before"""
    req = [tuple(r) + (0,) * (5 - len(r)) for r in req]
    _, members = R.number([r[0] for r in req])
    out = [None] * len(req)
    for mem in members:
        k = 0
        for u in mem:
            prog, before, after, fin, fout = req[u]
            out[u] = (prog, k + before, 0.0, after, fin, fout)
            k += before + lengths[u] + after
    return out
