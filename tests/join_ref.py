"""The join stage in numpy (include/jbonsai_amd.h "Join"): programmes numbered by first member, each its members in
ascending index between their pads of zeros, the smoothstep fades at the members' edges, the truncation toward zero
of a faded 16-bit sample.  What jb_join_host, the device seam and the batch path are held to, bit for bit."""
import numpy as np

NONE = None  # an utterance of its own

# member lengths around the 16-byte group and the tile, and pads: what the device tests join and the host tests lay out
LENGTHS = [0, 1, 7, 8, 63, 64, 65, 4095, 4096, 4097]
PADS = [0, 1, 3, 4097]


def ms_to_samples(ms, hz):
    """floor(ms * hz / 1000.0 + 0.5); 0 for a negative duration"""
    v = float(ms) * float(hz) / 1000.0 + 0.5
    return int(np.floor(v)) if v >= 1.0 else 0


def weight(k, fade):
    """s(t) of samples k (an integer array) of a fade of `fade` samples, counted from the edge"""
    t = (2 * k.astype(np.uint64) + 1).astype(np.float64) / np.float64(2 * fade)
    return (t * t) * (3.0 - 2.0 * t)


def member(x, fade_in=0, fade_out=0):
    """A member under its fades: x * s_in * s_out in that order, each factor only where its fade reaches; float64
    stays float64, int16 is truncated toward zero; samples outside both fades keep their bits."""
    x = np.asarray(x)
    n = x.size
    out = x.copy()
    k = np.arange(n, dtype=np.int64)
    fin = k < fade_in
    fout = (n - 1 - k) < fade_out
    touched = fin | fout
    if not touched.any():
        return out
    v = x.astype(np.float64)
    if fin.any():
        v[fin] = v[fin] * weight(k[fin], fade_in)
    if fout.any():
        v[fout] = v[fout] * weight((n - 1 - k)[fout], fade_out)
    if x.dtype == np.int16:
        out[touched] = np.trunc(v[touched]).astype(np.int16)
    else:
        out[touched] = v[touched]
    return out


def number(programmes):
    """(programme_of [n], members per programme) with programmes numbered densely in the order of their first member;
    an entry None is a programme of its own"""
    dense, prog_of, members = {}, [], []
    for u, p in enumerate(programmes):
        if p is None or p not in dense:
            d = len(members)
            members.append([])
            if p is not None:
                dense[p] = d
        else:
            d = dense[p]
        prog_of.append(d)
        members[d].append(u)
    return prog_of, members


def join(pcms, req):
    """req[u] = (programme, pad_before, pad_after, fade_in, fade_out), missing trailing entries 0.
    Returns (programmes, programme_of, member_start)."""
    req = [tuple(r) + (0,) * (5 - len(r)) for r in req]
    prog_of, members = number([r[0] for r in req])
    dtype = np.asarray(pcms[0]).dtype if len(pcms) else np.float64
    out, start = [], [0] * len(pcms)
    for mem in members:
        parts, k = [], 0
        for u in mem:
            _, before, after, fin, fout = req[u]
            x = member(pcms[u], fin, fout)
            start[u] = k + before
            parts += [np.zeros(before, dtype=dtype), x, np.zeros(after, dtype=dtype)]
            k += before + x.size + after
        out.append(np.concatenate(parts).astype(dtype, copy=False))
    return out, prog_of, start


def chapter(lengths, hz, lead_ms=0.0, gap_ms=0.0, trail_ms=0.0, fade_ms=0.0):
    """The request of a jb_synthesize_programme* call: one programme of all the utterances"""
    n = len(lengths)
    f = ms_to_samples(fade_ms, hz)
    return [(0, ms_to_samples(lead_ms, hz) if u == 0 else 0,
             ms_to_samples(trail_ms if u == n - 1 else gap_ms, hz), f, f) for u in range(n)]
