"""The table of tests/test_gpu_loudness_ld.py: output rates by the tiling class of the measurement (jb_loudness.hip),
the lengths and signals of each, the hop-count edges at the lowest rate, and the two references of every case -- the
long-double one (tests/loudness_ld_ref.py) and the f64 comparator (tests/loudness_ref.py, with the R128 fields of
tests/loudness_groups_ref.py on the same f64 hop energies) -- each computed once per process.

The tiling, restated (tile_of): a hop H = (hz + 5) // 10 is cut into tph = ceil(H / 4096) tiles of 256 lanes x S
samples, S = ceil(H / (256 tph)), G = 256 S, and the hop's last tile has last = H - (tph - 1) G samples.  Every row
carries the class it is there for, and check_table() holds it against the rule: a change of the tiling fails there
instead of quietly testing one class twice.

A case's samples are the first n of its kind's signal at that rate, so one serial long-double pass over the longest
serves every length (the filter is causal)."""
import functools
import math

import numpy as np

from tests import loudness_groups_ref as G64
from tests import loudness_ld_ref as R
from tests.loudness_ref import integrated

# hz: (H, tph, S, G, last, why)
RATES = {
    3400: (340, 1, 2, 512, 340, "the smallest stable rates' class: S = 2, half the lanes idle"),
    5120: (512, 1, 2, 512, 512, "exact fit, one tile"),
    5130: (513, 1, 3, 768, 513, "one sample over"),
    24000: (2400, 1, 10, 2560, 2400, "a common output rate"),
    32000: (3200, 1, 13, 3328, 3200, "a common output rate"),
    40960: (4096, 1, 16, 4096, 4096, "S = 16, the full LDS image, exact"),
    40970: (4097, 2, 9, 2304, 1793, "the smallest two-tile hop"),
    48000: (4800, 2, 10, 2560, 2240, "the product's own"),
    81920: (8192, 2, 16, 4096, 4096, "two full tiles"),
    81930: (8193, 3, 11, 2816, 2561, "the smallest three-tile hop: the first with an inner tile (A^G)"),
    176400: (17640, 5, 14, 3584, 3304, "five tiles"),
    192000: (19200, 5, 15, 3840, 3840, "exact fit at a real rate"),
    384000: (38400, 10, 15, 3840, 3840, "ten tiles, exact fit"),
    573450: (57345, 15, 15, 3840, 3585, "the first rate with 15 tiles"),
    614390: (61439, 15, 16, 4096, 4095, "the largest hop, last = G - 1"),
}
STEP_RATES = (48000, 192000)   # with the loud-then-quiet signal: the relative gate drops blocks
EDGE_HZ = 3400                 # the hop-count and block-count edges
EDGE_HOPS = (63, 64, 65, 127, 128, 129, 300)  # k_ln_scan's 64 lane chunks; 300: 297 blocks, 271 short-term windows
EDGE_TAIL = 17                 # samples of a tail hop behind the full ones


def tile_of(hz):
    """(H, tph, S, G, last) by the rule of loudness_rate (jb_loudness.hip), restated."""
    H = (int(hz) + 5) // 10
    tph = -(-H // 4096)
    S = -(-H // (256 * tph))
    return H, tph, S, 256 * S, H - (tph - 1) * 256 * S


def check_table():
    for hz, row in RATES.items():
        assert tile_of(hz) == row[:5], (hz, tile_of(hz), row[:5])
        H, tph, S, Gt, last = row[:5]
        assert 1 <= S <= 16 and 1 <= last <= Gt and tph <= 15
    rows = [r[:5] for r in RATES.values()]
    assert {r[1] for r in rows} >= {1, 2, 3, 5, 10, 15}                    # tiles per hop
    assert {r[2] for r in rows} >= {2, 3, 9, 10, 11, 13, 14, 15, 16}       # samples per lane
    assert sum(r[4] == r[3] for r in rows) >= 5                            # exact fits
    assert any(r[4] == r[3] - 1 for r in rows)                             # last = G - 1
    assert tile_of(40960)[1] == 1 and tile_of(40970)[1] == 2               # the threshold between one tile and two
    assert EDGE_HZ in RATES and max(EDGE_HOPS) - 3 > 256                   # more blocks than k_ln_gate has lanes


def lengths(hz):
    H, _, _, Gt, _ = RATES[hz][:5]
    if hz > 200000:
        return [4 * H, 5 * H + min(Gt, H) + 1]
    return [4 * H - 1, 4 * H, 4 * H + 1, 5 * H + min(Gt, H) + 1, 7 * H - 1]


# ---- signals, all inside +-32767 -------------------------------------------------------------------------------------
def _seed(hz, kind):
    return [20261021, int(hz), sum(kind.encode())]


@functools.lru_cache(maxsize=None)
def signal(hz, kind):
    """The kind's signal at hz in 16-bit units, as long as its longest case."""
    H = RATES[hz][0]
    rng = np.random.default_rng(_seed(hz, kind))
    if kind == "white":
        x = rng.standard_normal(max(lengths(hz))) * 3000.0
    elif kind == "carried":  # the states are O(x) and the output their difference
        n = max(lengths(hz))
        x = 20000.0 + 4000.0 * np.sin(2.0 * np.pi * 25.0 * np.arange(n) / hz) + rng.standard_normal(n) * 30.0
    elif kind == "step":     # a loud part, then the same part 40 dB down
        loud = rng.standard_normal(8 * H) * 6000.0
        x = np.concatenate([loud, loud * 0.01])
    elif kind == "quiet":    # under -70 LUFS
        x = rng.standard_normal(4 * H + 1) * 0.02
    elif kind == "silence":
        x = np.zeros(4 * H + 1)
    elif kind == "edge":     # a carried state under level steps of 6 and 12 dB every 40 hops
        n = max(EDGE_HOPS) * H + EDGE_TAIL
        g = np.array([1.0, 0.5, 0.25])[(np.arange(n) // (40 * H)) % 3]
        x = 20000.0 + g * (4000.0 * np.sin(2.0 * np.pi * 25.0 * np.arange(n) / hz) + rng.standard_normal(n) * 30.0)
    else:
        raise KeyError(kind)
    assert np.max(np.abs(x)) <= 32767.0
    x.setflags(write=False)
    return x


def cases(hz):
    """[(kind, n)] of the rate's seam call."""
    out = [(k, n) for k in ("white", "carried") for n in lengths(hz)]
    if hz in STEP_RATES:
        out.append(("step", 16 * RATES[hz][0]))
    out += [("quiet", 4 * RATES[hz][0] + 1), ("silence", 4 * RATES[hz][0] + 1)]
    return out


def edge_cases():
    H = RATES[EDGE_HZ][0]
    return [("edge", nh * H + EDGE_TAIL) for nh in EDGE_HOPS]


def pcm(hz, kind, n):
    return signal(hz, kind)[:n]


# ---- the two references ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _z_ld(hz, kind):
    return R.hop_energies_ld(signal(hz, kind), hz)[0]


@functools.lru_cache(maxsize=None)
def _z_f64(hz, kind):
    return G64.hop_energies(signal(hz, kind), hz)[0]


@functools.lru_cache(maxsize=None)
def reference(hz, kind, n):
    """The long-double Measure of the case, its gate margins checked."""
    H = RATES[hz][0]
    m = R.Measure(_z_ld(hz, kind)[: n // H], H)
    m.check_margin("%d Hz, %s, %d samples" % (hz, kind, n))
    return m


VALUES = ("lufs", "max_momentary", "max_short_term", "lra_low", "lra_high")


@functools.lru_cache(maxsize=None)
def comparator(hz, kind, n):
    """The f64 evaluation of the case: dict over VALUES (the names of Measure)."""
    H = RATES[hz][0]
    r = G64.r128([_z_f64(hz, kind)[: n // H]], H)
    return {"lufs": integrated(pcm(hz, kind, n), hz)[0], "max_momentary": r["max_momentary_lufs"],
            "max_short_term": r["max_short_term_lufs"], "lra_low": r["lra_low_lufs"], "lra_high": r["lra_high_lufs"]}


def err(v, ref):
    """|v - ref| in LU against a long-double reference value; 0 where both are the same infinity or both NaN, inf
    where one is finite and the other is not."""
    v, ref = R.LD(v), R.LD(ref)
    if np.isnan(ref) or np.isnan(v):
        return 0.0 if np.isnan(ref) and np.isnan(v) else math.inf
    if np.isinf(ref) or np.isinf(v):
        return 0.0 if v == ref else math.inf
    return float(abs(v - ref))


def e64(hz, kind, which):
    """The comparator's largest error over the given (kind, n) cases of one signal kind at hz, all VALUES."""
    worst = 0.0
    for k, n in which:
        if k != kind:
            continue
        ref, c = reference(hz, k, n), comparator(hz, k, n)
        worst = max(worst, max(err(c[v], getattr(ref, v)) for v in VALUES))
    return worst


if __name__ == "__main__":
    check_table()
    for hz in RATES:
        for kind in ("white", "carried") + (("step",) if hz in STEP_RATES else ()):
            cs = [c for c in cases(hz) if c[0] == kind]
            print("%7d %-8s e64 %.3e  margin %.3g" % (hz, kind, e64(hz, kind, cs),
                                                       min(reference(hz, k, n).margin for k, n in cs)), flush=True)
    cs = edge_cases()
    print("%7d %-8s e64 %.3e  margin %.3g" % (EDGE_HZ, "edge", e64(EDGE_HZ, "edge", cs),
                                               min(reference(EDGE_HZ, k, n).margin for k, n in cs)))
