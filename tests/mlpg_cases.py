"""The case table of the dense MLPG tests (tests/test_mlpg_dense.py without a GPU, tests/test_gpu_mlpg_dense.py with
one): window sets x stream shapes, each case one batch whose utterances are the voicing patterns (MSD) or the lengths
(no MSD).  Inputs are drawn once per (window set, stream shape); the GV-on and GV-off cases of a pair share them, so
that one dense solve serves both.  Dense systems, their solutions and the oracle's tracks are cached per process.

The table is a designed subset of the cross product (12 window sets x 7 shapes x GV on / off would be 168 batches):
  * the band-width-3 window sets are the ones the fused kernels of launch_mlpg_bw take ([dim][frame] workspace,
    k_mlpg_solve3, k_mlpg_fb_runs, k_mlpg_gv_vt): nitech's 1/3/3 gets every shape with GV on and off, the other two a
    spread of shapes;
  * every wider window set takes k_mlpg_build<BW> + k_mlpg_solve<BW>, one code path in which the shape shows only as
    L, the MSD compaction and the GV flag: each gets an MSD shape with L >= 2, a shape without MSD, and a third shape
    that rotates, so that every shape meets at least two wide window sets.
A GV-on case holds utterances with gv_weight 1.0 and 0.7 and the three switch patterns."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from typing import List

import numpy as np

from tests import mlpg_ref as R

DMAX = 1.7976931348623157e308
# The GV parameters and the level of the static means are this table's to choose.  They are chosen on the CPU, from the
# oracle's own error against the dense long-double ascent (tests/test_mlpg_dense.py asserts all of it):
#   * gv_var scales the part of the ascent's step divisor h (mlpg.rs:246-249) that can take either sign.  At 20..40 it
#     cancels the band term in isolated voiced frames, h passes near zero and the ascent amplifies rounding errors to
#     2e-8; at 0.1..0.3 the oracle stays within 2e-13 of the long-double ascent on the whole table.
#   * the project's contract for the time-parallel GV sums is elementwise, rtol 1e-12 / atol 1e-13.  Two f64
#     evaluations that are each within e of the exact result differ by up to 2 e, so a case can hold a kernel to that
#     contract only where the oracle's own elementwise error is at most half of it.  With variances over three decades
#     (cond_inf(A) ~ 1e4) and zero-mean parameters it is up to twice the contract at elements near zero, where atol
#     alone counts; static means around 1 (as LF0 and the low MCP dims have them) bring it to a third.
#   * GV_SALT picks the draw of the GV parameters: with this one the smallest relative change of the ascent's
#     objective is 1e-8, an order above the 1e-9 that the step-size branch needs.
GV_MEAN, GV_VAR = (0.6, 1.0), (0.1, 0.3)
STATIC_MEAN_OFFSET = 1.0
GV_SALT = 1
DENSE_DIMS_ABOVE = 40  # voiced frames above which a stream of more than 4 dims is solved densely on four dims only


def _fit(width):
    """Least-squares slope and a zero-sum curvature window over `width` taps (tests/test_gpu_configs.py's formulas)."""
    h = width // 2
    k = np.arange(-h, h + 1, dtype=np.float64)
    d1 = k / np.sum(k * k)
    d2 = k * k - np.mean(k * k)
    d2 = 2.0 * d2 / np.sum(d2 * d2) * np.sum(np.abs(d2)) / width
    return [[1.0], d1.tolist(), d2.tolist()]


WINDOW_SETS = {
    "nitech_1_3_3": [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]],
    "1_5_5": [[1.0], [-0.2, -0.1, 0.0, 0.1, 0.2], [0.285714, -0.142857, -0.285714, -0.142857, 0.285714]],
    "1_7_7": _fit(7),
    "1_9_9": _fit(9),
    "mixed_1_3_7": [[1.0], [-0.5, 0.0, 0.5], [0.1, -0.2, 0.05, 0.1, 0.05, -0.2, 0.1]],
    "mixed_1_9_3": [[1.0], (np.arange(-4, 5) / 60.0).tolist(), [1.0, -2.0, 1.0]],
    "even_1_2_4": [[1.0], [-1.0, 1.0], [0.25, -0.5, -0.25, 0.5]],
    "even_1_6_8": [[1.0], [0.1, -0.3, 0.2, 0.3, -0.2, -0.1], [0.05, 0.1, -0.2, 0.3, -0.3, 0.2, -0.1, -0.05]],
    "zero_taps_in_7": [[1.0], [0.0, 0.0, -0.5, 0.0, 0.5, 0.0, 0.0], [0.0, 1.0, 0.0, -2.0, 0.0, 1.0, 0.0]],
    "static_tap_0p7": [[0.7], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]],
    "two_windows_1_3": [[1.0], [-0.5, 0.0, 0.5]],
    "four_windows_1_3_3_5": [[1.0], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0], [-0.2, -0.1, 0.0, 0.1, 0.2]],
}
# The first window with more than one tap: the reference's own result differs from the normal equations there
# (mlpg.rs:48-56), so these are compared with the oracle only
QUIRK_WINDOW_SETS = {
    "static_3_taps": [[0.1, 0.8, 0.1], [-0.5, 0.0, 0.5], [1.0, -2.0, 1.0]],
    "static_2_taps": [[0.2, 0.8], [-0.5, 0.0, 0.5]],
}

SHAPES = {  # name: (L, is_msd)
    "L1_msd": (1, True), "L1": (1, False), "L2_msd": (2, True), "L2": (2, False),
    "L4_msd": (4, True), "L4": (4, False), "L35_msd": (35, True),
}

_ALL = list(SHAPES)
TABLE = ([("nitech_1_3_3", s, gv) for s in _ALL for gv in (True, False)]
         + [("static_tap_0p7", s, True) for s in ("L1_msd", "L4_msd", "L2", "L1")]
         + [("static_tap_0p7", "L2_msd", False)]
         + [("two_windows_1_3", s, True) for s in ("L1", "L4", "L2_msd", "L35_msd")]
         + [("two_windows_1_3", "L1_msd", False)])
_WIDE = ["1_5_5", "1_7_7", "1_9_9", "mixed_1_3_7", "mixed_1_9_3", "even_1_2_4", "even_1_6_8", "zero_taps_in_7",
         "four_windows_1_3_3_5"]
_THIRD = [("L1_msd", True), ("L1", False), ("L4_msd", False), ("L35_msd", True), ("L2", True), ("L1_msd", False),
          ("L1", True), ("L4_msd", True), ("L2", False)]
for _k, _w in enumerate(_WIDE):
    TABLE += [(_w, "L2_msd", True), (_w, "L4", True), (_w,) + _THIRD[_k]]
TABLE += [("1_9_9", "L35_msd", True)]  # nitech's own vector length under the widest band as well
# every GV-on case has its GV-off twin on the same inputs: the gates on the solve itself need a track without GV
TABLE += [(_w, _s, False) for _w, _s, _g in list(TABLE) if _g and (_w, _s, False) not in TABLE]


def band_width(windows):
    return max(len(w) for w in windows) // 2 * 2 + 1


def time_parallel_gv(windows, L, use_gv):
    """Whether the stream's GV runs as time-parallel sums by default: the [dim][frame] path of plan_stream_mode."""
    return bool(use_gv) and band_width(windows) == 3 and len(windows) <= 3 and 2 < L <= 60


def _seed(*words):
    return zlib.crc32(" ".join(str(w) for w in words).encode())


# ---- voicing patterns: lists of (duration, kind) states, kind V voiced, U unvoiced, E msd == threshold ----

def _split(rng, n, kind, zero_first=False, zero_inside=False, zero_last=False):
    """n frames of one kind as states of 1..3 frames, with zero-duration states of the same kind where asked."""
    out = []
    while n > 0:
        d = int(min(n, rng.integers(1, 4)))
        out.append((d, kind))
        n -= d
    if zero_inside:
        out.insert(max(1, len(out) // 2), (0, kind))
    if zero_first:
        out.insert(0, (0, kind))
    if zero_last:
        out.append((0, kind))
    return out


def _runs(rng, lengths, gap=1, lead=0, tail=0):
    """Voiced runs of the given lengths separated by `gap` unvoiced frames."""
    st = _split(rng, lead, "U")
    for i, n in enumerate(lengths):
        if i:
            st += _split(rng, gap, "U")
        st += _split(rng, n, "V")
    return st + _split(rng, tail, "U")


def _one_frame_states(S):
    """S states of one frame: a few short runs and one run across state 64 (to the end where S <= 65)."""
    kinds = ["U"] * S
    for a, b in ((2, 3), (7, 9), (20, 21), (50, 80), (100, 128)):
        for s in range(a, min(b, S - 1) + 1):
            kinds[s] = "V"
    return [(1, k) for k in kinds]


def msd_patterns(rng):
    """[(name, states, threshold)]: every voicing pattern of the MSD shapes."""
    zero = (_split(rng, 0, "V", zero_first=True)                       # the utterance's first state
            + _split(rng, 2, "U")
            + _split(rng, 7, "V", zero_first=True, zero_inside=True, zero_last=True)  # a run's first / inner / last state
            + _split(rng, 1, "U") + [(0, "U")]
            + _split(rng, 3, "V") + [(0, "U")] + _split(rng, 2, "V")   # an empty unvoiced state does not cut a run
            + _split(rng, 2, "U"))
    zero += [(1, "V" if (s // 3) % 2 else "U") for s in range(len(zero), 60)]
    zero += [(1, "V")] * (64 - len(zero)) + [(0, "V")] + [(1, "V")] * 4    # state 64, inside a run
    zero += _split(rng, 2, "U") + _split(rng, 3, "V", zero_last=True)     # the utterance's last state
    assert zero[64] == (0, "V") and zero[0][0] == 0 and zero[-1][0] == 0
    scattered = [(int(rng.integers(0, 4)), "R") for _ in range(20)]        # R: msd drawn over the whole of (0, 1)
    pats = [
        ("all_voiced", _split(rng, 21, "V"), 0.5),
        ("none_voiced", _split(rng, 9, "U"), 0.5),
        ("one_voiced_frame", [(3, "U"), (1, "V"), (3, "U")], 0.3),
        ("70_runs_of_one", _runs(rng, [1] * 70), 0.5),
        ("runs_1_to_17", _runs(rng, list(range(1, 11)) + [15, 16, 17]), 0.3),
        ("run_at_both_ends", _runs(rng, [5, 4], gap=2), 0.5),
        ("unvoiced_at_both_ends", _runs(rng, [6], lead=2, tail=3), 0.3),
        ("zero_duration_states", zero, 0.5),
        ("msd_equals_threshold_0p5", _split(rng, 4, "V") + [(2, "E")] + _split(rng, 5, "V") + [(1, "E")], 0.5),
        ("msd_equals_threshold_0p3", [(1, "E")] + _split(rng, 3, "V") + [(1, "E")] + _split(rng, 4, "V"), 0.3),
        ("scattered_threshold_0p3", scattered, 0.3),
        ("scattered_threshold_0p5", scattered, 0.5),
    ]
    pats += [("%d_one_frame_states" % S, _one_frame_states(S), 0.5) for S in (63, 64, 65, 130)]
    return pats


def lengths_without_msd(bw):
    return sorted({1, 2, 3, 4, 5, bw - 1, bw, bw + 1, 15, 16, 17, 33, 63, 64, 65} - {0})


def _states_of_length(rng, T):
    """T frames as states of 0..3 frames (zero-duration states included)."""
    out = []
    while T > 0:
        d = int(min(T, rng.choice([0, 1, 1, 2, 3])))
        out.append((d, "V"))
        T -= d
    return out


# ---- cases ----

@dataclass
class Utt:
    name: str
    durations: np.ndarray
    stream: R.Stream


@dataclass
class Case:
    wset: str
    shape: str
    use_gv: bool
    windows: List[List[float]]
    L: int
    is_msd: bool
    utts: List[Utt] = field(default_factory=list)
    tag: str = ""

    @property
    def name(self):
        return "%s-%s-%s%s" % (self.wset, self.shape, "gv" if self.use_gv else "nogv", self.tag)

    @property
    def slot(self):
        """Where the stream sits in a three-stream voice: the spectrum slot takes 2..64 dims, the LF0 slot one dim;
        one dim without MSD goes to the LPF slot (an odd number of taps)."""
        return 0 if self.L > 1 else 1 if self.is_msd else 2


def _draw(rng, states, threshold, L, W):
    """durations and the per-state arrays of one utterance.  Variances in 1e-3..1 (cond_inf(A) <= 1e8)."""
    S = len(states)
    dur = np.array([d for d, _ in states], dtype=np.uint32)
    mean = rng.standard_normal((S, W * L))
    mean[:, :L] += STATIC_MEAN_OFFSET
    var = 10.0 ** rng.uniform(-3.0, 0.0, (S, W * L))
    msd = np.array([rng.uniform(0.6, 1.0) if k == "V" else rng.uniform(0.0, 0.25) if k == "U" else
                    threshold if k == "E" else rng.uniform(0.0, 1.0) for _, k in states])
    return dur, mean, var, msd


def _gv_switch(rng, stream, dur, variant):
    """Per-state switch: variant 0 all on, 1 about 30 % of the states off, 2 all off.  GV needs a variance: where
    fewer than three states with frames that pass the mask stay switched on, the switch is all on, and where that
    does not do either, all off (gv_length = 0: no GV for this utterance)."""
    S = len(dur)
    live = (dur > 0) & ((stream.msd > stream.msd_threshold) if stream.is_msd else np.ones(S, bool))
    for sw in ([np.ones(S, bool), rng.random(S) >= 0.3, np.zeros(S, bool)][variant], np.ones(S, bool)):
        if variant == 2 or (sw & live).sum() >= 3:
            return sw.astype(np.uint8)
    return np.zeros(S, np.uint8)


def all_off_sources(is_msd):
    """The utterances a GV-on case repeats with every switch off: all_voiced and runs_1_to_17, or the fifth and eighth
    length."""
    return (0, 4) if is_msd else (4, 7)


@functools.lru_cache(maxsize=None)
def build_case(wset, shape, use_gv, quirk=False) -> Case:
    windows = (QUIRK_WINDOW_SETS if quirk else WINDOW_SETS)[wset]
    L, is_msd = SHAPES[shape]
    W = len(windows)
    rng = np.random.default_rng(_seed(wset, shape))  # not of use_gv: the GV-on and GV-off cases share their inputs
    grng = np.random.default_rng(_seed(wset, shape, "gv", GV_SALT))
    case = Case(wset, shape, use_gv, windows, L, is_msd, tag="-quirk" if quirk else "")
    if is_msd:
        items = msd_patterns(rng)
    else:
        items = [("T%d" % T, _states_of_length(rng, T), 0.5) for T in lengths_without_msd(band_width(windows))]
    gv_mean, gv_var = grng.uniform(*GV_MEAN, L), grng.uniform(*GV_VAR, L)
    for i, (name, states, thr) in enumerate(items):
        dur, mean, var, msd = _draw(rng, states, thr, L, W)
        s = R.Stream(L, windows, mean, var, msd if is_msd else None, thr)
        if use_gv:
            s.gv_mean, s.gv_var = gv_mean, gv_var
            s.gv_switch = _gv_switch(grng, s, dur, i % 2)
            s.gv_weight = (1.0, 0.7, 0.7, 1.0)[i % 4]
        case.utts.append(Utt(name, dur, s))
    if use_gv:  # all switches off, on two utterances that have voiced frames to spare
        for u in [case.utts[k] for k in all_off_sources(is_msd)]:
            s = R.Stream(**{**u.stream.__dict__, "gv_switch": np.zeros(len(u.durations), np.uint8)})
            case.utts.append(Utt(u.name + "_gv_all_off", u.durations, s))
    return case


def long_msd_case() -> Case:
    """One long MSD utterance, L = 4 with GV: about 2,055 voiced frames of about 2,600, one time-parallel GV tile
    (2,048 frames) plus its halo after compaction.  Compared with the oracle only."""
    rng = np.random.default_rng(_seed("long"))
    case = Case("nitech_1_3_3", "L4_msd", True, WINDOW_SETS["nitech_1_3_3"], 4, True, tag="-long")
    lens = [int(x) for x in rng.integers(1, 60, 200)]
    lens = lens[:int(np.searchsorted(np.cumsum(lens), 2055))]
    lens.append(2055 - sum(lens))  # (1..59 frames as well)
    assert all(n > 0 for n in lens) and sum(lens) == 2055
    states = []
    for i, n in enumerate(lens):
        states += ([] if i == 0 else _split(rng, int(rng.integers(1, 14)), "U")) + _split(rng, n, "V")
    dur, mean, var, msd = _draw(rng, states, 0.5, 4, 3)
    s = R.Stream(4, case.windows, mean, var, msd, 0.5, rng.uniform(*GV_MEAN, 4), rng.uniform(*GV_VAR, 4),
                 (rng.random(len(dur)) >= 0.3).astype(np.uint8), 1.0)
    case.utts.append(Utt("long", dur, s))
    return case


# ---- the dense reference and the oracle, once per process ----

def dense_dims(case: Case, n_voiced):
    if case.L <= 4 or n_voiced <= DENSE_DIMS_ABOVE:
        return list(range(case.L))
    return [0, 1, case.L // 2, case.L - 1]  # every dim runs the same code; the oracle comparison covers them all


@functools.lru_cache(maxsize=None)
def _dense_nogv(wset, shape, i):
    case = build_case(wset, shape, False)
    u = case.utts[i]
    n = int(R.voiced_mask(u.stream, u.durations).sum())
    dims = dense_dims(case, n)
    vidx, systems = R.dense_system(u.stream, u.durations, dims)
    sols = [R.solve(A, b) for A, b in systems]
    conds = [R.cond_inf(A) for A, _ in systems]
    return vidx, dims, systems, sols, conds


@functools.lru_cache(maxsize=None)
def dense(wset, shape, use_gv, i):
    """dict(vidx, dims, systems [(A, b)], x [solution without GV], cond, par [with this case's GV], margin [min
    relative objective change of the ascent]) for utterance i of the case."""
    case = build_case(wset, shape, use_gv)
    n_base = len(build_case(wset, shape, False).utts)
    src = i if i < n_base else all_off_sources(case.is_msd)[i - n_base]  # the all-off copies
    vidx, dims, systems, sols, conds = _dense_nogv(wset, shape, src)
    out = dict(vidx=vidx, dims=dims, systems=systems, x=sols, cond=conds, par=sols, margin=[float("inf")] * len(dims))
    if use_gv and len(vidx):
        u = case.utts[i]
        sw = R.gv_switch_frames(u.stream, u.durations, vidx)
        res = [R.gv_ascent(A, b, x, sw, R.LD(u.stream.gv_mean[d]) * R.LD(u.stream.gv_weight), u.stream.gv_var[d],
                           len(case.windows)) for d, (A, b), x in zip(dims, systems, sols)]
        out["par"], out["margin"] = [r[0] for r in res], [r[1] for r in res]
    return out


def oracle_stream(s: R.Stream, S):
    from oracle import oracle as O

    return O.StreamStates(s.L, len(s.windows), int(s.is_msd), int(s.use_gv), [len(w) for w in s.windows],
                          [c for w in s.windows for c in w], s.mean, s.var,
                          s.msd if s.is_msd else np.full(S, DMAX), s.gv_mean, s.gv_var, s.gv_switch, s.gv_weight,
                          s.msd_threshold)


_oracle_tracks = {}


def oracle_track(case: Case, i):
    """The oracle's [T][L] track of utterance i, computed once."""
    from oracle import oracle as O

    key = (case.name, i)
    if key not in _oracle_tracks:
        u = case.utts[i]
        _oracle_tracks[key] = O.mlpg(oracle_stream(u.stream, len(u.durations)), u.durations)
    return _oracle_tracks[key]
