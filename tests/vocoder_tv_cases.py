"""The case table of the time-varying vocoder tests (tests/test_vocoder_tv_ref.py without a GPU,
tests/test_gpu_vocoder_tv.py with one; the reference is tests/vocoder_tv_ref.py).  Seeded by name, as tests/mlsa_cases.py.

EXCITATION SHAPES (fperiod, nlpf, taps): one batch of five utterances each --
  glide    every frame voiced, the period gliding from about 0.3 to 1.3 frame periods
  noise    every frame unvoiced
  runs     voiced runs of 1, 2 and 3 frames between unvoiced gaps of 1 and 2 frames; the one-frame runs carry an lf0
           below MIN_LF0, which the vocoder clamps (a period of 800 samples at 16 kHz: above every frame period here)
  octave   from a period of 4.3 samples upwards, doubling every two frames, and down again
  one      a single voiced frame (shorter than the taps where nlpf > fperiod)
and the shapes reach every launch branch of launch_excite (jb_vocoder.hip) and its boundaries: the split form (240, 31),
(80, 15), (32, 31) with taps constant over the frames (the shared table) and different in every frame (the per-frame
pass); the staged kernel's edges (30, 31), (64, 64), (37, 2), (65, 64), an even tap count (80, 16) for the antipode's
floor, one tap other than 1 (80, 1); k_excite_any below 30 samples (29, 15), one tap past 64 (64, 65), nlpf - 1 =
fperiod + 1 (37, 39), and 2047 taps over 70 frames of 37 samples, whose window reaches back over 56 frames; nlpf = 0.
The taps are a low-pass bump plus noise, per frame where the shape says so.

FILTER SHAPES: a subset of mlsa_cases' grid with ALL rows moving, three utterances each (glide, runs, octave) on a mixed
excitation of 31 or 15 taps, different in every frame (one shape with one tap, one without a ring buffer, and one,
`_table`, with ONE row of taps for the whole batch, so that the split form's shared table feeds a moving filter).  A
cepstrum track is the shape's base row plus an AR(1) walk whose frame-to-frame step is 0.2 / sqrt(k): the step in the
low orders is a few tenths, a sizeable share of the row.  LSP rows are jittered per frame inside the ordering mlsa_cases._lsp_row keeps.  Two
Stage::Zero shapes run under a post-filter (beta 0.1, 0.3).

Every pitch track keeps every comparison of the pulse counter 1e-6 samples clear of a tie (asserted where a case is
built: no case may be skipped); a name whose first draw did not is listed in RESEED with the draw that does."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

from tests import mlsa_cases as C
from tests import mlsa_ref as R
from tests import vocoder_tv_ref as V

FS = 16000
MARGIN = 1e-6
KINDS = ("glide", "noise", "runs", "octave", "one")
FILTER_KINDS = ("glide", "runs", "octave")
CLAMPED_LF0 = 2.9  # below MIN_LF0

# name: (fperiod, nlpf, taps per frame, frames)
EXC_SHAPES = {
    "split_f240_l31": (240, 31, False, 12),
    "split_f240_l31_frame": (240, 31, True, 12),
    "split_f80_l15": (80, 15, False, 24),
    "split_f80_l15_frame": (80, 15, True, 24),
    "split_f32_l31": (32, 31, False, 40),
    "split_f32_l31_frame": (32, 31, True, 40),
    "staged_f30_l31": (30, 31, True, 40),
    "staged_f64_l64": (64, 64, True, 24),
    "staged_f37_l2": (37, 2, True, 40),
    "staged_f65_l64": (65, 64, True, 24),
    "staged_f80_l16": (80, 16, True, 24),
    "staged_f80_l1": (80, 1, True, 24),
    "any_f29_l15": (29, 15, True, 40),
    "any_f64_l65": (64, 65, True, 24),
    "any_f37_l39": (37, 39, True, 40),
    "any_f37_l2047": (37, 2047, False, 70),
    "nolpf_f80": (80, 0, False, 24),
}
# name: (stage, nmcp, alpha, fperiod, volume, frames, beta, nlpf, log gain)
FILTER_SHAPES = {
    "z3_a55_f37": (0, 3, 0.55, 37, 1.0, 24, 0.0, 15, False),
    "z5_a42_f65": (0, 5, 0.42, 65, 1.0, 20, 0.0, 31, False),
    "z25_a0_f64": (0, 25, 0.0, 64, 1.0, 20, 0.0, 31, False),
    "z35_a55_f240": (0, 35, 0.55, 240, 1.7, 12, 0.0, 31, False),
    "z35_a42_f80_l1": (0, 35, 0.42, 80, 1.0, 16, 0.0, 1, False),
    "z25_a42_f240_nolpf": (0, 25, 0.42, 240, 1.0, 12, 0.0, 0, False),
    "slow_z50_a77_f80": (0, 50, 0.77, 80, 1.0, 30, 0.0, 15, False),
    "z64_a55_f80": (0, 64, 0.55, 80, 1.0, 16, 0.0, 31, False),
    "z25_a55_f80_table": (0, 25, 0.55, 80, 1.0, 16, 0.0, 15, False),
    "zb1_n25_a42_f80": (0, 25, 0.42, 80, 1.0, 16, 0.1, 15, False),
    "zb3_n35_a55_f65": (0, 35, 0.55, 65, 1.0, 16, 0.3, 31, False),
    "g1_n9_a42_f80": (1, 9, 0.42, 80, 1.0, 16, 0.0, 15, False),
    "g4_n13_a55_f65": (4, 13, 0.55, 65, 1.0, 16, 0.0, 31, True),
    "g8_n24_a42_f37": (8, 24, 0.42, 37, 1.0, 24, 0.0, 15, False),
    "g9_n21_a30_f80": (9, 21, 0.3, 80, 1.0, 16, 0.0, 31, False),
}
BETA_SHAPES = [s for s, v in FILTER_SHAPES.items() if v[6] > 0.0]
RESEED = {}  # case name: draw
# the oracle's worst distance per class (profiles/r26_vocoder_tv.txt), the host gates at 8 x that, the bound on the
# reference's agreement with mlsa_ref, and the frozen cases it is measured on (tests/test_vocoder_tv_ref.py)
WORST = dict(exc=4.91e-15, zero=158.0, zero_beta=48.4, mglsa=4198.0)
GATE = {k: 8 * v for k, v in WORST.items()}
AGREE_U = 4.0
FROZEN = [("n4_a0_f64", "vuv"), ("n35_a55_f240", "pulses"), ("slow_n50_a77_f80", "noise"), ("n64_a55_f80", "vuv"),
          ("mglsa_s4_n35_a55", "vuv"), ("mglsa_s9_n21_a30", "pulses"), ("ramp_noise_n35_a55_f80", None),
          ("ramp_pulses_n35_a42_f65", None)]


@dataclass
class Utt:
    name: str
    fperiod: int
    lf0: np.ndarray   # [T] f64, NODATA = unvoiced
    lpf: np.ndarray   # [T][nlpf] f64
    spectrum: np.ndarray = None  # [T][nmcp] f64 (filter shapes)

    @property
    def frames(self):
        return len(self.lf0)

    @property
    def samples(self):
        return len(self.lf0) * self.fperiod

    @property
    def voiced(self):
        return self.lf0 != R.NODATA


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _lf0_track(kind, T, fperiod, rng):
    """[T] f64 with NODATA in unvoiced frames."""
    lp = lambda p: np.log(FS / np.asarray(p, dtype=np.float64))
    if kind == "noise":
        return np.full(T, R.NODATA)
    if kind in ("glide", "one"):
        p = np.geomspace(0.3 * fperiod, 1.3 * fperiod, T) * np.exp(rng.uniform(-0.06, 0.06, T))
        return lp(p)
    if kind == "octave":
        up = 4.3 * 2.0 ** (np.arange(T) / 2.0)
        return lp(np.minimum(np.minimum(up, up[::-1]), 700.0) * np.exp(rng.uniform(-0.03, 0.03, T)))
    assert kind == "runs"
    pattern = [0, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0]
    v = np.array([pattern[t % len(pattern)] for t in range(T)], dtype=bool)
    lf0 = lp(rng.uniform(0.2 * fperiod, 1.1 * fperiod, T))
    alone = v & ~np.concatenate(([False], v[:-1])) & ~np.concatenate((v[1:], [False]))
    lf0[alone] = CLAMPED_LF0
    return np.where(v, lf0, R.NODATA)


def _taps(nlpf, T, per_frame, rng):
    """[T][nlpf]: a low-pass bump around the antipode plus noise."""
    if nlpf == 0:
        return np.zeros((T, 0))
    if nlpf == 1:
        base = np.array([0.7])
    else:
        k = np.arange(nlpf) - (nlpf - 1) // 2
        base = 0.5 * np.sinc(k / 4.0) * np.hanning(nlpf + 2)[1:-1] / 2.0 + 0.3 * rng.standard_normal(nlpf) / np.sqrt(nlpf)
    if not per_frame:
        return np.tile(base, (T, 1))
    return base[None, :] * (1.0 + 0.3 * rng.standard_normal((T, nlpf))) + 0.05 * rng.standard_normal((T, nlpf)) / np.sqrt(nlpf)


def _checked(name, make):
    """make(rng) -> Utt, drawn with the name's seed (or RESEED's); its margin is asserted."""
    u = make(_rng(name if name not in RESEED else "%s#%d" % (name, RESEED[name])))
    margin = V.pulses(V.periods(u.lf0, FS), u.fperiod)[1]
    assert margin >= MARGIN, ("a pulse decision of %s is within %g of a tie: list another draw in RESEED" % (name, margin))
    return u, margin


@functools.lru_cache(maxsize=None)
def exc_utt(shape, kind):
    fperiod, nlpf, per_frame, T = EXC_SHAPES[shape]
    T = 1 if kind == "one" else T
    name = "%s-%s" % (shape, kind)

    def make(rng):
        taps = _taps(nlpf, EXC_SHAPES[shape][3], per_frame, _rng(shape + "/taps"))[:T]  # one table per shape when constant
        return Utt(name, fperiod, _lf0_track(kind, T, fperiod, rng), taps)
    return _checked(name, make)


def exc_cases(shape):
    return [exc_utt(shape, k)[0] for k in KINDS]


def _cepstrum_track(rng, base, T):
    k = np.arange(1, len(base))
    dev = np.zeros((T, len(base)))
    for t in range(T):
        step = 0.2 * rng.standard_normal(len(base)) / np.concatenate(([1.0], np.sqrt(k)))
        dev[t] = (0.8 * dev[t - 1] if t else 0.0) + step
    return base[None, :] + dev


def _lsp_track(rng, nmcp, T):
    base = C._lsp_row(rng, nmcp)
    h = np.pi / nmcp
    rows = np.tile(base, (T, 1))
    rows[:, 1:] += h * rng.uniform(-0.1, 0.1, (T, nmcp - 1))  # |0.08| + |0.1| < 0.5: the ordering holds
    rows[:, 0] = rng.uniform(0.02, 0.08, T)
    assert np.all(np.diff(rows[:, 1:], axis=1) > 0) and np.all(rows[:, 0] < rows[:, 1])
    return rows


@functools.lru_cache(maxsize=None)
def filter_utt(shape, kind):
    stage, nmcp, alpha, fperiod, volume, T, beta, nlpf, log_gain = FILTER_SHAPES[shape]
    name = "%s-%s" % (shape, kind)

    def make(rng):
        if stage:
            spec = _lsp_track(rng, nmcp, T)
        else:
            base = C.build_case("slow_n50_a77_f80", "pulses").mc[0] if shape.startswith("slow") else C._cepstrum(rng, nmcp)
            spec = _cepstrum_track(rng, base, T)
        lf0 = _lf0_track(kind, T, fperiod, rng)
        taps = _taps(nlpf, T, False, _rng(shape + "/taps")) if shape.endswith("_table") else _taps(nlpf, T, True, rng)
        return Utt(name, fperiod, lf0, taps, np.ascontiguousarray(spec))
    return _checked(name, make)


def filter_cases(shape):
    return [filter_utt(shape, k)[0] for k in FILTER_KINDS]


def margins():
    """{case name: margin} of the whole table."""
    out = {}
    for s in EXC_SHAPES:
        for k in KINDS:
            out["%s-%s" % (s, k)] = exc_utt(s, k)[1]
    for s in FILTER_SHAPES:
        for k in FILTER_KINDS:
            out["%s-%s" % (s, k)] = filter_utt(s, k)[1]
    return out


@functools.lru_cache(maxsize=None)
def noise():
    from oracle import oracle as O

    return O.noise(max(max(u.samples for u in exc_cases(s)) for s in EXC_SHAPES) + 240 * 40)


# ---- references, once per process, read-only ------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_excitation(shape, kind, filt=False):
    u = (filter_utt if filt else exc_utt)(shape, kind)[0]
    return _frozen(V.excitation(u.lf0, FS, u.fperiod, u.lpf, noise())[0])


def oracle_excitation(u):
    from oracle import oracle as O

    spec = np.zeros((u.frames, 3))
    return O.vocoder(FS, u.fperiod, 0.42, 1.0, u.lf0, spec, u.lpf if u.lpf.shape[1] else None, dumps=True)[1]


def exc_err(got, want):
    """max |got - want| over the case's peak, evaluated in long double."""
    want = np.asarray(want, dtype=R.LD)
    return float(np.abs(np.asarray(got, dtype=R.LD) - want).max() / np.abs(want).max())


def oracle_rows(shape, u):
    """MGLSA: (rows [T][nmcp], first [nmcp]) as the oracle converts the LSP track (the conversion is coef_ref's business)."""
    from oracle import oracle as O

    stage, nmcp, alpha, _, _, _, beta, _, log_gain = FILTER_SHAPES[shape]
    rows = np.array([O.stage_coefficients(r, alpha, beta, log_gain, stage, filtered=True) for r in u.spectrum])
    return rows, O.stage_coefficients(u.spectrum[0], alpha, beta, log_gain, stage, filtered=False)


def reference_pcm(shape, utts, rows=None, firsts=None, beta=None):
    """[PCM long double per utterance] of a filter shape.  Stage::Zero: from the spectrum tracks (beta: the shape's
    unless given).  MGLSA: from the coefficient rows the caller gives."""
    stage, nmcp, alpha, fperiod, volume, T, b, nlpf, log_gain = FILTER_SHAPES[shape]
    es = [expected_excitation(shape, u.name.rsplit("-", 1)[1], True) for u in utts]
    if not stage:
        rf = [V.zero_rows(u.spectrum, alpha, b if beta is None else beta) for u in utts]
        rows, firsts = [r for r, _ in rf], [f for _, f in rf]
    return [_frozen(p) for p in V.synthesize(es, rows, firsts, fperiod, alpha, volume, stage)]


@functools.lru_cache(maxsize=None)
def expected_pcm(shape, beta=None):
    """The table's own reference of a shape (MGLSA: on the oracle's coefficient rows), list over FILTER_KINDS."""
    utts = filter_cases(shape)
    if FILTER_SHAPES[shape][0]:
        rf = [oracle_rows(shape, u) for u in utts]
        return reference_pcm(shape, utts, [r for r, _ in rf], [f for _, f in rf])
    return reference_pcm(shape, utts, beta=beta)


def oracle_pcm(shape, u):
    from oracle import oracle as O

    stage, nmcp, alpha, fperiod, volume, T, beta, nlpf, log_gain = FILTER_SHAPES[shape]
    lpf = u.lpf if nlpf else None
    if stage:
        rows, first = oracle_rows(shape, u)
        return O.vocoder(FS, fperiod, alpha, volume, u.lf0, u.spectrum, lpf, stage=stage, use_log_gain=log_gain, coef=rows,
                         cfirst=first)
    return O.vocoder(FS, fperiod, alpha, volume, u.lf0, u.spectrum, lpf, beta=beta)


def filter_class(shape):
    stage, beta = FILTER_SHAPES[shape][0], FILTER_SHAPES[shape][6]
    return "mglsa" if stage else "zero_beta" if beta > 0.0 else "zero"
