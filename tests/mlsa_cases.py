"""The case table of the transfer-function tests of the synthesis filters (tests/test_mlsa_transfer.py without a GPU,
tests/test_gpu_mlsa_transfer.py with one; the reference is tests/mlsa_ref.py).

A SHAPE is what one vocoder is built for -- filter kind, nmcp, alpha, frame period, volume -- and holds one row of
coefficients that every frame repeats (the filter is then time-invariant).  A CASE is a shape with one excitation:
  pulses   every frame voiced at one constant pitch
  noise    every frame unvoiced
  vuv      one voiced / unvoiced / voiced pattern (the pitch restarts, the noise stream resumes)
so a shape is one batch of three utterances.  Stage::Zero: nmcp covers both ends of the range (2, 64) and every
remainder of (nmcp - 2) % 4, the taps the 4-way unrolled FIR leaves to its remainder loop; alpha 0 (mc2b is the
identity, the all-pass a delay), 0.42, 0.55, 0.77; the frame periods straddle the 64-sample block split of
plan_frame_blocks (37, 64, 65, 80, 240) and two are odd, which the lane-triple kernel does not take; two shapes have a
volume other than 1.  The cepstra decay like 1 / sqrt(k).  `slow` (order 49, alpha 0.77) rings for thousands of samples:
no 18-frame warm-up reproduces its state, so its hand-offs fail their check and its chunks are redone from the truth.
The two RAMP shapes vary mc[0] alone from frame to frame, which reaches the interpolation schedule through the input
gain (tests/mlsa_ref.py gain_schedule).  MGLSA: one to twelve stages -- the register kernel up to eight, the LDS kernel
above -- on one constant row of line spectral pairs."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np

from tests import mlsa_ref as R

EXCITATIONS = ("pulses", "noise", "vuv")

# name: (nmcp, alpha, fperiod, volume, frames)
ZERO_SHAPES = {
    "n2_a42_f80": (2, 0.42, 80, 1.0, 30),
    "n3_a55_f37": (3, 0.55, 37, 1.0, 40),
    "n4_a0_f64": (4, 0.0, 64, 1.0, 32),
    "n5_a42_f65": (5, 0.42, 65, 1.0, 32),
    "n6_a55_f240": (6, 0.55, 240, 1.0, 24),
    "n7_a77_f80": (7, 0.77, 80, 1.7, 30),
    "n25_a42_f240": (25, 0.42, 240, 1.0, 24),
    "n25_a55_f37": (25, 0.55, 37, 1.0, 40),
    "n35_a55_f240": (35, 0.55, 240, 1.0, 24),  # nitech's
    "n35_a42_f65": (35, 0.42, 65, 0.5, 32),
    "n35_a0_f80": (35, 0.0, 80, 1.0, 30),
    "n50_a55_f64": (50, 0.55, 64, 1.0, 32),
    "slow_n50_a77_f80": (50, 0.77, 80, 1.0, 40),
    "n64_a55_f80": (64, 0.55, 80, 1.0, 30),
    "n64_a77_f240": (64, 0.77, 240, 1.0, 24),
    "n64_a0_f37": (64, 0.0, 37, 1.0, 40),
}
# name: (nmcp, alpha, fperiod, frames, excitation)
RAMP_SHAPES = {
    "ramp_noise_n35_a55_f80": (35, 0.55, 80, 14, "noise"),
    "ramp_pulses_n35_a42_f65": (35, 0.42, 65, 24, "pulses"),
}
# name: (stage, nmcp, alpha, use_log_gain, fperiod, frames)
MGLSA_SHAPES = {
    "mglsa_s1_n9_a42": (1, 9, 0.42, False, 80, 30),
    "mglsa_s2_n13_a55": (2, 13, 0.55, True, 80, 30),
    "mglsa_s4_n35_a55": (4, 35, 0.55, False, 240, 24),
    "mglsa_s8_n24_a42": (8, 24, 0.42, False, 65, 32),
    "mglsa_s9_n21_a30": (9, 21, 0.3, False, 80, 30),
    "mglsa_s12_n16_a55": (12, 16, 0.55, True, 37, 40),
}
SHAPES = list(ZERO_SHAPES) + list(RAMP_SHAPES) + list(MGLSA_SHAPES)
FS = 16000
PITCH = 57.3137  # samples; every multiple in range stays 1e-6 clear of an integer (asserted in pulse_positions)


@dataclass
class Case:
    name: str
    shape: str
    exc: str
    stage: int          # 0: Stage::Zero (MLSA); > 0: the MGLSA cascade of that many stages
    nmcp: int
    alpha: float
    fperiod: int
    volume: float
    fs: int
    ramp: bool
    log_gain: bool
    mc: np.ndarray      # [T][nmcp] f64: the spectrum track (Stage::Zero: mel-cepstrum; MGLSA: [gain, LSP...])
    lf0: float          # of the voiced frames
    voiced: np.ndarray  # [T] bool

    @property
    def frames(self):
        return len(self.voiced)

    @property
    def samples(self):
        return len(self.voiced) * self.fperiod

    def lf0_track(self):
        return np.where(self.voiced, self.lf0, R.NODATA)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _voiced(exc, T):
    if exc == "pulses":
        return np.ones(T, dtype=bool)
    if exc == "noise":
        return np.zeros(T, dtype=bool)
    t = np.arange(T)
    return (t < T // 3) | (t >= T // 3 + max(2, T // 4))


def _cepstrum(rng, nmcp):
    k = np.arange(1, nmcp)
    return np.concatenate(([rng.uniform(-0.5, 1.0)], 0.5 * rng.standard_normal(nmcp - 1) / np.sqrt(k)))


def _lsp_row(rng, nmcp):
    """[gain, nmcp - 1 ordered frequencies]: an even grid, jittered (tests/test_gpu_stage.py lsp_utterance).  The
    reference's lsp2lpc takes the gain slot as a frequency too (lsp.rs:27-43): it stays below the first real one."""
    h = np.pi / nmcp
    w = h * (np.arange(1, nmcp) + rng.uniform(-0.08, 0.08, nmcp - 1))
    return np.concatenate(([rng.uniform(0.02, 0.08)], np.sort(w)))


@functools.lru_cache(maxsize=None)
def build_case(shape: str, exc: Optional[str] = None) -> Case:
    rng = _rng(shape)
    lf0 = float(np.log(FS / PITCH))
    if shape in ZERO_SHAPES:
        nmcp, alpha, fperiod, volume, T = ZERO_SHAPES[shape]
        mc = np.tile(_cepstrum(rng, nmcp), (T, 1))
        stage, ramp, log_gain = 0, False, False
    elif shape in RAMP_SHAPES:
        nmcp, alpha, fperiod, T, only = RAMP_SHAPES[shape]
        assert exc in (None, only)
        exc = only
        mc = np.tile(_cepstrum(rng, nmcp), (T, 1))
        mc[:, 0] = rng.uniform(-1.0, 1.0, T)
        stage, ramp, log_gain, volume = 0, True, False, 1.0
    else:
        stage, nmcp, alpha, log_gain, fperiod, T = MGLSA_SHAPES[shape]
        mc = np.tile(_lsp_row(rng, nmcp), (T, 1))
        ramp, volume = False, 1.0
    return Case("%s-%s" % (shape, exc), shape, exc, stage, nmcp, alpha, fperiod, volume, FS, ramp, log_gain,
                np.ascontiguousarray(mc), lf0, _voiced(exc, T))


def shape_cases(shape):
    if shape in RAMP_SHAPES:
        return [build_case(shape, RAMP_SHAPES[shape][4])]
    return [build_case(shape, e) for e in EXCITATIONS]


def all_cases():
    return [c for s in SHAPES for c in shape_cases(s)]


@functools.lru_cache(maxsize=None)
def noise():
    """The noise stream (O.noise: the reference's generator, pinned by its goldens), as long as the longest case."""
    from oracle import oracle as O

    n = max(c.samples for c in all_cases())
    return O.noise(n)


def oracle_coefficients(case):
    """MGLSA: the filter coefficients the oracle converts the case's LSP row to, [nmcp].  The row is chosen so that the
    post-filtered, stability-checked conversion of a frame (vocoder/mod.rs:148-155) equals the first frame's plain
    one (mod.rs:96-106) -- the filter is then constant from sample 0."""
    from oracle import oracle as O

    c = O.stage_coefficients(case.mc[0], case.alpha, 0.0, case.log_gain, case.stage, filtered=True)
    c0 = O.stage_coefficients(case.mc[0], case.alpha, 0.0, case.log_gain, case.stage, filtered=False)
    assert np.array_equal(c, c0), case.name
    return c


@functools.lru_cache(maxsize=None)
def _response(shape):
    case = shape_cases(shape)[0]
    return R.case_response(case, oracle_coefficients(case) if case.stage else None)


def response(case):
    """(h, N, margins) of the case's shape from the table's own coefficients, once per process."""
    return _response(case.shape)


@functools.lru_cache(maxsize=None)
def expected(name_shape, exc, nlpf):
    case = build_case(name_shape, exc)
    return R.expected_pcm(case, nlpf, noise(), response=response(case))


def expected_pcm(case, nlpf):
    """The reference PCM of a case with the table's own coefficients, once per process; left unchanged by its users."""
    out = expected(case.shape, case.exc, nlpf)
    out.setflags(write=False)
    return out


def oracle_pcm(case, nlpf):
    """The CPU oracle on the case: nlpf = 0 (no ring buffer) or 1 (lpf = [1.0])."""
    from oracle import oracle as O

    lpf = np.ones((case.frames, 1)) if nlpf else None
    if case.stage:
        c = oracle_coefficients(case)
        return O.vocoder(case.fs, case.fperiod, case.alpha, case.volume, case.lf0_track(), case.mc, lpf,
                         stage=case.stage, use_log_gain=case.log_gain, coef=np.tile(c, (case.frames, 1)), cfirst=c)
    return O.vocoder(case.fs, case.fperiod, case.alpha, case.volume, case.lf0_track(), case.mc, lpf)


def err_in_u(got, want):
    """max |got - want| in units of u * max |want|, evaluated in long double."""
    want = np.asarray(want, dtype=R.LD)
    peak = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=R.LD) - want).max() / (peak * R.LD(R.U)))
