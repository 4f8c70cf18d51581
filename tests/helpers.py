"""Shared test helpers: build state-level inputs with the ORACLE's front half and
hand the very same arrays to the HIP library."""
from __future__ import annotations

import json
import os

import numpy as np

import jbonsai_amd as J
from oracle import oracle as O

# ONE tolerance, stated once (VERDICT r5 "next" 5).  The vocoder runs an utterance as time-chunks and CERTIFIES every
# hand-off on the filter STATE: max|delta| <= VERIFY_TOL * max|state| (jb_batch_opts.verify_tol; the library's default:
# tests/test_abi.py holds this constant against jb_default_verify_tol() -- not asked here, at import, because loading
# the library while pytest COLLECTS would put its HIP runtime into the process before torch's, which later test modules
# import: with the two in that order hipOccupancyMaxActiveBlocksPerMultiprocessor answered 0 for every kernel).  The PCM behind a certified hand-off carries that difference while it decays; relative RMS of
# a whole utterance against the oracle, measured: worst 1.13e-9 over the 2,400 utterances of tests/tools/shape_sweep.py
# (orders 2-61, post-filter up to 0.5), 3.0e-10 over the 2,400 of parity_sweep.py, 3.4e-12 on BASELINE config 2's.
# The gate of every PCM comparison in tests/ and tests/tools/ is therefore 2 x VERIFY_TOL (north_star allows 1e-4).
# The excitation is feed-forward (no hand-off): its gate is absolute, on values of O(1..30).
VERIFY_TOL = 1e-9
PCM_TOL = 2.0 * VERIFY_TOL
EXC_TOL = 1e-9
# The local gate (assert_pcm_close).  Relative RMS dilutes an error confined to a few frames by sqrt(frames affected /
# frames): on a 25,546-frame utterance one whole 153-frame chunk may be off by 2.6e-8 of the utterance's RMS and pass
# PCM_TOL, one frame by 3e-7.  frame_err is the worst frame's RMS difference over the utterance's RMS.  A certified
# hand-off itself leaves up to ~2e-8 there: its bound is relative to max|state|, which is far above the RMS.  Measured
# on the MI355X, 2026-10-15 (profiles/r07_*_local_err_sweep.txt): worst 2.03e-8 on the nitech shapes --
# tests/test_gpu_boundaries.py::test_fast_invariant_geometry, 14,592 frames, frame 12,163 = 3 frames behind a seam of
# its 152-frame chunks (rel RMS 2.5e-10); 1.17e-8 over the 2,400 utterances of tests/tools/parity_sweep.py (3,277
# frames, 3 frames behind a seam).  Other shapes stay below that: worst 1.58e-8 over the 2,400 of shape_sweep.py
# (beta 0.5, nmcp 48; nmcp > 40 without post-filter 9.2e-9), 1.4e-9 on the MGLSA paths -- no path needs a constant of
# its own.  The gate is 4 x the nitech worst, rounded down.
LOCAL_TOL = 8e-8


def voice_info(v: "O.Voice", volume: float = 1.0, beta: float = 0.0) -> J.VoiceInfo:
    streams = [J.StreamInfo(v.vector_length[i], bool(v.is_msd[i]), bool(v.use_gv[i]), v.windows[i])
               for i in range(v.nstream)]
    return J.VoiceInfo(v.fs, v.fperiod, v.alpha, streams, volume=volume, beta=beta)


def oracle_states(v: "O.Voice", labels, speed=1.0, gv_weight=(1.0, 1.0, 1.0),
                  msd_threshold=(0.5, 0.5, 0.5)):
    dur = v.durations(labels, speed)
    sts = [v.stream_states(i, labels, gv_weight[i], msd_threshold[i]) for i in range(v.nstream)]
    return dur, sts


def to_utt(dur, sts) -> J.Utterance:
    out = []
    for s in sts:
        out.append(J.StreamStates(s.mean, s.var, s.msd if s.is_msd else None, s.gv_mean, s.gv_var,
                                  s.gv_switch, s.gv_weight, s.msd_threshold))
    return J.Utterance(dur, out)


def oracle_run(v: "O.Voice", dur, sts, volume=1.0, dumps=False, beta=0.0):
    """MLPG x3 + vocoder with the oracle on flat state arrays."""
    tracks = [O.mlpg(s, dur) for s in sts]
    r = O.vocoder(v.fs, v.fperiod, v.alpha, volume, tracks[1][:, 0], tracks[0], tracks[2], dumps=dumps,
                  beta=beta)
    return tracks, r


def rel_rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.sqrt(np.mean(b * b))
    return float(np.sqrt(np.mean((a - b) ** 2)) / (den if den > 0 else 1.0))


def frame_err(got, want, fperiod):
    """(max over frames f of rms(got - want over the samples of f) / rms(want over the whole utterance), that frame).
    Normalised by the utterance's RMS, not the frame's own: a silent frame does not dominate."""
    a, b = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert a.shape == b.shape and a.ndim == 1, (a.shape, b.shape)
    if b.size == 0:
        return 0.0, 0
    den = np.sqrt(np.mean(b * b))
    nf = -(-b.size // fperiod)
    d2 = np.zeros(nf * fperiod)
    d2[:b.size] = (a - b) ** 2
    n = np.full(nf, float(fperiod))
    n[-1] = b.size - (nf - 1) * fperiod
    per = np.sqrt(d2.reshape(nf, fperiod).sum(axis=1) / n) / (den if den > 0 else 1.0)
    f = int(np.argmax(per))
    return float(per[f]), f


def assert_pcm_close(got, want, fperiod, tol=None, local=None, what="", chunk=None):
    """The PCM gate: equal lengths, rel_rms <= tol (PCM_TOL) over the utterance and frame_err <= local (LOCAL_TOL) in
    every frame.  `chunk`: the chunk length in frames, when known -- the message then says where in its chunk the
    worst frame sits (an error at offset 0.. just after a seam is a hand-off's).  JB_PCM_LOG=<file> appends one JSON
    line per call (the test, `what`, both numbers): how LOCAL_TOL was measured."""
    tol = PCM_TOL if tol is None else tol
    local = LOCAL_TOL if local is None else local
    got, want = np.asarray(got), np.asarray(want)
    assert len(got) == len(want), f"{what}: {len(got)} samples against {len(want)}"
    e = rel_rms(got, want)
    fe, f = frame_err(got, want, fperiod)
    where = f"frame {f}" + (f" (chunk {f // chunk}, offset {f % chunk} of {chunk})" if chunk else "")
    log = os.environ.get("JB_PCM_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(json.dumps(dict(test=os.environ.get("PYTEST_CURRENT_TEST", ""), what=str(what), frames=len(want) // fperiod,
                                     rel_rms=e, frame_err=fe, frame=f, tol=tol, local=local)) + "\n")
    assert e <= tol, f"{what}: rel RMS {e:.3e} > {tol:g} (worst frame {fe:.3e} at {where})"
    assert fe <= local, f"{what}: frame error {fe:.3e} > {local:g} at {where}; rel RMS {e:.3e}"
