"""Cost of loudness normalization (jb_batch_set_loudness_target; jb_loudness.hip), in one process: on BASELINE
config 2 (256 copies of a 128 s utterance, native rate) the four modes alternate round by round -- f64 without and with
a target, 16-bit without and with one -- each step timed on its own with HIP events (jb_batch_run_timed: the launch
sequence including the measure and apply kernels); the feature's share is the step's excess over the same sink's
step without a target in the same round.  Also printed: the bytes the new kernels move and the floor that gives at
6.3 TB/s (one read to measure, one read and one write to apply).  The kernels alone: run this under
rocprofv3 --kernel-trace --stats with --rounds 1.

    python tools/loudness_cost.py [--rounds 2] [--steps 4] [--target -16]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--target", type=float, default=-16.0)
args = ap.parse_args()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256
frames = sum(int(np.sum(u.durations)) for u in utts)
N = frames * vi.fperiod
print(f"config 2: {len(utts)} utterances, {frames} frames, {N} samples at {vi.sampling_frequency} Hz; "
      f"{args.rounds} rounds x {args.steps} timed steps per mode after one untimed step; modes alternate within a round")

modes = [("f64", False, False), ("f64+target", False, True), ("i16", True, False), ("i16+target", True, True)]
ms = {m[0]: [] for m in modes}
excess = {"f64+target": [], "i16+target": []}
res = None
for _ in range(args.rounds):
    base = {}
    for name, i16, on in modes:
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=i16) as b:
            if on:
                b.set_loudness_target(args.target, 0.0)
            b.run_timed()
            t = [b.run_timed()[0] for _ in range(args.steps)]
            if on:
                res = b.loudness(0)
        ms[name] += t
        if not on:
            base[i16] = float(np.median(t))
        else:
            excess[name].append(float(np.median(t)) - base[i16])
        print(f"  {name:>10}: step ms {' '.join(f'{x:.2f}' for x in t)}")
print(f"  (utterance 0: L {res[0]:.3f} LUFS, P {res[1]:.3f} dBFS, gain {res[2]:+.3f} dB)")
print("\nconfig-2 step (device time, HIP events), median over rounds:")
for name, _, _ in modes:
    ex = f"; excess over the same sink without a target: {np.median(excess[name]):.2f} ms" if name in excess else ""
    print(f"  {name:>10}: {np.median(ms[name]):8.2f} ms{ex}")

bw = 6.3e12
measure = 2 * N * 8           # both tile passes read every sample
apply64, apply16 = N * 8 + N * 8, N * 8 + N * 2
print("\nbytes the new kernels move (HBM, by construction):")
print(f"  measure (k_ln_tiles x2): {measure / 1e9:.2f} GB  (floor of the issue: one read, {N * 8 / 1e9:.2f} GB = "
      f"{N * 8 / bw * 1e3:.2f} ms)")
print(f"  apply f64: {apply64 / 1e9:.2f} GB = {apply64 / bw * 1e3:.2f} ms at 6.3 TB/s; "
      f"apply 16-bit: {apply16 / 1e9:.2f} GB = {apply16 / bw * 1e3:.2f} ms")
print(f"  floor (one read to measure + apply): f64 {(N * 8 + apply64) / bw * 1e3:.2f} ms, "
      f"16-bit {(N * 8 + apply16) / bw * 1e3:.2f} ms; this design's traffic: f64 {(measure + apply64) / bw * 1e3:.2f} ms, "
      f"16-bit {(measure + apply16) / bw * 1e3:.2f} ms")
