"""Cost of the true-peak ceiling (jb_batch_set_peak_mode; jb_loudness.hip k_ln_true_peak), in one process: on BASELINE
config 2 (256 copies of a 128 s utterance) with a loudness target, sample mode and true-peak mode alternate round by
round at the native rate (48 kHz, F = 4) and at a 16 kHz output rate (F = 12) -- each step timed on its own with HIP
events (jb_batch_run_timed: the launch sequence including the converter, the measure and the apply kernels); the
mode's share is the step's excess over the sample-mode step at the same rate in the same round.  Also printed: the
bytes and FMAs the new kernel adds.  The kernels alone: run this under rocprofv3 --kernel-trace --stats with
--rounds 1.

    python tools/true_peak_cost.py [--rounds 2] [--steps 4] [--target -16] [--ceiling -1]"""
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
ap.add_argument("--ceiling", type=float, default=-1.0)
args = ap.parse_args()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256
frames = sum(int(np.sum(u.durations)) for u in utts)
N = frames * vi.fperiod
print(f"config 2: {len(utts)} utterances, {frames} frames, {N} samples at {vi.sampling_frequency} Hz; "
      f"{args.rounds} rounds x {args.steps} timed steps per mode after one untimed step; modes alternate within a round; "
      f"f64 sink, target {args.target} LUFS, ceiling {args.ceiling}")

modes = [("48k sample", 0, J.PEAK_SAMPLE), ("48k true", 0, J.PEAK_TRUE),
         ("16k sample", 16000, J.PEAK_SAMPLE), ("16k true", 16000, J.PEAK_TRUE)]
ms = {m[0]: [] for m in modes}
excess = {"48k true": [], "16k true": []}
reports = {}
n_out = {}
for _ in range(args.rounds):
    base = {}
    for name, hz, mode in modes:
        with J.Batch(vi, utts, pdf_set=pset) as b:
            b.set_loudness_target(args.target, args.ceiling)
            if hz:
                b.set_output_rate(hz)
            b.set_peak_mode(mode)
            b.run_timed()
            t = [b.run_timed()[0] for _ in range(args.steps)]
            reports[name] = b.loudness_report(0)
            n_out[hz] = b.total_samples
        ms[name] += t
        if mode == J.PEAK_SAMPLE:
            base[hz] = float(np.median(t))
        else:
            excess[name].append(float(np.median(t)) - base[hz])
        print(f"  {name:>10}: step ms {' '.join(f'{x:.2f}' for x in t)}")
for name, _, _ in modes:
    r = reports[name]
    print(f"  ({name}, utterance 0: L {r['lufs']:.3f} LUFS, P {r['sample_peak_dbfs']:.4f} dBFS, "
          f"TP {r['true_peak_dbtp']:.4f} dBTP, F {r['oversampling']}, gain {r['gain_db']:+.4f} dB)")
print("\nconfig-2 step (device time, HIP events), median over rounds:")
for name, _, _ in modes:
    ex = f"; excess over sample mode at the same rate: {np.median(excess[name]):.2f} ms" if name in excess else ""
    print(f"  {name:>10}: {np.median(ms[name]):8.2f} ms{ex}")

bw = 6.3e12
print("\nwhat k_ln_true_peak adds (by construction): one read of the measured f64 and 12 (F - 1) FMAs per sample")
for hz, F in ((0, 4), (16000, 12)):
    n = n_out[hz]
    print(f"  {hz or vi.sampling_frequency} Hz: {n} samples, {n * 8 / 1e9:.2f} GB = {n * 8 / bw * 1e3:.2f} ms at 6.3 TB/s; "
          f"{2 * 12 * (F - 1) * n / 1e12:.3f} TFLOP (F = {F})")
