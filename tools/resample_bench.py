"""Cost of the output-rate conversion (jb_batch_set_output_rate, k_resample), in one process: on BASELINE config 2
(256 copies of a 128 s utterance) the rates alternate round by round -- native, 16, 22.05, 24 and 44.1 kHz -- each step
timed on its own with HIP events (jb_batch_run_timed: the launch sequence including the converter); the converter's
share is the step's excess over the native step of the same round.  Then the step with the 16-bit PCM on the host
(run + sync + the staged read into touched buffers, wall clock) at 48 kHz against 16 kHz, and one sentence through
jb_synthesize at 16 kHz against native.  The converter kernel alone: run this under rocprofv3 --kernel-trace --stats
with --rates 16000.

    python tools/resample_bench.py [--rounds 2] [--steps 4] [--rates 0,16000,22050,24000,44100] [--no-host]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402
from tests.golden.labels import SAMPLE_SENTENCE_1  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--rates", default="0,16000,22050,24000,44100")
ap.add_argument("--no-host", action="store_true", help="skip the host-visible and sentence measurements")
args = ap.parse_args()
rates = [int(r) for r in args.rates.split(",")]

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256
frames = sum(int(np.sum(u.durations)) for u in utts)
print(f"config 2: {len(utts)} utterances, {frames} frames, {frames * vi.fperiod} samples at {vi.sampling_frequency} Hz; "
      f"{args.rounds} rounds x {args.steps} timed steps per rate after one untimed step; rates alternate within a round")

ms = {r: [] for r in rates}
excess = {r: [] for r in rates}
for _ in range(args.rounds):
    base = None
    for r in rates:
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if r:
                b.set_output_rate(r)
            b.run_timed()
            t = [b.run_timed()[0] for _ in range(args.steps)]
            ms[r] += t
            if r == 0:
                base = float(np.median(t))
            elif base is not None:
                excess[r].append(float(np.median(t)) - base)
            n_out = b.total_samples
        print(f"  rate {r or 'native':>6}: step ms {' '.join(f'{x:.2f}' for x in t)}; {n_out} output samples")
print("\nconfig-2 step (device time, HIP events), median over rounds:")
for r in rates:
    ex = f"; converter = step - native step of the round: {np.median(excess[r]):.2f} ms" if excess[r] else ""
    print(f"  {r or 'native':>6}: {np.median(ms[r]):8.2f} ms{ex}")

if not args.no_host:
    print("\nconfig-2 step with the 16-bit PCM on the host (run + sync + staged read, wall clock), alternating:")
    wall = {0: [], 16000: []}
    bufs = {}
    for _ in range(args.rounds):
        for r in (0, 16000):
            with J.Batch(vi, utts, pdf_set=pset, pcm_i16=True) as b:
                if r:
                    b.set_output_rate(r)
                if r not in bufs:
                    bufs[r] = [np.ones(b.num_samples(i), dtype=np.int16) for i in range(len(utts))]
                b.run()
                b.pcm_all(bufs[r])
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    b.run()
                    b.pcm_all(bufs[r])
                    wall[r].append((time.perf_counter() - t0) * 1e3)
    for r in (0, 16000):
        print(f"  {'48000' if r == 0 else r:>6} Hz: {np.median(wall[r]):8.2f} ms "
              f"({sum(x.size for x in bufs[r]) * 2 / 1e9:.2f} GB of 16-bit PCM)")

    print("\none sentence through jb_synthesize (wall clock, median of 20 warm calls):")
    for r in (0, 16000):
        e = eng.clone()
        e.condition.set_output_sampling_frequency(r)
        e.synthesize(SAMPLE_SENTENCE_1)
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            pcm = e.synthesize(SAMPLE_SENTENCE_1)
            t.append((time.perf_counter() - t0) * 1e3)
        print(f"  {'native' if r == 0 else r:>6}: {np.median(t):7.2f} ms, {pcm.size} samples")
