"""Cost and benefit of FLAC output (jb_batch_set_flac; jb_flac.hip), in one process.  On BASELINE config 2 (256
copies of a 128 s utterance, 16-bit) the two modes alternate round by round -- 16-bit PCM without and with FLAC --
each step timed on its own with HIP events (jb_batch_run_timed: the launch sequence including the encoder); the
encoder's share is the step's excess over the same round's step without it.  Then the serial host-visible step
(run, sync, read everything: jb_batch_read_pcm_i16_all against jb_batch_read_flac_all) for both, and bytes per
sample on config 2 and on --distinct utterances.  Also printed: the floor of the encoder's HBM traffic at 6.3 TB/s.
The kernels alone: run this under rocprofv3 --kernel-trace --stats with --rounds 1.

    python tools/flac_cost.py [--rounds 2] [--steps 4] [--distinct 16]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--distinct", type=int, default=16, help="distinct 128 s utterances for the bytes-per-sample line")
args = ap.parse_args()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256
frames = sum(int(np.sum(u.durations)) for u in utts)
N = frames * vi.fperiod
print(f"config 2: {len(utts)} utterances, {frames} frames, {N} samples at {vi.sampling_frequency} Hz; "
      f"{args.rounds} rounds x {args.steps} timed steps per mode after one untimed step; modes alternate within a round")

ms = {"i16": [], "i16+flac": []}
excess, host = [], {"i16": [], "i16+flac": []}
nbytes = 0
for _ in range(args.rounds):
    base = None
    for name in ("i16", "i16+flac"):
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=True) as b:
            if name == "i16+flac":
                b.set_flac()
            b.run_timed()
            t = [b.run_timed()[0] for _ in range(args.steps)]
            # the serial host-visible step: run, sync, read everything
            t0 = time.perf_counter()
            b.run()
            b.sync()
            if name == "i16":
                b.pcm_all()
            else:
                streams = b.flac_all()
                nbytes = sum(len(s) for s in streams)
            host[name].append((time.perf_counter() - t0) * 1e3)
        ms[name] += t
        if base is None:
            base = float(np.median(t))
        else:
            excess.append(float(np.median(t)) - base)
        print(f"  {name:>9}: step ms {' '.join(f'{x:.2f}' for x in t)}; host-visible step {host[name][-1]:.1f} ms")

print("\nconfig-2 step (device time, HIP events), median over rounds:")
print(f"        i16: {np.median(ms['i16']):8.2f} ms")
print(f"   i16+flac: {np.median(ms['i16+flac']):8.2f} ms; encoder's excess {np.median(excess):.2f} ms")
print("serial host-visible step (run + sync + read everything), median:")
print(f"        i16: {np.median(host['i16']):8.1f} ms ({2 * N / 1e9:.2f} GB to the host)")
print(f"   i16+flac: {np.median(host['i16+flac']):8.1f} ms ({nbytes / 1e9:.2f} GB to the host)")
print(f"bytes per sample, config 2: {nbytes / N:.3f} (16-bit PCM: 2)")

d = [synth.synth_utterance(tab, synth.T_128S, s, indexed=True) for s in range(args.distinct)]
with J.Batch(vi, d, pdf_set=pset, pcm_i16=True) as b:
    b.set_flac()
    b.run()
    nb = sum(len(s) for s in b.flac_all())
    ns = sum(b.num_samples(i) for i in range(len(d)))
print(f"bytes per sample, {args.distinct} distinct utterances: {nb / ns:.3f}")

bw = 6.3e12
floor = 2 * N + nbytes + 2 * nbytes  # read the 16-bit slab; write the slots; the compaction reads and writes them
print(f"\nHBM traffic of this design: {floor / 1e9:.2f} GB = {floor / bw * 1e3:.2f} ms at 6.3 TB/s "
      f"(issue's floor, one read of the slab plus the compressed write: {(2 * N + nbytes) / bw * 1e3:.2f} ms)")
