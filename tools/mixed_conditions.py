"""Cost of per-utterance vocoder conditions on the headline shape (BASELINE config 2: 256 x 25,546 frames, the
lane kernel at two waves per SIMD): the same batch with K = 1, 4, 16, 256 condition classes -- alpha and volume
differ between classes, utterance i in class i % K -- and one mixed-beta case (one class of alpha / volume, the
post-filter on every other utterance, against the same batch with it on every utterance).  K = 1 is jb_batch_create
itself (no per-utterance table: today's path); the others go through jb_batch_create_voc, whose lane-kernel launch
permutation pads every class to whole waves (21 chunks).  Median ms per step of jb_batch_run_timed (step, vocoder
kernel), alternating the cases round by round.

    python tools/mixed_conditions.py [--rounds 3] [--steps 6]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--batch", type=int, default=256)
args = ap.parse_args()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
utt = synth.synth_utterance(tab, synth.T_128S, 0)
utts = [utt] * args.batch
PER_WAVE = 21


def classes(k):
    return [(0.30 + 0.25 * (i % k) / max(1, k - 1), 0.0, 0.5 + (i % k) / max(1, k - 1)) for i in range(args.batch)]


cases = [("K=1 (jb_batch_create)", None), ("K=4", classes(4)), ("K=16", classes(16)), ("K=256", classes(256)),
         ("beta 0.4 on all (jb_batch_create)", "beta_all"),
         ("beta 0.4 on every other", [(vi.alpha, 0.4 if i % 2 else 0.0, vi.volume) for i in range(args.batch)])]


def make(name, voc):
    if voc == "beta_all":
        v2 = J.VoiceInfo(vi.sampling_frequency, vi.fperiod, vi.alpha, vi.streams, volume=vi.volume, beta=0.4)
        return J.Batch(v2, utts)
    return J.Batch(vi, utts, voc=voc)


# (one batch at a time: a config-2 batch holds 12.5 GB of PCM alone)
ms = {name: [] for name, _ in cases}
info0 = kinfo0 = None
for _ in range(args.rounds):
    for name, voc in cases:
        with make(name, voc) as b:
            for _ in range(2):
                b.run_timed()
            for _ in range(args.steps):
                ms[name].append(b.run_timed())
            if voc is None:
                info0, kinfo0 = b.info(), b.kernel_info()
kname, waves = kinfo0
items = info0["n_items"]
per_utt = items // args.batch
print(f"config 2 shape: {args.batch} x {synth.T_128S} frames, {kname} at {waves} waves per SIMD, "
      f"{items} chunks of {info0['chunk_frames']} frames ({per_utt} per utterance); "
      f"{args.rounds} rounds x {args.steps} steps per case, alternating")
base = np.median([t for t, _ in ms[cases[0][0]]])
for name, voc in cases:
    t = np.array(ms[name])
    step, voc_ms = np.median(t[:, 0]), np.median(t[:, 1])
    spread = (t[:, 0].max() - t[:, 0].min())
    if isinstance(voc, list):
        k = len(set((a, v) for a, _, v in voc))
        per_class = [sum(1 for i in range(args.batch) if i % k == c) * per_utt for c in range(k)]
        pad = sum(-n % PER_WAVE for n in per_class) if k > 1 else 0
    else:
        pad = 0
    print(f"{name:36s} step {step:7.2f} ms (min {t[:, 0].min():6.2f}, spread {spread:5.2f})  vocoder {voc_ms:6.2f} ms  "
          f"padding slots {pad:5d} ({100.0 * pad / items:4.2f} % of the chunks)  vs K=1 {100.0 * (step / base - 1):+5.2f} %")
