"""Cost of the fast batch-invariant mode (JB_BATCH_INVARIANT) against the default and the serial invariant mode
(JB_BATCH_SERIAL | JB_BATCH_SERIAL_GV), in one process: per shape the three modes alternate round by round, each
step timed on its own (jb_batch_run_timed); the median is reported with the geometry each mode chose (chunk length,
warm-up, work items, kernel and its waves per SIMD) and the chunks the last step redid.  Then the three sentences
of the reference's benches/bonsais.rs through jb_synthesize, per mode (latency, warm, median of the calls).

    python tools/fast_invariant_bench.py [--rounds 3] [--steps 4] [--serial-steps 1] [--only config2,...]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402
from tests.golden.labels import BENCH_LETTER, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--serial-steps", type=int, default=1)
ap.add_argument("--only", default="")
args = ap.parse_args()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)


def distinct(n, T, id0):
    return [synth.synth_utterance(tab, T, id0 + i, indexed=True) for i in range(n)]


def config3_sub():
    # one sub-batch of BASELINE config 3: lengths U[400, 25546], up to 7,000,000 frames
    rng = np.random.default_rng(3)
    lens, tot = [], 0
    while True:
        T = int(rng.integers(400, 25547))
        if tot + T > 7_000_000:
            break
        lens.append(T)
        tot += T
    return [synth.synth_utterance(tab, T, 9000 + i, indexed=True) for i, T in enumerate(lens)]


SHAPES = {
    "config2": lambda: [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256,
    "config4": lambda: distinct(1024, 6386, 2000),
    "64x4": lambda: distinct(64, synth.T_128S, 1000) * 4,
    "64x2000": lambda: distinct(64, 2000, 3000),
    "1024x500": lambda: distinct(1024, 500, 4000),
    "config3_sub": config3_sub,
}
MODES = {"default": dict(), "fast_invariant": dict(fast_invariant=True), "serial": dict(serial=True, serial_gv=True)}

only = set(args.only.split(",")) if args.only else None
print(f"{args.rounds} rounds, {args.steps} timed steps per mode and round ({args.serial_steps} for the serial mode), "
      "after one untimed step; modes alternate within a round; ms = median of individually timed steps")
for shape, mk in SHAPES.items():
    if only and shape not in only:
        continue
    utts = mk()
    frames = sum(int(np.sum(u.durations)) for u in utts)
    ms = {m: [] for m in MODES}
    geo = {}
    for _ in range(args.rounds):
        for m, kw in MODES.items():
            with J.Batch(vi, utts, pdf_set=pset, **kw) as b:
                b.run_timed()
                for _ in range(args.serial_steps if m == "serial" else args.steps):
                    ms[m].append(b.run_timed()[0])
                inf, (kern, waves) = b.info(), b.kernel_info()
                geo[m] = (f"C {inf['chunk_frames']:3d} W {inf['warmup_frames']:2d} items {inf['n_items']:6d} "
                          f"{kern} x{waves} redone {inf['n_redo']}")
    d = np.median(ms["default"])
    print(f"\n{shape}: {len(utts)} utterances, {frames} frames")
    for m in MODES:
        t = np.median(ms[m])
        print(f"  {m:15s} {t:9.2f} ms (min {np.min(ms[m]):9.2f}, n {len(ms[m]):2d})  x{t / d:6.3f} of default"
              f"  {geo[m]}")
    print(f"  serial / fast_invariant: {np.median(ms['serial']) / np.median(ms['fast_invariant']):.1f}x")

print("\nsentences through jb_synthesize (warm; median of 20 calls)")
engines = {}
for m in MODES:
    e = J.Engine.load([VOICE])
    if m == "fast_invariant":
        e.condition.set_fast_invariant(True)
    elif m == "serial":
        e.condition.set_batch_invariant(True)
    engines[m] = e
for name, lab in (("bonsai_8_labels", SAMPLE_SENTENCE_1), ("is_bonsai_20_labels", SAMPLE_SENTENCE_2),
                  ("bonsai_letter_43_labels", BENCH_LETTER)):
    res = {}
    for m, e in engines.items():
        for _ in range(3):
            e.synthesize(lab)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            e.synthesize(lab)
            ts.append(1e3 * (time.perf_counter() - t0))
        res[m] = float(np.median(ts))
    print(f"  {name:24s} " + "  ".join(f"{m} {t:6.2f} ms" for m, t in res.items())
          + f"  fast/default x{res['fast_invariant'] / res['default']:.2f}")
