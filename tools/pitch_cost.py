"""Cost of the pitch stage (jb_batch_set_pitch; jb_pitch.hip) on BASELINE config 2 (256 copies of a 128 s utterance).

1. Device time per step (jb_batch_run_timed) of the same batch plain, with the pitch stage at 25 / 10 ms at the voice's
   48 kHz beside k_fbank on the same frames, and behind the converter at 16 kHz; a stage's own time is its step minus
   the plain step at the same rate, medians over the rounds (the stage runs last on the vocoder's stream, nothing
   overlaps it).  The tracker is serial in a unit's frames, so nearly all of it is k_pitch_track; a kernel trace
   (rocprofv3 --kernel-trace --stats -- python tools/pitch_cost.py --rounds 1) splits it by kernel.
2. Bytes per sample of the output, and the scratch bytes (2 S per frame of choices, 28 per frame of lags, p and pi,
   8 per 4 kHz sample).
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, taken in
   alternation; several lines per file: the repeats): the default step side by side.

    python tools/pitch_cost.py [--rounds 3] [--copies 256] [--out profiles/r33_pitch.txt]   (appends to --out)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_pitch.txt"))
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
o = J.kaldi_pitch()
S = J.pitch_geometry(o, 48000, 0).S

# name -> (output rate, the sink, its request)
MODES = {
    "f64 plain": (0, None, None),
    "pitch 25 / 10 ms": (0, "pitch", o),
    "fbank 25 / 10 ms (2048)": (0, "fbank", J.fbank()),
    "f64 plain at 16 kHz": (16000, None, None),
    "pitch 25 / 10 ms at 16 kHz": (16000, "pitch", o),
}
dev = {k: [] for k in MODES}
bps, frames, n4 = {}, {}, {}
say(f"== config 2 ({args.copies} x 128 s): device step, {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (hz, sink, opts) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if hz:
                b.set_output_rate(hz)
            if sink:
                getattr(b, "set_" + sink)(opts)
                n = [b.num_samples(i) for i in range(len(b))]
                bps[name] = sum(getattr(b, sink + "_size")(i) for i in range(len(b))) / max(1, sum(n))
                frames[name] = sum(getattr(b, sink + "_shape")(i)[0] for i in range(len(b)))
                n4[name] = sum(-(-k * 4000 // (hz or 48000)) for k in n)
            b.run_timed()  # allocations, first launches
            dev[name].append(b.run_timed()[0])
        say(f"  round {rnd} {name:>28}: device step {dev[name][-1]:9.2f} ms")
say()
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    say(f"  {name:>28}: median {med[name]:9.2f} ms ({min(dev[name]):.2f} .. {max(dev[name]):.2f})")
say()
say("the stage's own device time = its step minus the plain step at the same rate (medians):")
for name, (hz, sink, _) in MODES.items():
    if sink:
        own = med[name] - med["f64 plain at 16 kHz" if hz else "f64 plain"]
        extra = ""
        if sink == "pitch":
            scratch = frames[name] * (2 * S + 28) + n4[name] * 8
            extra = f"; scratch {scratch / 1e9:.2f} GB ({2 * S} bytes of choices a frame)"
        say(f"  {name:>28}: {own:9.2f} ms for {frames[name]} frames ({own * 1e3 / max(1, frames[name]):.3f} us a frame of "
            f"the batch), {bps[name]:.4f} bytes per sample{extra}")

if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating runs ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in (json.loads(ln) for ln in open(path) if ln.strip().startswith("{")):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write("\n" + "\n".join(lines) + "\n")
print(f"appended to {args.out}")
