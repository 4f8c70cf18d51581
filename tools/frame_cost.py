"""Cost of the frame request (jb_batch_set_frame_opts; the conditioned loader of k_fbank, jb_fbank.hip) on BASELINE
config 2 (256 copies of a 128 s utterance) at 25 / 10 ms and 80 filters, in one go.

1. Device time per step (jb_batch_run_timed) of the same batch plain, with the filterbank stage, and with the stage
   under Kaldi's conditioning (Povey window, DC removal, pre-emphasis 0.97), at 48 kHz (n_fft 2048: two waves a frame,
   the mean crosses waves through LDS) and behind the converter at 16 kHz (n_fft 512: a wave a frame).  The stage's own
   time is its step minus the plain step at the same rate, medians over the rounds, modes alternating within a round
   (the stage runs last on the vocoder's stream, nothing overlaps it).  The same for the cepstral stage with the
   frame's log energy as c0.
2. With --gate-log (the output of pytest -s tests/test_gpu_frame.py -m gpu): the precision gate's measured ratios on the
   device seam, e(device) / e(model_f64) against the long double model (tests/frame_ref.py), and the largest of them.
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, taken in
   alternation; several lines per file: the repeats): the default step side by side, medians and range.

    python tools/frame_cost.py [--rounds 3] [--out profiles/r27_frame.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_frame.txt"))
ap.add_argument("--gate-log", default=None, help="the output of pytest -s tests/test_gpu_frame.py: its gate ratios")
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
kaldi = J.frame(preemph=0.97, window="povey", remove_dc=True)
energy = J.frame(preemph=0.97, window="povey", remove_dc=True, energy=True)
mo = J.mfcc(n_ceps=13, delta_order=2, cmvn="mean_var")

# name -> (output rate, fbank request, mfcc request, frame request)
MODES = {
    "plain": (0, None, None, None),
    "fbank": (0, J.fbank(), None, None),
    "fbank, kaldi frames": (0, J.fbank(), None, kaldi),
    "mfcc": (0, J.fbank(), mo, None),
    "mfcc, kaldi frames + energy": (0, J.fbank(), mo, energy),
    "plain at 16 kHz": (16000, None, None, None),
    "fbank at 16 kHz": (16000, J.fbank(), None, None),
    "fbank at 16 kHz, kaldi frames": (16000, J.fbank(), None, kaldi),
}
dev = {k: [] for k in MODES}
frames = {}
say(f"== config 2 ({args.copies} x 128 s), 25 / 10 ms, 80 filters: device step, {args.rounds} rounds, modes "
    f"alternating ==")
for rnd in range(args.rounds):
    for name, (hz, fo, mf, fr) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if hz:
                b.set_output_rate(hz)
            if mf is not None:
                b.set_mfcc(mf, fbank=fo)
                frames[name] = sum(b.mfcc_shape(i)[0] for i in range(len(b)))
            elif fo is not None:
                b.set_fbank(fo)
                frames[name] = sum(b.fbank_shape(i)[0] for i in range(len(b)))
            if fr is not None:
                b.set_frame(fr)
            b.run_timed()  # untimed below: allocations, first launches
            dev[name].append(b.run_timed()[0])
        say(f"  round {rnd} {name:>30}: device step {dev[name][-1]:8.2f} ms")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d = dev[name]
    say(f"  {name:>30}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
say()
say("the stage's own device time = its step minus the plain step at the same rate (medians), with the request against "
    "without it:")
for with_fr, without, plain in (("fbank, kaldi frames", "fbank", "plain"),
                                ("mfcc, kaldi frames + energy", "mfcc", "plain"),
                                ("fbank at 16 kHz, kaldi frames", "fbank at 16 kHz", "plain at 16 kHz")):
    a, b0 = med[with_fr] - med[plain], med[without] - med[plain]
    say(f"  {with_fr:>30}: {a:8.2f} ms against {b0:8.2f} ms for {frames[with_fr]} frames "
        f"({a * 1e6 / max(1, frames[with_fr]):.1f} against {b0 * 1e6 / max(1, frames[without]):.1f} ns a frame), "
        f"ratio {a / b0:.3f}")
say("what bounds the ratio: two more barriers and one more LDS round trip per frame (the samples staged, summed by "
    "one wave, read back with their neighbours).")


if args.gate_log:
    say()
    say("== the precision gate (tests/frame_ref.py) on the device seam: e = max |E - E_ld| / sum_k P_ld, ratio = "
        "e(device) / e(model_f64), gate 8 ==")
    ratios = []
    for ln in open(args.gate_log):
        at = ln.find("device ")
        if at >= 0 and " ratio " in ln:
            say("  " + ln[at:].rstrip())
            ratios.append(float(ln.rsplit(" ratio ", 1)[1].split()[0]))
    if ratios:
        say(f"  {len(ratios)} cases, ratios {min(ratios):.2f} .. {max(ratios):.2f}")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating runs ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        recs = bench_steps(path)
        for rec in recs:
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")
        v = [r["ms_per_step"] for r in recs if "ms_per_step" in r]
        say(f"  {label:>9}: ms_per_step median {np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f}) over {len(v)} runs")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
