"""Cost of the speech-activity stage (jb_batch_set_activity; jb_activity.hip) on BASELINE config 2 (256 copies of a
128 s utterance), at 25 / 10 ms on the plain filterbank grid.

1. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with the labels without smoothing, with the
   three smoothing steps, and with 128 two-talker mixes and a column per talker; a stage's own time is its step minus
   the step without it, medians over the rounds, modes alternating within a round (the stage runs last on the
   vocoder's stream, nothing overlaps it).  The label bytes against the f64 stem bytes a host detector would read.
2. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `tools/activity_cost.py
   --trace-run`, a run of its own): the times of k_act_energy, k_act_label without and with smoothing, and k_act_unit,
   and k_act_energy against the power sum of the noise stage over the same samples (k_noise_sums, 3.28 to 4.34 ms in
   profiles/r23_noise.txt).
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating): the
   step times side by side, their medians and spreads.

    python tools/activity_cost.py [--rounds 3] [--out profiles/r31_activity.txt]"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_activity.txt"))
ap.add_argument("--trace-run", action="store_true", help="the run to put under rocprofv3 --kernel-trace; writes nothing")
ap.add_argument("--kernels", default=None, help="output directory of the rocprofv3 run of --trace-run")
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
hz = vi.sampling_frequency
n = synth.T_128S * vi.fperiod  # samples of one member
RAW = J.activity(25, 10, gate_db=40)
SMOOTH = J.activity(25, 10, gate_db=40, min_speech=3, min_gap=20, hang_before=2, hang_after=10)
FULL = [(u // 2, 0, -6.0 * (u % 2)) for u in range(args.copies)]  # 128 two-talker programmes at full overlap

if args.trace_run:
    for opts, req in ((RAW, None), (SMOOTH, None), (SMOOTH, FULL)):
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if req:
                b.set_mix(req)
            b.set_activity(opts)
            for _ in range(2):
                b.run_timed()
    sys.exit(0)

# name -> (activity request, mix request, what its own time is counted from)
MODES = {
    "f64 plain": (None, None, None),
    "labels, no smoothing": (RAW, None, "f64 plain"),
    "labels, close + open + hang": (SMOOTH, None, "f64 plain"),
    "mix 128 x 2": (None, FULL, None),
    "mix 128 x 2, labels per talker": (SMOOTH, FULL, "mix 128 x 2"),
}
dev = {k: [] for k in MODES}
shape = {}
say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64), labels at 25 / 10 ms: device step, {args.rounds} rounds, "
    "modes alternating ==")
for rnd in range(args.rounds):
    for name, (opts, req, _) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if req:
                b.set_mix(req)
            if opts is not None:
                b.set_activity(opts)
            b.run_timed()  # allocations, first launches
            dev[name].append(b.run_timed()[0])
            if opts is not None and rnd == 0:
                T, C, _ = b.activity_shape(0)
                shape[name] = (T, C, b.num_outputs())
                rep, unit = b.activity_report(0, 0), b.activity_unit_report(0)
                say(f"  ({name}: {b.num_outputs()} units of [{T}][{C}]; column 0 of unit 0: {rep.active} active frames, "
                    f"{unit.none} / {unit.one} / {unit.many} frames under 0 / 1 / 2+ talkers)")
        say(f"  round {rnd} {name:>32}: device step {dev[name][-1]:8.2f} ms")
say()
say("median over rounds (min .. max); a stage's own device time = its step minus the step without it:")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name, (_, _, base) in MODES.items():
    d = dev[name]
    own = f"; own {med[name] - med[base]:8.2f} ms" if base else ""
    say(f"  {name:>32}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}){own}")
say()
stems = args.copies * n * 8
for name, (T, C, U) in shape.items():
    say(f"  {name}: {T * C * U / 1e6:.2f} MB of labels ({T * U / 1e6:.2f} million frames by {C}) against "
        f"{stems / 1e9:.2f} GB of f64 stems: 1 / {stems / max(T * C * U, 1):.0f}")

if args.kernels:
    say()
    say("== kernel times (rocprofv3 --kernel-trace, a run of its own: no smoothing, smoothing, smoothing over 128 "
        "two-talker mixes; two steps each) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    runs = {}
    for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
        for key in ("k_act_energy", "k_act_label", "k_act_unit"):
            if key in r["Kernel_Name"]:
                runs.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key in sorted(runs):
        t = runs[key]
        say(f"  {key:>14}: {sum(t) / len(t):8.3f} ms per launch ({len(t)} launches)")
        if len(t) == 6:  # (in the order of the trace run, two steps each)
            for i, what in enumerate(("no smoothing", "smoothing", "smoothing, 128 x 2 talkers")):
                say(f"  {'':>14}  {what:>28}: {sum(t[2 * i:2 * i + 2]) / 2:8.3f} ms per launch")
    if "k_act_energy" in runs:
        e = sum(runs["k_act_energy"][:4]) / 4
        say(f"  k_act_energy reads {stems / 1e9:.2f} GB: {stems / 1e9 / (e * 1e-3):.0f} GB/s; against k_noise_sums' power "
            f"sum over the same samples (3.28 .. 4.34 ms, profiles/r23_noise.txt): {e / 4.34:.2f} .. {e / 3.28:.2f}")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating ==")
    meds = {}
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        vals = []
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k
                                                                                   or k == "value")}
            say(f"  {label:>9}: {json.dumps(keep)}")
            if isinstance(rec.get("value"), (int, float)):
                vals.append(rec["value"])
        if vals:
            meds[label] = (float(np.median(vals)), min(vals), max(vals))
            say(f"  {label:>9}: value median {meds[label][0]:.4g} ({meds[label][1]:.4g} .. {meds[label][2]:.4g})")
    if len(meds) == 2:
        a, b_ = meds["parent"], meds["this tree"]
        say(f"  this tree / parent: {b_[0] / a[0]:.4f} (the runs' spread: parent {(a[2] - a[1]) / a[0]:.4f}, "
            f"this tree {(b_[2] - b_[1]) / b_[0]:.4f} of the median)")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
