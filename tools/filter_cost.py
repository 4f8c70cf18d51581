"""Cost and accuracy of the filter stage (jb_batch_set_filter; jb_filter.hip) on BASELINE config 2 (256 copies of a
128 s utterance).

1. Accuracy: the floor (scipy.signal.sosfilt in f64 against the long-double reference, the largest over the table of
   tests/filter_ref.py), the gate (8 x the floor), the host seam's and the device seam's largest error.
2. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with a one-section high-pass, with four
   sections, and with a loudness target (the measurement AND k_ln_apply); a stage's own time is its step minus the
   plain step, medians over the rounds, modes alternating within a round (the stages run last on the vocoder's
   stream, nothing overlaps them).
3. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `tools/filter_cost.py --trace-run`,
   a run of its own: one f64 batch with a one-section high-pass and a loudness target, then one with four sections):
   the times of k_filter_tiles<NS, false>, k_filter_scan<NS> and k_filter_tiles<NS, true> beside k_ln_apply on the
   same samples.
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating;
   several lines per file: the repeats): the step times side by side and their spread.

    python tools/filter_cost.py [--rounds 3] [--out profiles/r18_filter.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_filter.txt"))
ap.add_argument("--no-accuracy", action="store_true", help="skip part 1")
ap.add_argument("--no-steps", action="store_true", help="skip part 2")
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

ONE = J.highpass(70.0)
FOUR = J.highpass(70.0) + J.peaking(3000.0, 6.0, 2.0) + J.lowshelf(200.0, -6.0) + J.highshelf(8000.0, 4.0)

if not args.trace_run and not args.no_accuracy:
    from tests import filter_ref as R  # noqa: E402

    say("== accuracy: max|y - y_ld| / max|y_ld| against the serial cascade in numpy.longdouble over the library's own "
        f"coefficients; {len(R.filters())} filters x {len(R.LENGTHS)} lengths (tests/filter_ref.py) ==")
    host = R.host_errors()
    pcms, filts, rates, which = [], [], [], []
    for i, (_, f, hz_) in enumerate(R.filters()):
        for n in R.LENGTHS:
            pcms.append(R.signal_at(hz_)[:n])
            filts.append(f)
            rates.append(hz_)
            which.append(i)
    dev_err = [R.error(y, i) for y, i in zip(J.filter_pcm(pcms, filts, rates), which)]
    k = int(np.argmax(dev_err))
    say(f"  floor (sosfilt, f64): {R.floor():.3e}   gate (8 x floor): {R.gate():.3e}")
    say(f"  host seam's largest error:   {max(host.values()):.3e}")
    say(f"  device seam's largest error: {dev_err[k]:.3e} ({R.filters()[which[k]][0]}, {pcms[k].size} samples)")
    say()

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
hz = vi.sampling_frequency

if args.trace_run:
    for f in (ONE, FOUR):
        with J.Batch(vi, utts, pdf_set=pset) as b:
            b.set_filter(f)
            b.set_loudness_target(-23.0)
            for _ in range(3):
                b.run_timed()
    sys.exit(0)

if not args.no_steps:
    MODES = {"plain": None, "high-pass, 1 section": ONE, "4 sections": FOUR,
             "loudness (measure + k_ln_apply)": "loudness"}
    dev = {k: [] for k in MODES}
    say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64): device step, {args.rounds} rounds, modes alternating ==")
    for rnd in range(args.rounds):
        for name, stage in MODES.items():
            with J.Batch(vi, utts, pdf_set=pset) as b:
                if stage == "loudness":
                    b.set_loudness_target(-23.0)
                elif stage is not None:
                    b.set_filter(stage)
                b.run_timed()  # allocations, first launches
                dev[name].append(b.run_timed()[0])
            say(f"  round {rnd} {name:>34}: device step {dev[name][-1]:8.2f} ms")
    say()
    say("median over rounds (min .. max):")
    med = {k: float(np.median(v)) for k, v in dev.items()}
    for name in MODES:
        d = dev[name]
        say(f"  {name:>34}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
    say()
    say("a stage's own device time = its step minus the plain step (medians):")
    samples = args.copies * synth.T_128S * vi.fperiod
    for name in list(MODES)[1:]:
        own = med[name] - med["plain"]
        say(f"  {name:>34}: {own:8.2f} ms")
        if MODES[name] != "loudness" and own > 0:
            say(f"  {'':>34}  {3 * samples * 8 / 1e9:.2f} GB (each sample read twice, written once): "
                f"{3 * samples * 8 / 1e9 / (own * 1e-3):.0f} GB/s")

if args.kernels:
    say()
    say("== kernel times (rocprofv3 --kernel-trace, a run of its own: f64 batches with a loudness target behind a "
        "one-section and a four-section filter; three steps each) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    tot, cnt = {}, {}
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"]
        key = None
        if "k_ln_apply" in k:
            key = "k_ln_apply"
        elif "k_filter" in k:
            key = k[k.index("k_filter"):].split("(")[0]
        if key:
            tot[key] = tot.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            cnt[key] = cnt.get(key, 0) + 1
    for key in sorted(tot):
        say(f"  {key:>48}: {tot[key] / cnt[key]:8.3f} ms per launch ({cnt[key]} launches)")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
