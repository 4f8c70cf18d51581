"""Cost of loudness groups and the R128 report (jb_batch_set_loudness_groups, jb_batch_set_loudness_report;
jb_loudness.hip: k_ln_gate_group, k_ln_windows, k_ln_range) on BASELINE config 2 (256 copies of a 128 s utterance), from
one process.

1. Device time per step (jb_batch_run_timed: HIP events around the whole step, the output chain on the vocoder's
   stream inside them) of the same batch: plain; with a loudness target (the baseline: without a group or a report
   request the chain launches and allocates exactly what it did before groups existed); with the 256 utterances in
   256, 16 and 1 groups; each with the R128 report on and off.  The variants alternate within a round, so drift hits
   them alike; each timed run follows --warmup untimed runs of its batch, medians over --steps rounds.
2. The added milliseconds of every variant over the baseline, and each kernel alone by difference (the kernels run one
   after the other on the vocoder's stream, nothing overlaps them): k_ln_gate_group = groups minus baseline,
   k_ln_windows + k_ln_range = report minus the same variant without it; the two measure passes and the apply pass
   together = baseline minus plain.
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent commit and this tree; several
   lines per file: the repeats): the plain steps side by side with both spreads.

    python tools/loudness_groups_cost.py [--steps 5] [--warmup 1] [--out profiles/r16_loudness_groups.txt]"""
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
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_loudness_groups.txt"))
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
N = args.copies

# name -> (target, utterances per group or None, report)
MODES = {"plain": (False, None, False), "target (baseline)": (True, None, False), "target + report": (True, None, True)}
for groups in (N, 16, 1):
    if groups <= N:
        MODES[f"{groups} group(s)"] = (True, N // groups, False)
        MODES[f"{groups} group(s) + report"] = (True, N // groups, True)

def make(name):
    target, per, report = MODES[name]
    b = J.Batch(vi, utts, pdf_set=pset)
    if target:
        b.set_loudness_target(-23.0, -1.0)
    if per:
        b.set_loudness_groups([i // per for i in range(N)])
    if report:
        b.set_loudness_report()
    return b


dev = {k: [] for k in MODES}
say(f"== config 2 ({N} x 128 s): device step; {args.steps} rounds, in each a fresh batch per variant (two of them "
    f"would not fit the card side by side), {args.warmup} warm-up run(s) then one timed run, variants alternating ==")
g = None
for step in range(args.steps):
    for name in MODES:
        with make(name) as b:
            for _ in range(args.warmup):
                b.run_timed()  # allocations, first launches
            dev[name].append(b.run_timed()[0])
            if name == "1 group(s) + report" and g is None:
                g = b.loudness_group(0)
        say(f"  round {step} {name:>24}: {dev[name][-1]:8.2f} ms")
say()
say(f"the 1-group variant walks {g['members']} members and {g['r128']['n_windows']} gated windows "
    f"(L_G {g['lufs']:.2f} LUFS, LRA {g['r128']['lra_lu']:.2f} LU)")
say()
say("median over steps (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d = dev[name]
    say(f"  {name:>24}: {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
base = med["target (baseline)"]
say()
say(f"measure passes + apply pass (baseline minus plain): {base - med['plain']:8.2f} ms")
say("added over the baseline, and the kernels alone by difference:")
for name in MODES:
    if name in ("plain", "target (baseline)"):
        continue
    extra = ""
    if name.endswith("+ report"):
        off = name[: -len(" + report")]
        off = "target (baseline)" if off == "target" else off
        extra = f"; k_ln_windows + k_ln_range {med[name] - med[off]:7.2f} ms"
    else:
        extra = f"; k_ln_gate_group {med[name] - base:7.2f} ms"
    say(f"  {name:>24}: {med[name] - base:+8.2f} ms{extra}")
worst = med["1 group(s) + report"] - base
say(f"the 1-group case with the report adds {worst:.2f} ms against {base - med['plain']:.2f} ms of measure and apply passes: "
    + ("MORE than the passes themselves" if worst > base - med["plain"] else "small beside them"))


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, same session ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
