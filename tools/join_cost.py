"""Cost of the join stage (jb_batch_set_join; jb_join.hip) on BASELINE config 2 (256 copies of a 128 s utterance).

1. Device time per step (jb_batch_run_timed) of the same batch plain, with a join (16 programmes of 16 members, 500 ms
   pads, 5 ms fades; f64 and 16-bit), with a loudness target (the measurement AND k_ln_apply) and with k_format<S16>;
   a stage's own time is its step minus the plain step of the same source, medians over the rounds, modes alternating
   within a round (the stages run last on the vocoder's stream, nothing overlaps them).
2. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `tools/join_cost.py --trace-run`, a
   run of its own: one f64 batch with a loudness target, the join and k_format<S16>, then one 16-bit batch with the
   join): the kernel times of the join's kernel by sample type, k_ln_apply and k_format on the same samples, and the
   ratio of the join's kernel to k_ln_apply.
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating;
   several lines per file: the repeats): the step times side by side.

    python tools/join_cost.py [--rounds 3] [--out profiles/r17_join.txt]"""
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
ap.add_argument("--per-programme", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_join.txt"))
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
pad, fade = J.join_ms_to_samples(500.0, hz), J.join_ms_to_samples(5.0, hz)
REQ = [(u // args.per_programme, pad, pad, fade, fade) for u in range(args.copies)]

if args.trace_run:
    with J.Batch(vi, utts, pdf_set=pset) as b:
        b.set_loudness_target(-23.0)
        b.set_join(REQ)
        b.set_format("s16")
        for _ in range(3):
            b.run_timed()
    with J.Batch(vi, utts, pdf_set=pset, pcm_i16=True) as b:
        b.set_join(REQ)
        for _ in range(3):
            b.run_timed()
    sys.exit(0)


def kernel_key(name):
    """The kernels this tool compares, in a trace: k_join by sample type, k_ln_apply and k_format by name"""
    if "k_join" in name:
        return f"join kernel <{'f64' if '<double' in name else 'i16'}>"
    for key in ("k_ln_apply", "k_format"):
        if key in name:
            return key
    return None


# name -> (16-bit sink, stage)
MODES = {
    "f64 plain": (False, None),
    "i16 plain": (True, None),
    "join from f64": (False, "join"),
    "join from i16": (True, "join"),
    "loudness (measure + k_ln_apply), f64": (False, "loudness"),
    "k_format s16": (False, "s16"),
}
dev = {k: [] for k in MODES}
say(f"== config 2 ({args.copies} x 128 s at {hz} Hz): device step, {args.rounds} rounds, modes alternating; the join: "
    f"{args.copies // args.per_programme} programmes of {args.per_programme}, pads of {pad} samples, fades of {fade} ==")
for rnd in range(args.rounds):
    for name, (i16, stage) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=i16) as b:
            if stage == "join":
                b.set_join(REQ)
            elif stage == "loudness":
                b.set_loudness_target(-23.0)
            elif stage:
                b.set_format(stage)
            b.run_timed()  # allocations, first launches
            dev[name].append(b.run_timed()[0])
        say(f"  round {rnd} {name:>38}: device step {dev[name][-1]:8.2f} ms")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d = dev[name]
    say(f"  {name:>38}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
say()
say("a stage's own device time = its step minus the plain step of the same source (medians):")
own = {
    "k_join<f64>": med["join from f64"] - med["f64 plain"],
    "k_join<i16>": med["join from i16"] - med["i16 plain"],
    "loudness (measure + k_ln_apply)": med["loudness (measure + k_ln_apply), f64"] - med["f64 plain"],
    "k_format<S16>": med["k_format s16"] - med["f64 plain"],
}
for k, v in own.items():
    say(f"  {k:>32}: {v:8.2f} ms")
samples = args.copies * synth.T_128S * vi.fperiod
say(f"the join reads {samples} samples and writes {samples + 2 * pad * args.copies}: "
    f"{(2 * samples + 2 * pad * args.copies) * 8 / 1e9:.2f} GB in f64, "
    f"{(2 * samples + 2 * pad * args.copies) * 2 / 1e9:.2f} GB in 16 bits")
for k, width in (("k_join<f64>", 8), ("k_join<i16>", 2)):
    if own[k] > 0:
        say(f"  {k}: {(2 * samples + 2 * pad * args.copies) * width / 1e9 / (own[k] * 1e-3):.0f} GB/s of its own traffic")

if args.kernels:
    say()
    say("== kernel times (rocprofv3 --kernel-trace, a run of its own: one f64 batch with a loudness target, the join "
        "and k_format<S16>, then one 16-bit batch with the join; three steps each) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    tot, cnt = {}, {}
    for r in csv.DictReader(open(f)):
        key = kernel_key(r["Kernel_Name"])
        if key:
            tot[key] = tot.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            cnt[key] = cnt.get(key, 0) + 1
    for key in sorted(tot):
        say(f"  {key:>18}: {tot[key] / cnt[key]:8.3f} ms per launch ({cnt[key]} launches)")
    jk = "join kernel <f64>"
    if jk in tot and "k_ln_apply" in tot:
        say(f"join kernel <f64> / k_ln_apply<f64> = {(tot[jk] / cnt[jk]) / (tot['k_ln_apply'] / cnt['k_ln_apply']):.2f}")


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
