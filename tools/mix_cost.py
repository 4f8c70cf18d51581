"""Cost of the mix stage (jb_batch_set_mix; jb_mix.hip) on BASELINE config 2 (256 copies of a 128 s utterance).

1. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with a join (16 programmes of 16 members,
   500 ms pads, 5 ms fades), with the mix of the same geometry (the join's starts at 0 dB: the same bytes), with 128
   two-talker programmes at half and at full overlap (the second talker at -6 dB), the full overlap with JB_MIX_FIT (the
   second pass), and with k_format<S16>; a stage's own time is its step minus the plain step, medians over the rounds,
   modes alternating within a round (the stages run last on the vocoder's stream, nothing overlaps them).  The
   two-talker rates count the members read once per cover and the programme written once.
2. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `tools/mix_cost.py
   --trace-run`, a run of its own): the kernel times of the join's kernel, k_mix's sum pass
   (by request) and fit pass, k_mix_peak and k_format.
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating): the
   step times side by side.

    python tools/mix_cost.py [--rounds 3] [--out profiles/r29_mix.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_mix.txt"))
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
pad, fade = J.join_ms_to_samples(500.0, hz), J.join_ms_to_samples(5.0, hz)
per = args.per_programme
JOIN = [(u // per, pad, pad, fade, fade) for u in range(args.copies)]
# the join's starts: member i of its programme starts i (pad + n + pad) + pad
MIX_AS_JOIN = [(u // per, (u % per) * (2 * pad + n) + pad, 0.0, pad, fade, fade) for u in range(args.copies)]
HALF = [(u // 2, (u % 2) * (n // 2), -6.0 * (u % 2), 0, fade, fade) for u in range(args.copies)]
FULL = [(u // 2, 0, -6.0 * (u % 2), 0, fade, fade) for u in range(args.copies)]

if args.trace_run:
    for req, fit in ((None, False), (MIX_AS_JOIN, False), (HALF, False), (FULL, True)):
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if req is None:
                b.set_join(JOIN)
                b.set_format("s16")
            else:
                b.set_mix(req, fit=fit, ceiling_db=-12.0)
            for _ in range(2):
                b.run_timed()
    sys.exit(0)


def kernel_key(name):
    """The stage kernels of a trace by instantiation: k_join by sample type, k_mix's sum and fit passes by sample type,
    and the others by name"""
    ty = "f64" if "<double" in name else "i16" if "<short" in name else "?"
    if "k_join" in name:
        return f"join kernel <{ty}>"
    if "k_mix_peak" in name:
        return "k_mix_peak"
    if "k_mix" in name:
        return f"k_mix {'fit' if 'true>' in name else 'sum'} <{ty}>"
    return "k_format" if "k_format" in name else None


# name -> (stage, request, fit)
MODES = {
    "f64 plain": (None, None, False),
    "join 16 x 16": ("join", JOIN, False),
    "mix, the join's geometry": ("mix", MIX_AS_JOIN, False),
    "mix 128 x 2, half overlap": ("mix", HALF, False),
    "mix 128 x 2, full overlap": ("mix", FULL, False),
    "mix 128 x 2, full overlap, fit": ("mix", FULL, True),
    "k_format s16": ("s16", None, False),
}
dev = {k: [] for k in MODES}
say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64): device step, {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (stage, req, fit) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if stage == "join":
                b.set_join(req)
            elif stage == "mix":
                b.set_mix(req, fit=fit, ceiling_db=-12.0)  # (speech at full level passes -12 dBFS: the second pass runs)
            elif stage:
                b.set_format(stage)
            b.run_timed()  # allocations, first launches
            dev[name].append(b.run_timed()[0])
            if fit and rnd == 0:
                say(f"  (fit: scale of programme 0 = {b.mix_report(0).scale:.4f})")
        say(f"  round {rnd} {name:>32}: device step {dev[name][-1]:8.2f} ms")
say()
say("median over rounds (min .. max); a stage's own device time = its step minus the plain step:")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d = dev[name]
    say(f"  {name:>32}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}); own "
        f"{med[name] - med['f64 plain']:8.2f} ms")
own = {k: med[k] - med["f64 plain"] for k in MODES}
say()
if own["join 16 x 16"] > 0:
    ratio = own["mix, the join's geometry"] / own["join 16 x 16"]
    say(f"the mix on the join's geometry / the join on the same members: {ratio:.2f} (the same bytes)")
total = args.copies * n
traffic = {
    "mix 128 x 2, half overlap": (total + (args.copies // 2) * (n + n // 2)) * 8,
    "mix 128 x 2, full overlap": (total + (args.copies // 2) * n) * 8,
    "k_format s16": total * (8 + 2),
}
for k, bytes_ in traffic.items():
    if own[k] > 0:
        say(f"  {k}: {bytes_ / 1e9:.2f} GB of its own traffic, {bytes_ / 1e9 / (own[k] * 1e-3):.0f} GB/s")
say(f"the second pass that fit adds: {own['mix 128 x 2, full overlap, fit'] - own['mix 128 x 2, full overlap']:.2f} ms")

if args.kernels:
    say()
    say("== kernel times (rocprofv3 --kernel-trace, a run of its own: the join with k_format<S16>, then the mix "
        "of the join's geometry, half overlap, full overlap with fit; two steps each) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    runs = {}
    for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
        key = kernel_key(r["Kernel_Name"])
        if key:
            runs.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for key in sorted(runs):
        t = runs[key]
        say(f"  {key:>18}: {sum(t) / len(t):8.3f} ms per launch ({len(t)} launches)")
        if key.startswith("k_mix sum") and len(t) == 6:  # (in the order of the trace run, two steps each)
            for i, shape in enumerate(("the join's geometry", "half overlap", "full overlap")):
                say(f"  {'':>18}  {shape:>20}: {sum(t[2 * i:2 * i + 2]) / 2:8.3f} ms per launch")


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
