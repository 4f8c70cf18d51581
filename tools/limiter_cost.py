"""Cost of the limiter stage (jb_batch_set_limiter; jb_limiter.hip) on BASELINE config 2 (256 copies of a 128 s
utterance), and what it buys.

1. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with a loudness target and a ceiling alone
   (the measurement and k_ln_apply), and with the limiter on top (the measurement, k_ln_limit and its fold); a stage's
   own time is its step minus the plain step, medians over the rounds, modes alternating within a round (the stages
   run last on the vocoder's stream, nothing overlaps them).
2. The loudness shortfall under the target on a synthesized utterance: the loudness of the output (measured with
   jb_loudness_pcm_batch) under a -16 LUFS target and a -1 dBFS ceiling without the limiter and with 3, 6 and 12 dB
   of max_reduction_db, beside what the limiter did.
3. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace --output-format csv` run of `tools/limiter_cost.py --trace-run`,
   a run of its own: one f64 batch with the target alone, then one with the limiter): k_ln_limit beside k_ln_apply on
   the same samples.
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating;
   several lines per file: the repeats): the step times side by side, their spread and whether the spreads overlap.
The file holds what this tool prints and nothing else; the kernels' resource report and the reading of the numbers are
in DESIGN.md (section 4) and LABNOTES.md.

    python tools/limiter_cost.py [--rounds 3] [--out profiles/r19_limiter.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_limiter.txt"))
ap.add_argument("--no-steps", action="store_true", help="skip part 1")
ap.add_argument("--no-shortfall", action="store_true", help="skip part 2")
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

TARGET, CEIL = -16.0, -1.0
LIM = J.limiter(max_reduction_db=6.0)

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
hz = vi.sampling_frequency


def request(b, mode):
    if mode != "plain":
        b.set_loudness_target(TARGET, CEIL)
    if mode == "limiter":
        b.set_limiter(LIM)


if args.trace_run:
    for mode in ("target", "limiter"):
        with J.Batch(vi, utts, pdf_set=pset) as b:
            request(b, mode)
            for _ in range(3):
                b.run_timed()
    sys.exit(0)

if not args.no_steps:
    MODES = {"plain": "plain", "target and ceiling (measure + k_ln_apply)": "target",
             "with the limiter (measure + k_ln_limit)": "limiter"}
    dev = {k: [] for k in MODES}
    say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64), target {TARGET} LUFS, ceiling {CEIL} dBFS, limiter 2 ms / "
        f"8 ms / 6 dB: device step, {args.rounds} rounds, modes alternating ==")
    rep = None
    for rnd in range(args.rounds):
        for name, mode in MODES.items():
            with J.Batch(vi, utts, pdf_set=pset) as b:
                request(b, mode)
                b.run_timed()  # allocations, first launches
                dev[name].append(b.run_timed()[0])
                if mode == "limiter":
                    rep = b.limiter_report(0)
            say(f"  round {rnd} {name:>44}: device step {dev[name][-1]:8.2f} ms")
    say()
    say("median over rounds (min .. max):")
    med = {k: float(np.median(v)) for k, v in dev.items()}
    for name in MODES:
        d = dev[name]
        say(f"  {name:>44}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
    say()
    say("a stage's own device time = its step minus the plain step (medians):")
    names = list(MODES)
    for name in names[1:]:
        say(f"  {name:>44}: {med[name] - med['plain']:8.2f} ms")
    say(f"  the limiter against the target alone: {med[names[2]] - med[names[1]]:+.2f} ms per step")
    say(f"  what it did to each copy: {rep}")

if not args.no_shortfall:
    say()
    say(f"== the shortfall under the target: one synthesized utterance (1,500 frames), target {TARGET} LUFS, ceiling "
        f"{CEIL} dBFS; the output's loudness by jb_loudness_pcm_batch ==")
    one = [synth.synth_utterance(tab, 1500, 3)]
    for depth in (None, 3.0, 6.0, 12.0):
        with J.Batch(vi, one) as b:
            b.set_loudness_target(TARGET, CEIL)
            if depth is not None:
                b.set_limiter(J.limiter(max_reduction_db=depth))
            b.run()
            y = b.pcm(0)
            lufs, peak, gain = b.loudness(0)
            rep = b.limiter_report(0) if depth is not None else None
        (out_lufs, out_peak), = J.loudness([y], hz)
        label = "no limiter" if depth is None else f"max_reduction_db {depth:4.1f}"
        say(f"  {label:>22}: measured {lufs:7.2f} LUFS, peak {peak:6.2f} dBFS, static gain {gain:6.2f} dB -> output "
            f"{out_lufs:7.2f} LUFS ({TARGET - out_lufs:5.2f} LU under the target), peak {out_peak:6.2f} dBFS"
            + ("" if rep is None else f"; reduced by at most {rep['max_reduction_db']:.2f} dB, "
               f"{rep['limited_samples']} of {y.size} samples"))

if args.kernels:
    say()
    say("== kernel times (rocprofv3 --kernel-trace, a run of its own: the config-2 f64 batch with the target alone, then "
        "with the limiter; three steps each) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    tot, cnt = {}, {}
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"]
        key = None
        for name in ("k_ln_apply", "k_ln_limit_fold", "k_ln_limit"):
            if name in k:
                key = name
                break
        if key:
            tot[key] = tot.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
            cnt[key] = cnt.get(key, 0) + 1
    for key in sorted(tot):
        say(f"  {key:>20}: {tot[key] / cnt[key]:8.3f} ms per launch ({cnt[key]} launches)")
    if "k_ln_limit" in tot and "k_ln_apply" in tot:
        say(f"  k_ln_limit / k_ln_apply: {tot['k_ln_limit'] / cnt['k_ln_limit'] / (tot['k_ln_apply'] / cnt['k_ln_apply']):.2f}")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating ==")
    span = {}
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        ms = []
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")
            ms.append(rec["ms_per_step"])
        span[label] = (min(ms), max(ms))
    (p0, p1), (t0, t1) = span["parent"], span["this tree"]
    verdict = ("this tree's spread lies inside the parent's" if p0 <= t0 and t1 <= p1
               else "the spreads overlap" if t0 <= p1 and p0 <= t1
               else f"this tree is {'slower' if t0 > p1 else 'faster'}: the spreads are {min(abs(t0 - p1), abs(p0 - t1)):.2f} ms apart")
    say(f"  parent {p0:.2f} .. {p1:.2f} ms, this tree {t0:.2f} .. {t1:.2f} ms: {verdict}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
