"""Cost of the stems of a mix (jb_batch_set_mix_stems; jb_mix.hip) on BASELINE config 2 (256 copies of a 128 s
utterance) as 128 programmes of two fully overlapped talkers (the second at -6 dB), one stem per talker.

1. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with the mix alone, with the mix and its
   stems, with the stems and their levels, and the same with JB_MIX_FIT.  A stage's own time is its step minus the
   plain step, medians over the rounds, modes alternating within a round (the stage runs last on the vocoder's stream,
   nothing overlaps it).
2. --seam-run (works on the parent commit too, where it runs the baseline alone): the baseline for "what stems cost".
   jb_mix_pcm_batch over PCM the caller holds, given the same stems spelt as single-subset programmes -- the two
   talkers' mixture, and each talker once more as a programme of one member with pad_after up to the programme's
   length, over a copy of the member -- and, where the tree has it, jb_mix_stems_pcm_batch over the members alone.
   Both write the same P + S units; the kernel times of the two come from a `rocprofv3 --kernel-trace` run of this
   mode (stems-as-units should equal the baseline within the runs' spread; a fused pass would have to beat it).
3. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `--trace-run` or `--seam-run`, a
   run of its own): every launch of k_mix's passes, k_mix_peak, k_mix_levels and its fold in launch order with its
   grid, and k_noise_sums on the same samples (white noise at 20 dB over every utterance: the same work with one
   load per term, not two), then the medians per kernel.
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating): the
   step times side by side.
5. With --gate LOG (the output of `pytest tests/test_stems_abi.py -k long_double -s`): the dB gate's measured ratios.
Which form ships: stems as units of k_mix; no fused pass was built, so there is no second form to compare.
tools/stems_cost.sh is the recipe: every GPU step under a timeout of its own, chained with &&.

    python tools/stems_cost.py [--rounds 3] [--out profiles/r32_stems.txt]"""
import argparse
import csv
import glob
import json
import os
import re
import sys

# (JB_COST_ROOT: another checkout to take the library from -- the parent commit's, for the seam baseline)
ROOT = os.environ.get("JB_COST_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "r32_stems.txt"))
ap.add_argument("--trace-run", action="store_true", help="the run to put under rocprofv3 --kernel-trace; writes nothing")
ap.add_argument("--seam-run", action="store_true", help="the seam baseline, to put under rocprofv3 --kernel-trace")
ap.add_argument("--seam-programmes", type=int, default=8)
ap.add_argument("--seam-seconds", type=float, default=32.0)
ap.add_argument("--gate", default=None, help="output of pytest tests/test_stems_abi.py -k long_double -s")
ap.add_argument("--kernels", default=None, help="output directory of the rocprofv3 run of --trace-run")
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


import jbonsai_amd as J  # noqa: E402

if args.seam_run:
    # (no voice, no batch: PCM the caller holds; runs on the parent commit, which has jb_mix_pcm_batch alone)
    P, n = args.seam_programmes, int(args.seam_seconds * 48000)
    rng = np.random.default_rng(0)
    talk = [rng.standard_normal(n) * 3000.0 for _ in range(2 * P)]
    mixreq = [(u // 2, 0, -6.0 * (u % 2), 0, 240, 240) for u in range(2 * P)]
    # the stems spelt as programmes of one member over copies of the members (ids P .. 3 P - 1)
    spelt = mixreq + [(P + u, 0, -6.0 * (u % 2), 0, 240, 240) for u in range(2 * P)]
    # (all baseline calls first, then all stems calls: in the trace the launches of k_mix's sum pass fall into two
    # runs of three, told apart by their order -- both forms launch it with the same grid)
    for _ in range(3):
        J.mix_pcm(talk + [x.copy() for x in talk], spelt)
    for _ in range(3 if hasattr(J, "mix_stems_pcm") else 0):
        J.mix_stems_pcm(talk, mixreq, [u % 2 for u in range(2 * P)])
    sys.exit(0)

from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
hz = vi.sampling_frequency
n = synth.T_128S * vi.fperiod  # samples of one member
fade = J.join_ms_to_samples(5.0, hz)
FULL = [(u // 2, 0, -6.0 * (u % 2), 0, fade, fade) for u in range(args.copies)]
STEMS = [u % 2 for u in range(args.copies)]
MODES = {
    "plain": lambda b: None,
    "mix": lambda b: b.set_mix(FULL),
    "mix + stems": lambda b: (b.set_mix(FULL), b.set_mix_stems(STEMS)),
    "mix + stems + levels": lambda b: (b.set_mix(FULL), b.set_mix_stems(STEMS, levels=True)),
    "mix, fit": lambda b: b.set_mix(FULL, fit=True, ceiling_db=-12.0),
    "mix + stems, fit": lambda b: (b.set_mix(FULL, fit=True, ceiling_db=-12.0), b.set_mix_stems(STEMS)),
}

if args.trace_run:
    for name in ("mix", "mix + stems + levels", "mix + stems, fit"):
        with J.Batch(vi, utts, pdf_set=pset) as b:
            MODES[name](b)
            for _ in range(2):
                b.run_timed()
    with J.Batch(vi, utts, pdf_set=pset) as b:
        b.set_noise(J.noise(snr_db=20.0, seed=1))  # (no bed: white noise)
        for _ in range(2):
            b.run_timed()
    sys.exit(0)

say(f"config 2 as {args.copies // 2} programmes of two fully overlapped talkers of {n} samples at {hz} Hz, f64; "
    f"device ms per step, medians of {args.rounds} rounds, modes alternating")
times = {k: [] for k in MODES}
for rnd in range(args.rounds):
    for name, setup in MODES.items():  # (one batch at a time: config 2 fills most of the card)
        with J.Batch(vi, utts, pdf_set=pset) as b:
            setup(b)
            b.run_timed()  # allocations, first launches
            times[name].append(b.run_timed()[0])
        say(f"  round {rnd} {name:>24}: device step {times[name][-1]:8.2f} ms")
med = {k: float(np.median(v)) for k, v in times.items()}
for k, v in times.items():
    say(f"  {k:34s} {med[k]:9.3f} ms   (max - min {max(v) - min(v):.3f})   stage {med[k] - med['plain']:8.3f} ms")
say(f"  stems cost, by difference: {med['mix + stems'] - med['mix']:.3f} ms; the levels {med['mix + stems + levels'] - med['mix + stems']:.3f} ms")
say(f"  with the fit: stems {med['mix + stems, fit'] - med['mix, fit']:.3f} ms")

say("the form that ships: stems as units of k_mix (spans of their own, the fit pass under the parent's scale); no fused "
    "pass was built, so there is no second form to compare")

if args.kernels:
    # one report per trace directory: the parent's seam run, this tree's (the baseline's three calls first, then the
    # stems' three), and the batch run
    traces = {}
    for path in sorted(glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)):
        traces.setdefault(os.path.relpath(path, args.kernels).split(os.sep)[0], []).append(path)
    for trace, paths in traces.items():
        rows, launches = {}, []
        for path in paths:
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    name = r["Kernel_Name"]
                    if not any(k in name for k in ("k_mix", "k_noise_sums")):
                        continue
                    # (the kernel with its template arguments, without namespaces and the argument list)
                    m = re.search(r"k_[A-Za-z0-9_]+(<[^>]*>)?", name)
                    key = m.group(0) if m else name
                    t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                    rows.setdefault(key, []).append(t)
                    launches.append((int(r["Start_Timestamp"]), key, r.get("Grid_Size", "?"), t))
        say(f"trace {trace}: every launch under rocprofv3 --kernel-trace, in order (kernel, grid, ms)")
        for _, key, grid, t in sorted(launches):
            say(f"  {key:60s} {grid:>12s} {t:8.3f}")
        say(f"trace {trace}: per kernel (ms per launch: median, min, max, launches)")
        for key in sorted(rows):
            v = rows[key]
            say(f"  {key:60s} {np.median(v):8.3f} {min(v):8.3f} {max(v):8.3f} {len(v):4d}")
        if trace.startswith("seam"):
            # the sum pass alone (the first k_mix<double, false> of every call): baseline calls, then stems calls
            sums = [t for _, key, _, t in sorted(launches) if re.match(r"k_mix<\w+, false", key)]
            if len(sums) == 6:
                say(f"  sum pass, stems spelt as programmes (jb_mix_pcm_batch):   {np.median(sums[:3]):8.3f} ms "
                    f"(max - min {max(sums[:3]) - min(sums[:3]):.3f})")
                say(f"  sum pass, stems as units (jb_mix_stems_pcm_batch):        {np.median(sums[3:]):8.3f} ms "
                    f"(max - min {max(sums[3:]) - min(sums[3:]):.3f})")
            elif len(sums) == 3:
                say(f"  sum pass, stems spelt as programmes (jb_mix_pcm_batch):   {np.median(sums):8.3f} ms "
                    f"(max - min {max(sums) - min(sums):.3f})")

if args.gate:
    say("the dB gate of tests/test_stems_abi.py (8 times the sequential float64 evaluation's error): measured")
    for ln in open(args.gate):
        if "stems dB gate" in ln:
            say("  " + ln.strip())

for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
    if path:
        vals = [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]
        say(f"bench.py default step, {label}: " + ", ".join(str(v.get("ms_per_step", v)) for v in vals))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
