"""Accuracy and cost of the convolution stage (jb_batch_set_fir; jb_fir.hip) on BASELINE config 2 (256 copies of a
128 s utterance).

1. Accuracy of partitioned mode over the shapes of tests/test_gpu_fir.py: e = max|y - y_ld| / (||h||_1 max|x|) of the
   device seam against the long-double sum, beside e_np, the same metric of float64 numpy.fft convolution of the whole
   signal (the yardstick of the gate, 8 e_np) and of the float64 model of the partitioned algorithm (tests/fir_ref.py).
   Direct mode is bit for bit the host rule and has no row.
2. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with K = 64 (direct), K = 4800 and K = 24000
   taps (a 0.1 s and a 0.5 s response at 48 kHz) and with a loudness target; a stage's own time is its step minus the
   plain step, medians over the rounds, modes alternating within a round (the stages run last on the vocoder's stream,
   nothing overlaps them).
3. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating;
   several lines per file: the repeats): the default step times side by side and their spread.

    python tools/fir_cost.py [--rounds 3] [--out profiles/r21_fir.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_fir.txt"))
ap.add_argument("--no-accuracy", action="store_true", help="skip part 1")
ap.add_argument("--no-steps", action="store_true", help="skip part 2")
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests import fir_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402


def signal(n, seed=1):
    return np.round(np.random.default_rng(seed).standard_normal(n) * 6000.0, 3)


def response(k, seed=2):
    return np.random.default_rng(seed + k).standard_normal(k) * np.exp(-np.arange(k) / max(1.0, k / 4.0))


if not args.no_accuracy:
    PART_K = (257, 1024, 1025, 2 * 1024 + 3, 2048, 2049, 2 * 2048 + 3, 5000)
    say("== accuracy of partitioned mode: e = max|y - y_ld| / (||h||_1 max|x|) against the long-double sum; e_np: float64 "
        "numpy.fft.irfft(rfft(x, n) rfft(h, n)) of the whole signal; model: the partitioned algorithm in float64 numpy ==")
    cases = []
    for k in PART_K:
        _, bk, parts = J.fir_geometry(k)
        for n in sorted({1, bk - 1, bk, bk + 1, 3 * bk + 17, k - 1}):
            cases += [(k, n, d, bk, parts) for d in R.delays(k)]
    hs = {k: response(k) for k in PART_K}
    xs = {c[1]: signal(c[1]) for c in cases}
    got = J.fir_pcm([xs[c[1]] for c in cases], [J.fir(hs[c[0]], 48000, c[2]) for c in cases], 48000)
    worst, worst_many = 0.0, 0.0
    for (k, n, d, bk, parts), y in zip(cases, got):
        x, h = xs[n], hs[k]
        y_ld = R.direct_ld(x, h, d)
        e, e_np = R.rel_err(y, y_ld, x, h), R.rel_err(R.fft_whole(x, h, d), y_ld, x, h)
        e_m = R.rel_err(R.model_partitioned(x, h, d, bk, parts), y_ld, x, h)
        say(f"  K {k:5d} (Bk {bk}, P {parts}) N {n:5d} d {d:5d}: device {e:.3e}  e_np {e_np:.3e}  model {e_m:.3e}  "
            f"device / e_np {e / e_np:6.2f}  model / e_np {e_m / e_np:6.2f}")
        worst = max(worst, e / e_np)
        worst_many = max(worst_many, e / e_np) if n > 1 else worst_many
    say(f"  largest device / e_np: {worst:.2f} over all shapes, {worst_many:.2f} over the shapes of more than one sample "
        "(gate: 8; twice the model's ratio where the model alone exceeds 4)")
    say()

if not args.no_steps:
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    pset = tab.pdf_set(0)
    utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
    hz = vi.sampling_frequency
    MODES = {"plain": None, "K = 64 (direct)": 64, "K = 4800 (Bk 2048, P 3)": 4800, "K = 24000 (Bk 2048, P 12)": 24000,
             "loudness (measure + k_ln_apply)": "loudness"}
    dev = {k: [] for k in MODES}
    say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64): device step, {args.rounds} rounds, modes alternating ==")
    for rnd in range(args.rounds):
        for name, stage in MODES.items():
            with J.Batch(vi, utts, pdf_set=pset) as b:
                if stage == "loudness":
                    b.set_loudness_target(-23.0)
                elif stage is not None:
                    b.set_fir(J.fir(response(stage), hz, stage // 100))
                b.run_timed()  # allocations, tables, first launches
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
    for name in list(MODES)[1:]:
        say(f"  {name:>34}: {med[name] - med['plain']:8.2f} ms")


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
