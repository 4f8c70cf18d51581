"""Cost of the noise stage (jb_batch_set_noise; jb_noise.hip) on BASELINE config 2 (256 copies of a 128 s utterance),
four cases: white noise at 15 dB, a 10 s bed at 15 dB, a 7-sample bed, and the active reference (a 10 s bed).

1. The gain: |g_dev / g_host - 1| of the device seam over the shapes of tests/test_gpu_noise.py (the gate: 2^-50).
2. Device time per step (jb_batch_run_timed) of the same f64 batch plain, with each case, with a loudness target and
   with k_format<S16>; a stage's own time is its step minus the plain step, medians over the rounds, modes alternating
   within a round (the stages run last on the vocoder's stream, nothing overlaps them).
3. With --kernels DIR (the output directory of a `rocprofv3 --kernel-trace` run of `tools/noise_cost.py --trace-run`,
   a run of its own: per case one f64 batch with the noise, a loudness target and k_format<S16>, three steps each):
   the device time of k_noise_sums, k_noise_gain and k_noise_apply per case, beside the loudness measurement's
   kernels, k_ln_apply and k_format on the same batch, and the bytes per second of the sums pass (8 bytes per sample
   read) and the apply pass (16 bytes per sample: 8 read, 8 written) against k_format<S16> (10 bytes per sample).
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating;
   several lines per file: the repeats): the default step times side by side and their spread.

    python tools/noise_cost.py [--rounds 3] [--out profiles/r23_noise.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_noise.txt"))
ap.add_argument("--no-gain", action="store_true", help="skip part 1")
ap.add_argument("--no-steps", action="store_true", help="skip part 2")
ap.add_argument("--trace-run", action="store_true", help="the run to put under rocprofv3 --kernel-trace; writes nothing")
ap.add_argument("--kernels", default=None, help="output directory of the rocprofv3 run of --trace-run")
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []
TRACE_STEPS = 3


def say(s=""):
    print(s, flush=True)
    lines.append(s)


import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests import noise_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402


def bed(n, seed=7):
    return np.round(np.random.default_rng(seed + n).standard_normal(n) * 500.0, 2)


def cases(hz):
    return {
        "white, 15 dB": J.noise(None, hz, snr_db=15.0, seed=1, vary=True),
        "10 s bed, 15 dB": J.noise(bed(10 * hz), hz, snr_db=15.0, vary=True),
        "7-sample bed, 15 dB": J.noise(bed(7), hz, snr_db=15.0, offset=3),
        "10 s bed, 15 dB, active (20 dB gate)": J.noise(bed(10 * hz), hz, snr_db=15.0, reference="active", gate_db=20.0,
                                                       vary=True),
    }


if not args.no_gain and not args.trace_run:
    say("== the gain of the device seam against jb_noise_host over the shapes of tests/test_gpu_noise.py ==")
    shapes = R.cases()
    reqs = [J.noise(b, 48000, **kw) for _, b, kw in shapes]
    _, reps = J.noise_pcm([x for x, _, _ in shapes], reqs, 48000)
    worst, mixed, sums = 0.0, 0, True
    for (x, _, _), req, rep in zip(shapes, reqs, reps):
        _, host = J.noise_host(x, req)
        sums = sums and (rep.speech_power, rep.noise_power, rep.active_samples) == \
            (host.speech_power, host.noise_power, host.active_samples)
        if host.gain != 0.0:
            worst = max(worst, abs(rep.gain / host.gain - 1.0))
            mixed += 1
    say(f"  {len(shapes)} shapes, {mixed} of them mixed: A / C, C and Bs / N equal the host's bit for bit: {sums}; "
        f"largest |g_dev / g_host - 1| = {worst:.3e} (gate 2^-50 = {2.0 ** -50:.3e})")
    say()

if not (args.no_steps and not args.trace_run):
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    pset = tab.pdf_set(0)
    utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
    hz = vi.sampling_frequency
    CASES = cases(hz)
    samples = args.copies * synth.T_128S * vi.fperiod

if args.trace_run:
    for req in CASES.values():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            b.set_noise(req)
            b.set_loudness_target(-23.0)
            b.set_format("s16")
            for _ in range(TRACE_STEPS):
                b.run_timed()
    sys.exit(0)

if not args.no_steps:
    MODES = {"plain": None, **CASES, "loudness (measure + k_ln_apply)": "loudness", "k_format<S16>": "s16"}
    dev = {k: [] for k in MODES}
    say(f"== config 2 ({args.copies} x 128 s at {hz} Hz, f64, {samples} samples): device step, {args.rounds} rounds, "
        "modes alternating ==")
    for rnd in range(args.rounds):
        for name, stage in MODES.items():
            with J.Batch(vi, utts, pdf_set=pset) as b:
                if stage == "loudness":
                    b.set_loudness_target(-23.0)
                elif stage == "s16":
                    b.set_format("s16")
                elif stage is not None:
                    b.set_noise(stage)
                b.run_timed()  # allocations, tables, first launches
                dev[name].append(b.run_timed()[0])
            say(f"  round {rnd} {name:>38}: device step {dev[name][-1]:8.2f} ms")
    say()
    say("median over rounds (min .. max):")
    med = {k: float(np.median(v)) for k, v in dev.items()}
    for name in MODES:
        d = dev[name]
        say(f"  {name:>38}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f})")
    say()
    say("a stage's own device time = its step minus the plain step (medians); the noise stage reads x twice and writes "
        "y once, 24 bytes per sample:")
    for name in list(MODES)[1:]:
        own = med[name] - med["plain"]
        extra = f"  {samples * 24 / 1e9 / (own * 1e-3):7.0f} GB/s" if name in CASES and own > 0 else ""
        say(f"  {name:>38}: {own:8.2f} ms{extra}")

if args.kernels:
    say()
    say(f"== kernel times (rocprofv3 --kernel-trace, a run of its own: per case one f64 batch with the noise, a loudness "
        f"target and k_format<S16>, {TRACE_STEPS} steps; ms per launch, the mean over the case's launches) ==")
    f = glob.glob(os.path.join(args.kernels, "**", "*kernel_trace.csv"), recursive=True)[0]
    keys = ("k_noise_sums", "k_noise_gain", "k_noise_apply", "k_ln_tiles", "k_ln_scan", "k_ln_gate", "k_ln_apply",
            "k_format")
    seen = {k: [] for k in keys}
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for key in keys:
            if key in r["Kernel_Name"] and not (key == "k_ln_gate" and "k_ln_gate_group" in r["Kernel_Name"]):
                seen[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    names = list(cases(48000))
    n_samples = samples if not args.no_steps else args.copies * 128 * 48000
    for c, name in enumerate(names):
        say(f"  {name}:")
        t = {}
        for key in keys:
            per = len(seen[key]) // len(names)
            part = seen[key][c * per:(c + 1) * per]
            if part:
                t[key] = float(np.mean(part))
                say(f"    {key:>14}: {t[key]:8.3f} ms ({len(part)} launches)")
        measure = sum(t.get(k, 0.0) for k in ("k_ln_tiles", "k_ln_scan", "k_ln_gate"))
        say(f"    the noise stage: {sum(t.get(k, 0.0) for k in keys[:3]):.3f} ms; the loudness measurement: {measure:.3f} ms; "
            f"k_ln_apply: {t.get('k_ln_apply', 0.0):.3f} ms")
        if all(k in t for k in ("k_noise_sums", "k_noise_apply", "k_format")):
            say(f"    bytes per second: k_noise_sums {n_samples * 8 / 1e9 / (t['k_noise_sums'] * 1e-3):.0f} GB/s (8 B a "
                f"sample), k_noise_apply {n_samples * 16 / 1e9 / (t['k_noise_apply'] * 1e-3):.0f} GB/s (16 B a sample), "
                f"k_format<S16> {n_samples * 10 / 1e9 / (t['k_format'] * 1e-3):.0f} GB/s (10 B a sample)")


if args.kernels:
    say()
    say("what bounds them (from the code and its ISA; no counters were collected):")
    say("  k_noise_apply moves the 16 bytes per sample of k_ln_apply in the same dwordx4 loads and stores and takes its "
        "time with white noise or a short bed; a long bed adds a gathered 8-byte read per sample (the bed stays in L2 / "
        "the Infinity Cache: 8 bytes more per sample through the TA path, not through HBM).")
    say("  k_noise_sums falls short of the streaming kernels' bytes per second: the rule gives lane l the samples "
        "l + 256 j, so a lane's loads are 8 bytes wide (512 bytes per wave instruction, half the widest form), four "
        "in flight per lane, and a workgroup holds only 8 KB of x for three barriers and six lane shifts of the partial "
        "tree: it is bound by that latency per tile and by the generator's 64-bit multiplies (white) or the bed's "
        "gathered loads, not by HBM.  Wider loads need an exchange through LDS in front of the partials.")
    say("  k_noise_gain is one wave per utterance: about 6,000 tile sums each added by one lane out of LDS, 0.1 ms for 256 "
        "utterances side by side; the active reference walks them a second time with two products and a compare each.")


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
