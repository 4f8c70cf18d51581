"""Cost of the output sample formats (jb_batch_set_format; jb_format.hip) on BASELINE config 2 (256 copies of a 128 s
utterance), in one go.

1. Device time per step of k_format in every format, and of k_ln_apply<int16_t> on the same samples beside it, each
   launch between two HIP events: tools/microbench/format_kernels (built from format_kernels.hip, see its head), run
   as a child process.
2. The serial host-visible step -- run, sync, read everything into buffers whose pages are already touched -- for
   f32, s24 and mu-law at 8 kHz through the format stage, 16-bit through the fused sink, and the f64 read; modes
   alternate within a round.
3. With --bench-before / --bench-after (the JSON lines of two plain bench.py runs, parent and this tree): both step
   times side by side.

    python tools/format_cost.py [--rounds 3] [--out profiles/r12_formats.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_formats.txt"))
ap.add_argument("--bench-before", default=None, help="JSON line of bench.py's plain run on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON line of bench.py's plain run on this tree")
ap.add_argument("--skip-kernels", action="store_true")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


if not args.skip_kernels:
    exe = os.path.join(ROOT, "tools", "microbench", "format_kernels")
    if not os.path.exists(exe):
        sys.exit(f"{exe} is missing: build it first (the command is at the head of format_kernels.hip)")
    say("== device time of the kernels (HIP events; tools/microbench/format_kernels) ==")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    say(r.stdout.rstrip())
    if r.returncode != 0:
        say(f"format_kernels failed ({r.returncode}): {r.stderr.strip()}")
        sys.exit(1)

eng = J.Engine.load([VOICE])
tab, vi = synth.VoiceTables(eng), eng.voice_info()
pset = tab.pdf_set(0)
utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * 256
L = J.lib()

# name -> (16-bit sink, output rate, format); the reads go into buffers touched before the clock starts
MODES = {"f64 read": (False, 0, None), "s16 fused sink": (True, 0, None), "f32 stage": (False, 0, "f32"),
         "s24 stage": (False, 0, "s24"), "ulaw 8 kHz stage": (False, 8000, "ulaw")}
host = {k: [] for k in MODES}
dev = {k: [] for k in MODES}
gb = {}
say()
say(f"== host-visible step on config 2 (run + sync + read everything), {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (i16, hz, fmt) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=i16) as b:
            if hz:
                b.set_output_rate(hz)
            if fmt:
                b.set_format(fmt)
            n = [b.num_samples(i) for i in range(len(b))]
            if fmt:
                nb = L.jb_format_bytes_per_sample(J._ffi.FORMATS[fmt])
                bufs = [np.zeros(max(1, k * nb), dtype=np.uint8) for k in n]
            else:
                bufs = [np.zeros(k, dtype=np.int16 if i16 else np.float64) for k in n]
            gb[name] = sum(x.nbytes for x in bufs) / 1e9
            ptrs = (C.c_void_p * len(bufs))(*[x.ctypes.data for x in bufs])
            b.run_timed()  # untimed by the clock below: allocations, first launches
            dev[name].append(b.run_timed()[0])
            t0 = time.perf_counter()
            b.run()
            b.sync()
            if fmt:
                J._ffi.check(L.jb_batch_read_formatted_all(b._h, ptrs))
            else:
                b.pcm_all(out=bufs)
            host[name].append((time.perf_counter() - t0) * 1e3)
            del bufs
        say(f"  round {rnd} {name:>17}: device step {dev[name][-1]:8.2f} ms, host-visible step {host[name][-1]:8.1f} ms")
say()
say("median over rounds (min .. max):")
for name in MODES:
    h, d = host[name], dev[name]
    say(f"  {name:>17}: host-visible {np.median(h):8.1f} ms ({min(h):.1f} .. {max(h):.1f}), device step "
        f"{np.median(d):7.2f} ms ({min(d):.2f} .. {max(d):.2f}), {gb[name]:.2f} GB to the host")
f64, f32 = float(np.median(host["f64 read"])), float(np.median(host["f32 stage"]))
say(f"f32 through the stage against the f64 read: {f32:.1f} / {f64:.1f} ms = {f32 / f64:.2f}")


def bench_step(path):
    rec = None
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith("{"):
            rec = json.loads(ln)
    return rec


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default), parent commit against this tree ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        rec = bench_step(path)
        keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
        say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
