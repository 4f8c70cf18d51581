"""Cost of the filterbank stage (jb_batch_set_fbank; jb_fbank.hip) on BASELINE config 2 (256 copies of a 128 s
utterance) at 25 / 10 ms and 80 filters, in one go.

1. Device time per step (jb_batch_run_timed) of the same batch plain, with k_fbank (f32 and f64 elements), and behind
   the converter at 16 kHz; the stage's own time is its step minus the plain step at the same rate, medians over the
   rounds (the stage runs last on the vocoder's stream, nothing overlaps it).
2. The serial host-visible step -- run, sync, read everything into buffers whose pages are already touched -- for the
   features against the f64 read; modes alternate within a round.  The feature read is one pageable copy.
3. Bytes per sample achieved.
4. The precision gate of tests/fbank_ref.py on the device seam at its six shapes: e(model_f64), e(device), the ratio.
5. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, taken in
   alternation; several lines per file: the repeats): the default step side by side.

    python tools/fbank_cost.py [--rounds 3] [--out profiles/r20_fbank.txt]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import jbonsai_amd as J  # noqa: E402
from jbonsai_amd import synth  # noqa: E402
from tests import fbank_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_fbank.txt"))
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
L = J.lib()

# name -> (output rate, the request, what is read)
MODES = {
    "f64 plain (f64 read)": (0, None, "pcm"),
    "fbank f32": (0, J.fbank(), "stage"),
    "fbank f64": (0, J.fbank(f64=True), None),
    "fbank f32, centre": (0, J.fbank(center=True), None),
    "f64 plain at 16 kHz": (16000, None, None),
    "fbank f32 at 16 kHz": (16000, J.fbank(), "stage"),
}
host = {k: [] for k in MODES}
dev = {k: [] for k in MODES}
gb, bps, frames = {}, {}, {}
say(f"== config 2 ({args.copies} x 128 s), 25 / 10 ms, 80 filters: device step and host-visible step (run + sync + "
    f"one pageable read of everything), {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (hz, opts, read) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if hz:
                b.set_output_rate(hz)
            if opts is not None:
                b.set_fbank(opts)
            n = [b.num_samples(i) for i in range(len(b))]
            bufs = None
            if opts is not None:
                nb = [b.fbank_size(i) for i in range(len(b))]
                bps[name] = sum(nb) / max(1, sum(n))
                frames[name] = sum(b.fbank_shape(i)[0] for i in range(len(b)))
            if read == "stage":
                bufs = [np.zeros(max(1, k), dtype=np.uint8) for k in nb]
            elif read == "pcm":
                bufs = [np.zeros(k, dtype=np.float64) for k in n]
            if bufs is not None:
                gb[name] = sum(x.nbytes for x in bufs) / 1e9
                ptrs = (C.c_void_p * len(bufs))(*[x.ctypes.data for x in bufs])
            b.run_timed()  # untimed by the clock below: allocations, first launches
            dev[name].append(b.run_timed()[0])
            if bufs is not None:
                t0 = time.perf_counter()
                b.run()
                b.sync()
                if read == "stage":
                    J._ffi.check(L.jb_batch_read_fbank_all(b._h, ptrs))
                else:
                    b.pcm_all(out=bufs)
                host[name].append((time.perf_counter() - t0) * 1e3)
            del bufs
        hv = f", host-visible step {host[name][-1]:8.1f} ms" if host[name] else ""
        say(f"  round {rnd} {name:>22}: device step {dev[name][-1]:8.2f} ms{hv}")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d, h = dev[name], host[name]
    hv = f"; host-visible {np.median(h):8.1f} ms ({min(h):.1f} .. {max(h):.1f}), {gb[name]:.2f} GB to the host" if h else ""
    say(f"  {name:>22}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}){hv}")
say()
say("the stage's own device time = its step minus the plain step at the same rate (medians):")
for name, plain in (("fbank f32", "f64 plain (f64 read)"), ("fbank f64", "f64 plain (f64 read)"),
                    ("fbank f32, centre", "f64 plain (f64 read)"), ("fbank f32 at 16 kHz", "f64 plain at 16 kHz")):
    own = med[name] - med[plain]
    say(f"  {name:>22}: {own:8.2f} ms for {frames[name]} frames ({own * 1e6 / max(1, frames[name]):.1f} ns a frame), "
        f"{bps[name]:.4f} bytes per sample")
say(f"run + read, features against the f64 samples: {np.median(host['fbank f32']):.1f} / "
    f"{np.median(host['f64 plain (f64 read)']):.1f} ms")

say()
say("== the precision gate (tests/fbank_ref.py) on the device seam: e = max |E - E_ld| / sum_k P_ld ==")
for hz, n_mels, n_fft in R.SHAPES:
    x, E_ld, total, e64 = R.gate_case(hz, n_mels, R.HANN, False, n_fft)
    e = R.rel_err(J.fbank_pcm(x, hz, J.fbank(n_mels=n_mels, n_fft=n_fft, linear=True, f64=True)), E_ld, total)
    say(f"  {hz:>6} Hz, n_fft {R.geometry(hz, n_fft=n_fft)[2]:>4}, {n_mels} filters: e(model_f64) {e64:.2e}, e(device) {e:.2e}, "
        f"ratio {e / e64:.2f} (gate: {R.GATE:.0f})")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, alternating runs ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
