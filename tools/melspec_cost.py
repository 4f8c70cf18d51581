"""Cost of the mel spectrogram stage (jb_batch_set_melspec; jb_melspec.hip) on BASELINE config 2 (256 copies of a
128 s utterance), in one go.

1. Device time per step (jb_batch_run_timed) of the same batch plain, with k_melspec at N = 1200, H = 480 at the voice's
   48 kHz beside k_fbank's 2048-point pass on the same frames (25 / 10 ms), and with Whisper's front end behind the
   converter at 16 kHz; a stage's own time is its step minus the plain step at the same rate, medians over the rounds
   (the stage runs last on the vocoder's stream, nothing overlaps it).
2. The serial host-visible step -- run, sync, read everything into buffers whose pages are already touched -- for the
   features against the f64 read; modes alternate within a round.  The feature read is one pageable copy.
3. Bytes per sample achieved.
4. The precision gate of tests/melspec_ref.py on the device seam at its ten shapes: e(model_f64), e(device), the ratio.
5. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, taken in
   alternation; several lines per file: the repeats): the default step side by side.

    python tools/melspec_cost.py [--rounds 3] [--out profiles/r24_melspec.txt]"""
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
from tests import melspec_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_melspec.txt"))
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

# name -> (output rate, the sink, its request, what is read)
MODES = {
    "f64 plain (f64 read)": (0, None, None, "pcm"),
    "melspec 1200 / 480, log10": (0, "melspec", J.melspec(n_fft=1200, hop=480, log="log10"), "stage"),
    "melspec 1200 / 480, range 8": (0, "melspec", J.melspec(n_fft=1200, hop=480, log="log10", range=8.0), None),
    "fbank 25 / 10 ms (2048)": (0, "fbank", J.fbank(), None),
    "f64 plain at 16 kHz": (16000, None, None, None),
    "whisper at 16 kHz": (16000, "melspec", J.whisper_mel(80), "stage"),
    "fbank 25 / 10 ms at 16 kHz": (16000, "fbank", J.fbank(), None),
}
host = {k: [] for k in MODES}
dev = {k: [] for k in MODES}
gb, bps, frames = {}, {}, {}
say(f"== config 2 ({args.copies} x 128 s), 80 filters: device step and host-visible step (run + sync + one pageable "
    f"read of everything), {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (hz, sink, opts, read) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if hz:
                b.set_output_rate(hz)
            if sink:
                getattr(b, "set_" + sink)(opts)
            n = [b.num_samples(i) for i in range(len(b))]
            bufs = None
            if sink:
                nb = [getattr(b, sink + "_size")(i) for i in range(len(b))]
                bps[name] = sum(nb) / max(1, sum(n))
                frames[name] = sum(getattr(b, sink + "_shape")(i)[0] for i in range(len(b)))
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
                    J._ffi.check(getattr(L, f"jb_batch_read_{sink}_all")(b._h, ptrs))
                else:
                    b.pcm_all(out=bufs)
                host[name].append((time.perf_counter() - t0) * 1e3)
            del bufs
        hv = f", host-visible step {host[name][-1]:8.1f} ms" if host[name] else ""
        say(f"  round {rnd} {name:>28}: device step {dev[name][-1]:8.2f} ms{hv}")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d, h = dev[name], host[name]
    hv = f"; host-visible {np.median(h):8.1f} ms ({min(h):.1f} .. {max(h):.1f}), {gb[name]:.2f} GB to the host" if h else ""
    say(f"  {name:>28}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}){hv}")
say()
say("the stage's own device time = its step minus the plain step at the same rate (medians):")
for name, (hz, sink, _, _) in MODES.items():
    if sink:
        own = med[name] - med["f64 plain at 16 kHz" if hz else "f64 plain (f64 read)"]
        say(f"  {name:>28}: {own:8.2f} ms for {frames[name]} frames ({own * 1e6 / max(1, frames[name]):.1f} ns a frame), "
            f"{bps[name]:.4f} bytes per sample")
for name in ("melspec 1200 / 480, log10", "whisper at 16 kHz"):
    say(f"run + read, {name} against the f64 samples at the voice's rate: {np.median(host[name]):.1f} / "
        f"{np.median(host['f64 plain (f64 read)']):.1f} ms")

say()
say("== the precision gate (tests/melspec_ref.py) on the device seam: e = max |E - E_ld| / (wmax sum_k S_ld), reflect "
    "padding, power ==")
for shape in R.SHAPES:
    x, E_ld, total, wmax, e64 = R.gate_case(shape)
    e = R.rel_err(J.melspec_pcm(x, shape[0], R.opts_of(shape, log="none", f64=True)), E_ld, total, wmax)
    say(f"  {shape}: e(model_f64) {e64:.2e}, e(device) {e:.2e}, ratio {e / e64:.2f} (gate: {R.GATE:.0f})")


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
