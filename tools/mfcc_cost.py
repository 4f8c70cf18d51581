"""Cost of the cepstral stage (jb_batch_set_mfcc; jb_mfcc.hip) on BASELINE config 2 (256 copies of a 128 s utterance)
at 25 / 10 ms, 80 filters, 13 cepstra, order 2, MEAN_VAR, in one go.

1. Device time per step (jb_batch_run_timed) of the same batch plain and with requests that add the stage's kernels one
   group at a time; a group's own time is the difference of two steps, medians over the rounds (the stage runs last on
   the vocoder's stream, nothing overlaps it):
     fbank f64                   - plain               = the stage's own filterbank pass (k_fbank, unchanged)
     mfcc 13, order 0, none      - fbank f64           = k_ceps + k_delta (a conversion of 13 columns)
     mfcc 13, order 2, none      - mfcc order 0        = the delta rows of k_delta
     mfcc 13, order 2, mean_var  - mfcc order 2, none  = the four statistics launches and the division
     log-mel 80, order 2, mean_var                      : n_ceps = 0, the fbank + deltas + CMVN form
   beside each group's compulsory bytes (what it must read and write once) and the rate that gives, as a fraction of
   the rate k_format reaches on the same machine (s16: 8 bytes in, 2 out per sample; its step minus the plain step).
2. The serial host-visible step -- run, sync, read everything into buffers whose pages are already touched -- for the
   rows against the f64 read; modes alternate within a round.  The feature read is one pageable copy.
3. The precision gate of tests/mfcc_ref.py on the device seam: e(model_f64), e(device), the ratio.
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, taken in
   alternation; several lines per file: the repeats): the default step side by side.

    python tools/mfcc_cost.py [--rounds 3] [--out profiles/r22_mfcc.txt]"""
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
from tests import mfcc_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_mfcc.txt"))
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
FB = J.fbank()

# name -> (what is set, what is read)
MODES = {
    "f64 plain (f64 read)": (None, "pcm"),
    "format s16": ("s16", None),
    "fbank f64": (J.fbank(f64=True), None),
    "mfcc 13, order 0, none": (J.mfcc(), None),
    "mfcc 13, order 2, none": (J.mfcc(delta_order=2), None),
    "mfcc 13, order 2, mean_var": (J.mfcc(delta_order=2, cmvn="mean_var"), "stage"),
    "log-mel 80, order 2, mean_var": (J.mfcc(n_ceps=0, delta_order=2, cmvn="mean_var"), None),
}
host = {k: [] for k in MODES}
dev = {k: [] for k in MODES}
gb = {}
frames = samples = 0
say(f"== config 2 ({args.copies} x 128 s), 25 / 10 ms, 80 filters: device step and host-visible step (run + sync + "
    f"one pageable read of everything), {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (req, read) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset) as b:
            if isinstance(req, str):
                b.set_format(req)
            elif isinstance(req, J.FbankOpts):
                b.set_fbank(req)
            elif req is not None:
                b.set_mfcc(req, fbank=FB)
            n = [b.num_samples(i) for i in range(len(b))]
            samples = sum(n)
            bufs = None
            if read == "stage":
                frames = sum(b.mfcc_shape(i)[0] for i in range(len(b)))
                bufs = [np.zeros(max(1, b.mfcc_size(i)), dtype=np.uint8) for i in range(len(b))]
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
                    J._ffi.check(L.jb_batch_read_mfcc_all(b._h, ptrs))
                else:
                    b.pcm_all(out=bufs)
                host[name].append((time.perf_counter() - t0) * 1e3)
            del bufs
        hv = f", host-visible step {host[name][-1]:8.1f} ms" if host[name] else ""
        say(f"  round {rnd} {name:>30}: device step {dev[name][-1]:8.2f} ms{hv}")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d, h = dev[name], host[name]
    hv = f"; host-visible {np.median(h):8.1f} ms ({min(h):.1f} .. {max(h):.1f}), {gb[name]:.2f} GB to the host" if h else ""
    say(f"  {name:>30}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}){hv}")
say()
fmt_ms = med["format s16"] - med["f64 plain (f64 read)"]
fmt_rate = samples * 10 / 1e9 / (fmt_ms * 1e-3)
say(f"k_format (s16): {fmt_ms:.2f} ms for {samples} samples, 10 bytes each: {fmt_rate:.0f} GB/s -- the rate the fractions "
    "below refer to")
say(f"a kernel group's own device time = the difference of two steps (medians), {frames} frames:")
F = frames
GROUPS = (
    ("the stage's filterbank pass (k_fbank, f64)", "fbank f64", "f64 plain (f64 read)", samples * 8 + F * 80 * 8),
    ("k_ceps + k_delta of 13 columns", "mfcc 13, order 0, none", "fbank f64", F * (80 * 8 + 13 * 8) + F * (13 * 8 + 13 * 4)),
    ("the delta rows (order 0 -> 2)", "mfcc 13, order 2, none", "mfcc 13, order 0, none", F * 26 * 4),
    ("the statistics (MEAN_VAR)", "mfcc 13, order 2, mean_var", "mfcc 13, order 2, none", 2 * F * 13 * 8),
    ("the whole stage, 13 cepstra, order 2, MEAN_VAR", "mfcc 13, order 2, mean_var", "f64 plain (f64 read)",
     samples * 8 + F * 80 * 8 * 2 + F * 13 * 8 * 4 + F * 39 * 4),
    ("the whole stage, log-mel 80, order 2, MEAN_VAR", "log-mel 80, order 2, mean_var", "f64 plain (f64 read)",
     samples * 8 + F * 80 * 8 * 4 + F * 240 * 4),
)
for what, a, b_, nbytes in GROUPS:
    own = med[a] - med[b_]
    rate = nbytes / 1e9 / (own * 1e-3) if own > 0 else float("nan")
    say(f"  {what:>48}: {own:8.2f} ms, {nbytes / 1e9:6.3f} GB compulsory, {rate:7.0f} GB/s = {rate / fmt_rate:5.2f} of "
        "k_format's rate")
say(f"run + read, rows against the f64 samples: {np.median(host['mfcc 13, order 2, mean_var']):.1f} / "
    f"{np.median(host['f64 plain (f64 read)']):.1f} ms")

say()
say("== the precision gate (tests/mfcc_ref.py) on the device seam, 300 frames: e = max |X - X_ld| / bound ==")
for n_mels, n_ceps in ((23, 13), (80, 13), (80, 80), (128, 40), (128, 0), (1, 1)):
    Lm = R.logmel(n_mels)
    for cmvn in ("none", "mean", "mean_var"):
        kw = dict(n_ceps=n_ceps, delta_order=2, delta_window=2, cmvn=cmvn)
        e, e64 = R.errors(J.mfcc_frames(Lm, J.mfcc(f64=True, **kw)), Lm, **kw)
        say(f"  {n_mels:>3} filters, {n_ceps:>3} cepstra, order 2, {cmvn:>8}: e(model_f64) {e64:.2e}, e(device) {e:.2e}, "
            f"ratio {e / e64 if e64 else 0:.2f} (gate: {R.GATE:.0f})")


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
