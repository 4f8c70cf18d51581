"""Cost of the IMA ADPCM stage (jb_batch_set_adpcm; jb_adpcm.hip) on BASELINE config 2 (256 copies of a 128 s
utterance), in one go.

1. Device time per step (jb_batch_run_timed) of the same batch plain, with k_adpcm (f64 and 16-bit source) and with
   k_format<S16> / k_format<ULAW>; a stage's own time is its step minus the plain step of the same source, medians
   over the rounds (the stages run last on the vocoder's stream, nothing overlaps them).
2. The serial host-visible step -- run, sync, read everything into buffers whose pages are already touched -- for
   ADPCM at 48 kHz against the 16-bit read, and at 8 kHz against mu-law; modes alternate within a round.  Every read
   here is one pageable copy of the slab's used bytes.
3. Bytes per sample achieved.
4. The is_bonsai sentence at 48, 16 and 8 kHz: SNR of decode(encode) with the block-local start index against the
   carried-index encoder of tests/adpcm_ref.py (recorded, not a gate).
5. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree; several lines per
   file: the repeats): the step times side by side.

    python tools/adpcm_cost.py [--rounds 3] [--out profiles/r14_adpcm.txt]"""
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
from tests import adpcm_ref as R  # noqa: E402
from tests.conftest import VOICE  # noqa: E402
from tests.golden.labels import SAMPLE_SENTENCE_2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_adpcm.txt"))
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

# name -> (16-bit sink, output rate, stage, what is read); stage: None, "adpcm" or a sample format
MODES = {
    "f64 plain": (False, 0, None, None),
    "i16 plain (16-bit read)": (True, 0, None, "pcm"),
    "adpcm from f64": (False, 0, "adpcm", "stage"),
    "adpcm from i16": (True, 0, "adpcm", "stage"),
    "k_format s16": (False, 0, "s16", None),
    "k_format ulaw": (False, 0, "ulaw", None),
    "ulaw at 8 kHz": (False, 8000, "ulaw", "stage"),
    "adpcm at 8 kHz from i16": (True, 8000, "adpcm", "stage"),
    "i16 plain at 8 kHz": (True, 8000, None, None),
    "f64 plain at 8 kHz": (False, 8000, None, None),
}
host = {k: [] for k in MODES}
dev = {k: [] for k in MODES}
gb, bps = {}, {}
say(f"== config 2 ({args.copies} x 128 s): device step and host-visible step (run + sync + one pageable read of "
    f"everything), {args.rounds} rounds, modes alternating ==")
for rnd in range(args.rounds):
    for name, (i16, hz, stage, read) in MODES.items():
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=i16) as b:
            if hz:
                b.set_output_rate(hz)
            if stage == "adpcm":
                b.set_adpcm()
            elif stage:
                b.set_format(stage)
            n = [b.num_samples(i) for i in range(len(b))]
            bufs = None
            if read == "stage":
                nb = [b.adpcm_size(i) for i in range(len(b))] if stage == "adpcm" else \
                    [k * L.jb_format_bytes_per_sample(J._ffi.FORMATS[stage]) for k in n]
                bufs = [np.zeros(max(1, k), dtype=np.uint8) for k in nb]
                bps[name] = sum(nb) / max(1, sum(n))
            elif read == "pcm":
                bufs = [np.zeros(k, dtype=np.int16 if i16 else np.float64) for k in n]
            if bufs is not None:
                gb[name] = sum(x.nbytes for x in bufs) / 1e9
                ptrs = (C.c_void_p * len(bufs))(*[x.ctypes.data for x in bufs])
            b.run_timed()  # untimed by the clock below: allocations, first launches
            dev[name].append(b.run_timed()[0])
            if bufs is not None:
                t0 = time.perf_counter()
                b.run()
                b.sync()
                if read == "stage" and stage == "adpcm":
                    J._ffi.check(L.jb_batch_read_adpcm_all(b._h, ptrs))
                elif read == "stage":
                    J._ffi.check(L.jb_batch_read_formatted_all(b._h, ptrs))
                else:
                    b.pcm_all(out=bufs)
                host[name].append((time.perf_counter() - t0) * 1e3)
            del bufs
        hv = f", host-visible step {host[name][-1]:8.1f} ms" if host[name] else ""
        say(f"  round {rnd} {name:>24}: device step {dev[name][-1]:8.2f} ms{hv}")
say()
say("median over rounds (min .. max):")
med = {k: float(np.median(v)) for k, v in dev.items()}
for name in MODES:
    d, h = dev[name], host[name]
    hv = f"; host-visible {np.median(h):8.1f} ms ({min(h):.1f} .. {max(h):.1f}), {gb[name]:.2f} GB to the host" if h else ""
    say(f"  {name:>24}: device step {med[name]:8.2f} ms ({min(d):.2f} .. {max(d):.2f}){hv}")
say()
say("a stage's own device time = its step minus the plain step of the same source and rate (medians):")
own = {
    "k_adpcm<f64>": med["adpcm from f64"] - med["f64 plain"],
    "k_adpcm<i16>": med["adpcm from i16"] - med["i16 plain (16-bit read)"],
    "k_format<S16>": med["k_format s16"] - med["f64 plain"],
    "k_format<ULAW>": med["k_format ulaw"] - med["f64 plain"],
    "k_format<ULAW> at 8 kHz": med["ulaw at 8 kHz"] - med["f64 plain at 8 kHz"],
    "k_adpcm<i16> at 8 kHz": med["adpcm at 8 kHz from i16"] - med["i16 plain at 8 kHz"],
}
for k, v in own.items():
    say(f"  {k:>24}: {v:8.2f} ms")
if own["k_format<S16>"] > 0:
    say(f"k_adpcm<f64> / k_format<S16> = {own['k_adpcm<f64>'] / own['k_format<S16>']:.2f}; "
        f"k_adpcm<i16> / k_format<S16> = {own['k_adpcm<i16>'] / own['k_format<S16>']:.2f}")
say()
say("bytes per sample: " + ", ".join(f"{k}: {v:.4f}" for k, v in bps.items()))
for a, b_ in (("adpcm from i16", "i16 plain (16-bit read)"), ("adpcm at 8 kHz from i16", "ulaw at 8 kHz")):
    say(f"run + read, {a} against {b_}: {np.median(host[a]):.1f} / {np.median(host[b_]):.1f} ms")

say()
say("== the is_bonsai sentence (nitech voice): SNR of decode(encode), block-local against carried start index ==")
for hz in (48000, 16000, 8000):
    e = eng.clone()
    if hz != e.condition.get_sampling_frequency():
        e.condition.set_output_sampling_frequency(hz)
    s = e.synthesize_adpcm(SAMPLE_SENTENCE_2)
    x = np.trunc(np.clip(e.synthesize(SAMPLE_SENTENCE_2), -32768, 32767))
    assert s.data == J.adpcm_encode_host(x, hz)
    carried = J.adpcm_decode_host(R.encode(x, hz, carry=True), s.block_align, x.size)
    say(f"  {hz:>6} Hz, A = {s.block_align:>4}, {x.size} samples, {len(s.data) / x.size:.4f} bytes per sample: "
        f"block-local {R.snr_db(x, s.decode()):.2f} dB, carried {R.snr_db(x, carried):.2f} dB")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (config 2, default, no request), parent commit against this tree, same session ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
