"""Cost of the FLAC metadata (jb_batch_set_flac_meta; jb_flac.hip k_flac_md5, k_flac_seektable) on BASELINE config 2
(256 copies of a 128 s utterance, 16-bit), this tree against a built tree of the parent commit, on one box in one
session.  The parent's tree (its package with its own library, and what the package needs of tests/):

    mkdir -p tools/_ab_parent && git archive HEAD~ jbonsai_amd include tests/__init__.py tests/conftest.py \
        tests/golden/voice | tar -x -C tools/_ab_parent && bash tools/_ab_parent/jbonsai_amd/csrc/build.sh

The runs alternate, parent then this tree, --runs times; every run is a process of its own that imports one tree and
measures, each mode in a batch of its own: the device step by HIP events (jb_batch_run_timed: nothing overlaps the
output stages, so a stage's own time is its step minus the step without it) and, for the FLAC modes, the serial
host-visible step (run, sync, jb_batch_read_flac_all into touched buffers), the bytes, and a SHA-256 of all streams.
Modes: the default step (f64, no request), 16-bit FLAC without the new request, and -- this tree only -- FLAC with MD5,
with a SEEKTABLE (--seek-ms), with both.

    python tools/flac_meta_cost.py [--parent-tree tools/_ab_parent] [--runs 4] [--steps 3]
                                   [--out profiles/r15_flac_meta.txt]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--parent-tree", default=os.path.join(ROOT, "tools", "_ab_parent"))
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--copies", type=int, default=256)
ap.add_argument("--seek-ms", type=int, default=1000)
ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the cycles-per-byte line assumes (peak)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_flac_meta.txt"))
ap.add_argument("--child", default=None, help="(internal) measure with the package of this tree, print one JSON line")
ap.add_argument("--new", action="store_true", help="(internal) the tree has the metadata entries")
args = ap.parse_args()


def child():
    sys.path.insert(0, os.path.abspath(args.child))
    import numpy as np

    import jbonsai_amd as J
    from jbonsai_amd import _ffi, synth
    from tests.conftest import VOICE

    assert os.path.abspath(J.__file__).startswith(os.path.abspath(args.child) + os.sep), J.__file__
    eng = J.Engine.load([VOICE])
    tab, vi = synth.VoiceTables(eng), eng.voice_info()
    pset = tab.pdf_set(0)
    utts = [synth.synth_utterance(tab, synth.T_128S, 0, indexed=True)] * args.copies
    modes = [("default", None), ("flac", {})]
    if args.new:
        modes += [("flac+md5", {"md5": True}), ("flac+table", {"seek_interval_ms": args.seek_ms}),
                  ("flac+both", {"md5": True, "seek_interval_ms": args.seek_ms})]
    res = {}
    for name, kw in modes:
        with J.Batch(vi, utts, pdf_set=pset, pcm_i16=kw is not None) as b:
            if kw is not None:
                b.set_flac()
                if kw:
                    b.set_flac_meta(**kw)
            b.run_timed()  # untimed: allocations, first launches
            r = {"step_ms": [b.run_timed()[0] for _ in range(args.steps)]}
            if kw is not None:
                b.run()
                b.sync()
                ns = []
                for i in range(len(b)):
                    n = C.c_size_t()
                    _ffi.check(b._L.jb_batch_flac_size(b._h, i, C.byref(n)))
                    ns.append(n.value)
                bufs = [np.zeros(max(1, n), dtype=np.uint8) for n in ns]
                u8p = C.POINTER(C.c_uint8)
                ptrs = (u8p * len(bufs))(*[x.ctypes.data_as(u8p) for x in bufs])
                t0 = time.perf_counter()
                b.run()
                b.sync()
                _ffi.check(b._L.jb_batch_read_flac_all(b._h, ptrs))
                r["host_ms"] = (time.perf_counter() - t0) * 1e3
                h = hashlib.sha256()
                for x, n in zip(bufs, ns):
                    h.update(x[:n].tobytes())
                r.update(bytes=sum(ns), sha256=h.hexdigest(), samples=sum(b.num_samples(i) for i in range(len(b))),
                         longest=max(b.num_samples(i) for i in range(len(b))))
                if kw.get("md5"):
                    pcm = b.pcm_i16(0)
                    r["md5_ok"] = bytes(bufs[0][26:42]) == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
            res[name] = r
    print("RESULT " + json.dumps(res), flush=True)


if args.child:
    child()
    sys.exit(0)

sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


runs = {"parent": [], "this tree": []}
say(f"== config 2 ({args.copies} x 128 s), parent commit against this tree, {args.runs} alternating runs, each a "
    f"process of its own; {args.steps} timed steps per mode after one untimed ==")
for k in range(args.runs):
    for label, tree in (("parent", args.parent_tree), ("this tree", ROOT)):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(args.steps), "--copies",
               str(args.copies), "--seek-ms", str(args.seek_ms)] + (["--new"] if label == "this tree" else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode or not out:
            say(f"run {k} of {label} failed ({p.returncode}): {p.stderr[-400:]}")
            sys.exit(1)  # nothing more is started on the GPU behind a failed run
        res = json.loads(out[-1][7:])
        runs[label].append(res)
        for name, r in res.items():
            hv = f"; run + read {r['host_ms']:7.1f} ms, {r['bytes']} bytes, sha256 {r['sha256'][:16]}" if "bytes" in r else ""
            say(f"  run {k} {label:>9} {name:>10}: step ms {' '.join(f'{x:.2f}' for x in r['step_ms'])}{hv}")


def steps(label, name):
    return [x for res in runs[label] for x in res[name]["step_ms"]]


def med(label, name, key="step_ms"):
    v = steps(label, name) if key == "step_ms" else [res[name][key] for res in runs[label]]
    return float(np.median(v)), min(v), max(v)


say()
say("median (min .. max) over all runs:")
for label in runs:
    for name in runs[label][0]:
        m, lo, hi = med(label, name)
        hv = ""
        if "host_ms" in runs[label][0][name]:
            hm, hlo, hhi = med(label, name, "host_ms")
            hv = f"; run + read {hm:7.1f} ms ({hlo:.1f} .. {hhi:.1f})"
        say(f"  {label:>9} {name:>10}: device step {m:8.2f} ms ({lo:.2f} .. {hi:.2f}){hv}")
say()
pm, plo, phi = med("parent", "default")
tm, _, _ = med("this tree", "default")
say(f"default step without any request: parent {pm:.2f} ms (its own spread {plo:.2f} .. {phi:.2f}), this tree {tm:.2f} "
    f"ms: {'within' if plo <= tm <= phi else 'OUTSIDE'} the parent's spread")
pm, plo, phi = med("parent", "flac")
tm, _, _ = med("this tree", "flac")
say(f"FLAC without the new request: parent {pm:.2f} ms ({plo:.2f} .. {phi:.2f}), this tree {tm:.2f} ms: "
    f"{'within' if plo <= tm <= phi else 'OUTSIDE'} the parent's spread")
shas = {res["flac"]["sha256"] for label in runs for res in runs[label]}
nbytes = {res["flac"]["bytes"] for label in runs for res in runs[label]}
say(f"FLAC without the new request, bytes: {sorted(nbytes)}; streams {'identical' if len(shas) == 1 else 'DIFFER'} "
    f"between parent and this tree in every run (SHA-256 of all streams)")
t = runs["this tree"]
base = med("this tree", "flac")[0]
for name in ("flac+md5", "flac+table", "flac+both"):
    m = med("this tree", name)[0]
    say(f"{name}: device step {m:.2f} ms = FLAC step of this tree + {m - base:.2f} ms (parent's FLAC step + {m - pm:.2f} ms)")
own = med("this tree", "flac+md5")[0] - base
longest = t[0]["flac+md5"]["longest"]
say(f"k_flac_md5 alone (HIP events: the step with it minus the step without it, the same stream, nothing beside "
    f"it): {own:.2f} ms for {args.copies} chains of {2 * longest} bytes each")
cpb = own * 1e-3 * args.clock_ghz * 1e9 / (2 * longest)
say(f"  = {cpb:.1f} cycles per byte of one chain at {args.clock_ghz} GHz (the issue's estimate: 20-24); "
    f"{cpb * 64:.0f} cycles per 64-byte block")
say(f"digest of utterance 0 against hashlib in every run: {all(res['flac+md5']['md5_ok'] and res['flac+both']['md5_ok'] for res in t)}")
hb, hp = med("this tree", "flac+both", "host_ms")[0], med("this tree", "flac", "host_ms")[0]
say(f"run + read of everything, both requests against plain FLAC: {hb:.1f} / {hp:.1f} ms; "
    f"{t[0]['flac+both']['bytes'] - t[0]['flac']['bytes']} bytes more (the tables; the digest adds none: "
    f"{t[0]['flac+md5']['bytes'] - t[0]['flac']['bytes']})")
say("side stream for k_flac_md5: not tried")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
