"""Cost and accuracy of the room responses (jb_room_rir_batch; jb_room.hip).

1. The device seam's time and pair visits per second (entries_x entries_y K, summed over the call's rooms) for 256
   distinct rooms and for one room, at 16 kHz with K = 8000 and at 48 kHz with K = 24000, rt60 = 0.5 s; the host
   rule's time for one room of the first beside it.  The time is the whole call's (tables, upload, k_room, read-back), the median
   of the rounds after a first call; the launch budget of jb_room.h (2^35 pair visits) beside the rate.
2. Whether device and host taps have the same bits over the shapes of tests/test_gpu_room.py.
3. The Schroeder T30 of the host-rule response for rt60 = 0.3 / 0.6 s beside the requested value (recorded, not
   gated: image-source decay in a shoebox is known to differ from Eyring's figure).
4. With --bench-before / --bench-after (the JSON lines of plain bench.py runs, parent and this tree, alternating):
   the default step times side by side.

    python tools/room_cost.py [--rounds 3] [--out profiles/r25_room.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rooms", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_room.txt"))
ap.add_argument("--no-device", action="store_true", help="skip parts 1 and 2 (no GPU)")
ap.add_argument("--bench-before", default=None, help="JSON lines of bench.py's plain runs on the parent commit")
ap.add_argument("--bench-after", default=None, help="JSON lines of bench.py's plain runs on this tree")
args = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


import jbonsai_amd as J  # noqa: E402

BUDGET = 2 ** 35


def corpus(n, hz, K, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        size = rng.uniform((3.0, 3.0, 2.4), (10.0, 8.0, 4.0))
        src, mic = J.room_vary(seed, i, size, 0.5)
        out.append(J.room(size, src, mic, rt60=0.5, hz=hz, n_taps=K))
    return out


def timed(fn, rounds):
    fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


if not args.no_device:
    say("== jb_room_rir_batch: the call's time (median of %d rounds after a first call) and pair visits per second ==" %
        args.rounds)
    rate, slow = 0.0, float("inf")
    for hz, K in ((16000, 8000), (48000, 24000)):
        rs = corpus(args.rooms, hz, K)
        for name, sel in (("%d rooms" % args.rooms, rs), ("1 room", rs[:1])):
            visits = sum(J.room_geometry(r).pair_visits for r in sel)
            t = timed(lambda: J.room_rir(sel), args.rounds)
            rate = max(rate, visits / t)
            slow = min(slow, visits / t) if len(sel) > 1 else slow
            say(f"  {hz} Hz, K = {K:5d}, {name:>9}: {t * 1e3:9.2f} ms  {visits:.3e} pair visits  {visits / t:.3e} / s")
        if K == 8000:
            t0 = time.perf_counter()
            J.room_host(rs[0])
            say(f"  {hz} Hz, K = {K:5d}, the host rule for 1 room: {(time.perf_counter() - t0) * 1e3:9.2f} ms")
    say(f"  launch budget: 2^35 = {BUDGET:.3e} pair visits: {BUDGET / rate:.2f} s of one launch at the best rate above, {BUDGET / slow:.2f} s at the lowest of the many-room rates")
    say()
    from tests.test_room_abi import rooms, to_room  # noqa: E402
    from tests import room_ref as R  # noqa: E402
    cases = [(name, dict(rm, n_taps=k)) for name, rm in rooms().items() for k in (1, 255, 256, 257, 513)
             if k > R.tables(rm)["direct"]]
    got = J.room_rir([to_room(rm) for _, rm in cases])
    diff = [(name, rm["n_taps"]) for (name, rm), h in zip(cases, got) if h.tobytes() != J.room_host(to_room(rm)).tobytes()]
    say("== device against host taps over the %d test shapes: %s ==" %
        (len(cases), "the same bits everywhere" if not diff else "different bits at %s" % diff))
    say()

say("== Schroeder T30 of the host rule's response (3.2 x 4.1 x 2.5 m, 16 kHz) beside the requested rt60 ==")
for rt60 in (0.3, 0.6):
    K = int(0.8 * rt60 * 16000)  # the decay to -48 dB: the fit ends at -35 dB
    h = J.room_host(J.room((3.2, 4.1, 2.5), (1.1, 1.4, 1.2), (2.5, 3.3, 1.6), rt60=rt60, hz=16000, n_taps=K))
    edc = 10 * np.log10(np.cumsum((h ** 2)[::-1])[::-1] / np.sum(h ** 2))
    k5, k35 = int(np.argmax(edc <= -5.0)), int(np.argmax(edc <= -35.0))
    slope = np.polyfit(np.arange(k5, k35) / 16000.0, edc[k5:k35], 1)[0]
    say(f"  rt60 requested {rt60:.2f} s: T30 {-60.0 / slope:.3f} s (K = {K})")


def bench_steps(path):
    return [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]


if args.bench_before and args.bench_after:
    say()
    say("== bench.py plain run (default, no request), parent commit against this tree, alternating ==")
    for label, path in (("parent", args.bench_before), ("this tree", args.bench_after)):
        for rec in bench_steps(path):
            keep = {k: rec[k] for k in rec if isinstance(rec[k], (int, float)) and ("ms" in k or "spread" in k or "real" in k)}
            say(f"  {label:>9}: {json.dumps(keep)}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
