"""Front half of an engine-level request with the tree search on the host threads and on the device
(jb_engine_set_tree_search), in one process on one machine: the front-half time and the wall time the library
reports under JB_E2E_TIMING=1, for

  64 x the genji text (1,456 labels each), jb_synthesize_batch_i16
  256 x 1,400 labels (the config-2 shape), jb_synthesize_batch_i16
  one sentence of 8, 20 and 43 labels, jb_synthesize
  a sweep of single texts and small batches, to place the crossover JB_SEARCH_AUTO uses

Modes alternate within each repeat (host, device, host, ...); five repeats; median and [min .. max] per mode.  The
host-mode lines are the baseline: run on the parent commit (whose library has no device mode, the tool then prints
host lines only) they must agree within the spread printed here.  --quick: two repeats, the large batches smaller.
"""
import os
import re
import statistics
import sys
import tempfile

os.environ["JB_E2E_TIMING"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jbonsai_amd as J  # noqa: E402
from tests.conftest import VOICE  # noqa: E402
from tests.golden.labels import BENCH_LETTER, GENJI, SAMPLE_SENTENCE_1, SAMPLE_SENTENCE_2  # noqa: E402

LINE = re.compile(r"jb_synthesize_batch: (\d+) group\(s\), wall ([\d.]+) ms; front half ([\d.]+) ms")
PHASES = re.compile(r"front half of \d+ utterance\(s\): parse [^\n]*")


def timed(fn):
    """fn() with the library's stderr captured: (groups, wall ms, front-half ms) of its JB_E2E_TIMING line, and the
    device mode's phase lines (one per group)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = LINE.search(text)
    assert m, text
    return int(m.group(1)), float(m.group(2)), float(m.group(3)), PHASES.findall(text)


def spread(xs):
    return f"{statistics.median(xs):9.2f} [{min(xs):8.2f} .. {max(xs):8.2f}]"


def main():
    quick = "--quick" in sys.argv
    reps = 2 if quick else 5
    base = J.Engine.load([VOICE])
    modes = [("host", 0)]
    if hasattr(base.condition, "set_tree_search"):
        modes.append(("device", 2))
    engines = {}
    for name, mode in modes:
        e = base.clone()
        if mode:
            e.condition.set_tree_search(mode)
        engines[name] = e

    def single(labels):
        return lambda e: e.synthesize(labels)

    def batch(utts):
        return lambda e: e.synthesize_batch(utts, i16=True)

    big = 16 if quick else 64
    cfg2 = 32 if quick else 256
    cases = [
        (f"{big} x genji text ({len(GENJI)} labels), batch_i16", big * len(GENJI), batch([GENJI] * big)),
        (f"{cfg2} x 1400 labels, batch_i16", cfg2 * 1400, batch([GENJI[:1400]] * cfg2)),
        ("1 sentence, 8 labels, jb_synthesize", 8, single(SAMPLE_SENTENCE_1)),
        ("1 sentence, 20 labels, jb_synthesize", 20, single(SAMPLE_SENTENCE_2)),
        ("1 sentence, 43 labels, jb_synthesize", 43, single(BENCH_LETTER)),
    ]
    for n in (64, 128, 256, 512, 1024, len(GENJI)):
        cases.append((f"sweep: 1 text, {n} labels, jb_synthesize", n, single(GENJI[:n])))
    for b, n in ((8, 64), (8, 128), (4, 512), (8, 256), (2, len(GENJI)), (16, 512), (16, len(GENJI))):
        cases.append((f"sweep: {b} x {n} labels, batch_i16", b * n, batch([GENJI[:n]] * b)))

    print(f"# tools/front_half.py: {reps} repeats, modes alternating; ms as median [min .. max]; "
          f"JB_HOST_THREADS={os.environ.get('JB_HOST_THREADS', 'default')}")
    print(f"# {'case':52s} {'labels':>7s} {'mode':6s} {'front half':>31s} {'wall':>31s}")
    wins = []  # (labels, device mode wins front half and wall)
    for what, n_labels, fn in cases:
        for e in engines.values():  # warm-up: tables, pools, the noise table
            timed(lambda: fn(e))
        front = {k: [] for k in engines}
        wall = {k: [] for k in engines}
        for _ in range(reps):
            for name, e in engines.items():
                _, w, f, phases = timed(lambda: fn(e))
                front[name].append(f)
                wall[name].append(w)
        for name in engines:
            print(f"  {what:52s} {n_labels:7d} {name:6s} {spread(front[name])} {spread(wall[name])}")
        if "device" in engines:
            fh, fd = statistics.median(front["host"]), statistics.median(front["device"])
            wh, wd = statistics.median(wall["host"]), statistics.median(wall["device"])
            print(f"  {'':52s} {'':7s} {'d/h':6s} {fd / fh:9.2f}x front half {wd / wh:25.2f}x wall")
            wins.append((n_labels, fd < fh and wd < wh))
            for ph in phases:  # of the last device-mode run
                print(f"  {'':52s} {'':7s} {'':6s} {ph}")
        sys.stdout.flush()
    if "device" in engines:
        print(f"# labels searched on the device: {engines['device'].device_searched_labels}; "
              f"on the host engine: {engines['host'].device_searched_labels}")
        # the crossover: the smallest size from which device mode wins front half and wall in EVERY shape measured
        lost = [n for n, w in wins if not w]
        above = [n for n, w in wins if w and n > max(lost, default=0)]
        if above:
            pow2 = 1 << (min(above) - 1).bit_length()
            print(f"# device mode wins both front half and wall in every case from {min(above)} labels on "
                  f"(largest case it does not win: {max(lost, default=0)} labels); rounded up to a power of two: {pow2}")
        else:
            print("# device mode does not win at the largest sizes measured: no crossover")


if __name__ == "__main__":
    main()
